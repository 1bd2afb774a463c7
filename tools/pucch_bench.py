"""Time one srsran_pucch_gpu_get_batch over 256 entries of a 50-PRB cell: 100 x format 1a, 100 x SR + 1b (two
passes), 40 x format 2 and 16 x format 3, grids already on the device.  Median of 20 calls after 3 warm-up calls:
wall time of the call (it returns with the results on the host, so this includes the descriptor upload, the launch
and the result copy) and the time between two device events recorded around it.  Writes profiles/pucch_batch.json.

    python tools/pucch_bench.py
"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pucch_cases as C  # noqa: E402
import pucch_tx as T  # noqa: E402
from srsran_4g_amd import pucch as P  # noqa: E402
from srsran_4g_amd import pusch as PU  # noqa: E402
from srsran_4g_amd.ue_dl import cell as make_cell  # noqa: E402


def mix():
    return ([dict(nof_prb=50, acks=[[1, 0, 0, 0]], N_pucch_1=i % 36) for i in range(100)] +
            [dict(nof_prb=50, acks=[[2, 0, 0, 0]], sr_tti=1, n_pucch_sr=40 + i % 30, N_pucch_1=i % 36) for i in range(100)] +
            [dict(nof_prb=50, cqi=[0, 0, 0], n_pucch_2=i % 12) for i in range(40)] +
            [dict(nof_prb=50, mode=2, acks=[[2, 0, 0, 0], [2, 0, 1, 0]], n3=[5 * (i % 4)] * 4) for i in range(16)])


def main():
    cell = make_cell(50, 1, 1)
    chest = PU.ChestUl(cell, PU.srsran_refsignal_dmrs_pusch_cfg_t(), max_prb=50)
    pucch = P.Pucch(cell)
    rng = np.random.default_rng(5)
    # one subframe: a format 1a UE on resource 0 and a format 2 UE on resource 0 of its PRB, 10 dB
    g = T.encode(T.Res(T.F1A, 0), 50, 1, 0, 0, bits=[1]) + T.encode(T.Res(T.F2, 12 * 2), 50, 1, 0, 0, bits=[1, 0, 1, 1])
    g = g + np.sqrt(0.05) * (rng.standard_normal(g.shape) + 1j * rng.standard_normal(g.shape))
    d_grid = torch.from_numpy(g.astype(np.complex64).view(np.float32).copy()).cuda()
    specs = mix()
    sfs = [C.build_sf(s) for s in specs]
    wall, dev = [], []
    ncand = 100 + 100 * 2 + 40 + 16
    for it in range(23):
        cfgs = [C.build_cfg(C.full(s)) for s in specs]  # fresh: the call writes them
        n = len(specs)
        ues = (P.srsran_pucch_gpu_ue_t * n)()
        res = (P.srsran_pucch_res_t * n)()
        for i in range(n):
            ues[i].chest, ues[i].sf, ues[i].cfg = ctypes.pointer(chest.q), ctypes.pointer(sfs[i]), ctypes.pointer(cfgs[i])
            ues[i].d_sf_symbols = d_grid.data_ptr()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        ret = P.lib().srsran_pucch_gpu_get_batch(ctypes.byref(pucch.q), n, ues, res)
        t1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        assert ret == 0
        if it >= 3:
            wall.append((t1 - t0) * 1e6)
            dev.append(e0.elapsed_time(e1) * 1e3)
    out = dict(entries=len(specs), candidates=ncand, cell_prb=50, calls=len(wall), warmup=3,
               wall_us_median=statistics.median(wall), wall_us_min=min(wall), wall_us_max=max(wall),
               event_us_median=statistics.median(dev),
               note="the call is host-synchronous: wall covers descriptor build and upload, launch, result copy and the pick",
               detected=int(sum(bool(r.detected) for r in res)))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pucch_batch.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    pucch.free()
    chest.free()


if __name__ == "__main__":
    main()
