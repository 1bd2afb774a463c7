"""Time the UE's PUCCH transmit over the 256-entry mix the receive side is measured on (tools/pucch_bench.py): 100 x
format 1a, 100 x SR + 1b, 40 x format 2 and 16 x format 3 of a 50-PRB cell, samples and grids left on the device.
Once as one srsran_ue_ul_gpu_tx_batch, once as 256 single-entry calls.  Median of 20 repetitions after 3 warm-up
repetitions: the time between two device events recorded around the call(s), and the host wall time until the
stream has drained.  Writes profiles/pucch_tx_batch.json (or the path given).

    python tools/pucch_tx_bench.py [out.json]
"""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pucch_cases as C  # noqa: E402
from srsran_4g_amd import ue_ul as UL  # noqa: E402
from srsran_4g_amd.sch import srsran_uci_value_t  # noqa: E402
from srsran_4g_amd.ue_dl import cell as make_cell  # noqa: E402


def mix():
    """(case, what the UE sends)"""
    return ([(dict(nof_prb=50, acks=[[1, 0, 0, 0]], N_pucch_1=i % 36), dict(ack=[i % 2])) for i in range(100)] +
            [(dict(nof_prb=50, acks=[[2, 0, 0, 0]], sr_tti=1, n_pucch_sr=40 + i % 30, N_pucch_1=i % 36),
              dict(sr=1, ack=[i % 2, 1])) for i in range(100)] +
            [(dict(nof_prb=50, cqi=[0, 0, 0], n_pucch_2=i % 12), dict(cqi=[i % 16, 0, 0])) for i in range(40)] +
            [(dict(nof_prb=50, mode=2, acks=[[2, 0, 0, 0], [2, 0, 1, 0]], n3=[5 * (i % 4)] * 4),
              dict(ack=[1, 0, i % 2, 1])) for i in range(16)])


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pucch_tx_batch.json")
    ue = UL.UeUl(make_cell(50, 1, 1))
    specs = mix()
    n = len(specs)
    d_out = torch.zeros((n, 2 * ue.sf_len), dtype=torch.float32, device="cuda")
    sfs = [C.build_sf(dict(tti=i % 10)) for i in range(n)]
    vals = [C.build_uci_value(tx, srsran_uci_value_t) for _, tx in specs]

    def entries():
        cfgs = []
        for s, _ in specs:  # fresh: the call writes format / n_pucch
            u = UL.srsran_ue_ul_cfg_t()
            c = C.build_cfg(C.full(s))
            ctypes.memmove(ctypes.byref(u.ul_cfg.pucch), ctypes.byref(c), ctypes.sizeof(c))
            cfgs.append(u)
        return cfgs, [(ue, sfs[i], cfgs[i], vals[i], None, d_out[i].data_ptr(), None) for i in range(n)]

    res = {}
    for label in ("batch", "single"):
        wall, dev = [], []
        for it in range(23):
            cfgs, es = entries()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            if label == "batch":
                assert UL.tx_batch(es) == 0
            else:
                for e in es:
                    assert UL.tx_batch([e]) == 0
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if it >= 3:
                wall.append((t1 - t0) * 1e6)
                dev.append(e0.elapsed_time(e1) * 1e3)
        res[label] = dict(event_us_median=statistics.median(dev), event_us_min=min(dev), event_us_max=max(dev),
                          wall_us_median=statistics.median(wall))
        formats = sorted({c.ul_cfg.pucch.format for c in cfgs})
    assert float(d_out.abs().amax(dim=1).min()) > 0  # every entry produced samples
    out = dict(entries=n, cell_prb=50, repetitions=20, warmup=3, formats=formats, batch=res["batch"], single_calls=res["single"],
               note="wall includes the Python entry building of ctypes arrays inside tx_batch and the host-side descriptor work")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    ue.free()


if __name__ == "__main__":
    main()
