"""Time srsran_ue_ul_gpu_tx_batch: batches of 1, 16 and 200 UE subframes with L = 6 (25-PRB cell, 16QAM, TBS 936) and
L = 100 (100-PRB cell, 64QAM, TBS 61664), grid only (d_out = NULL: TB encode, multiplexing, transform precoding +
DMRS) and through to samples (OFDM modulation and normalisation as well).  Each sample is the time between two device
events on one stream around LOOP back-to-back calls, divided by LOOP: it covers the host part of every call (the UCI /
segmentation planning, the DMRS sequences computed on the host, the descriptor upload) and its launches, as a caller
that keeps the stream busy sees them.  Median and spread of REPS samples after WARMUP calls.  Writes
profiles/pusch_tx_batch.json.

    python tools/pusch_tx_bench.py [--out FILE]

Per-stage kernel times come from a kernel trace taken in a run of its own (tracing slows the host, so the figures above
are taken with the profiler off) and are merged into the file afterwards:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tx -- python tools/pusch_tx_bench.py --only 100:200 --out /dev/null
    python tools/pusch_tx_bench.py --merge-kernel-stats DIR/.../tx_kernel_stats.csv --only 100:200 [--out FILE]
"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pusch_tx as TX  # noqa: E402  (tests/pusch_tx.py: make_cfg)
from srsran_4g_amd import pusch as P  # noqa: E402
from srsran_4g_amd import ue_ul as UL  # noqa: E402
from srsran_4g_amd.ue_dl import cell as make_cell  # noqa: E402

LOOP, REPS, WARMUP = 10, 15, 3
SHAPES = [(25, 6, 4, 936), (100, 100, 6, 61664)]  # (cell PRB, L_prb, Qm, TBS)
BATCHES = (1, 16, 200)


def timed(fn):
    stream = torch.cuda.current_stream()
    for _ in range(WARMUP):
        assert fn(stream.cuda_stream) == 0
    torch.cuda.synchronize()
    us = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(LOOP):
            fn(stream.cuda_stream)
        b.record(stream)
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / LOOP)
    return dict(us_per_call_median=statistics.median(us), us_per_call_min=min(us), us_per_call_max=max(us))


STAGES = ("enc_tb_crc_kernel", "enc_cb_kernel", "pusch_tx_mux_kernel", "pusch_tx_grid_kernel", "ofdm_tx_kernel",
          "ofdm_tx_post_kernel", "pusch_tx_norm_kernel")


def merge_kernel_stats(path, only, out):
    """the average time per launch of every transmit-stage kernel in a rocprofv3 --stats table -> out's "kernel_trace"""
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        for st in STAGES:
            if st in name:
                e = rows.setdefault(st, dict(calls=0, total_ns=0.0))
                e["calls"] += int(r["Calls"])
                e["total_ns"] += float(r["TotalDurationNs"])
    res = json.load(open(out))
    res["kernel_trace"] = dict(shape=only, note="rocprofv3 --kernel-trace --stats of the tool restricted to this shape "
                               "(cell PRB : UEs; L = cell PRB for 100, else 6); average per launch over every call of the "
                               "run, grid-only and to-samples batches alike",
                               kernels={k: dict(calls=v["calls"], avg_us_per_launch=v["total_ns"] / v["calls"] / 1e3)
                                        for k, v in rows.items()})
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pusch_tx_batch.json"))
    ap.add_argument("--only", default=None, help="CELL_PRB:UES -- run (or label) that one configuration")
    ap.add_argument("--merge-kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv to merge into --out")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.only, args.out)
    only = tuple(int(v) for v in args.only.split(":")) if args.only else None
    if not torch.cuda.is_available():
        raise SystemExit("pusch_tx_bench: no HIP device")
    rng = np.random.default_rng(11)
    runs = []
    for nprb, L, Qm, tbs in SHAPES:
        if only and nprb != only[0]:
            continue
        cell = make_cell(nof_prb=nprb, cell_id=57)
        ue = UL.UeUl(cell)
        d = P.srsran_refsignal_dmrs_pusch_cfg_t()
        d.group_hopping_en = True
        for n in BATCHES:
            if only and n != only[1]:
                continue
            keep, ent = [], {"grid": [], "samples": []}
            for i in range(n):
                cfg = TX.make_cfg(nprb, Qm, L, 0 if L == nprb else 3 + (i % 4), tbs, rnti=0x100 + i)
                u = UL.srsran_ue_ul_cfg_t()
                u.ul_cfg.pusch, u.ul_cfg.dmrs, u.grant_available = cfg, d, True
                sf = P.srsran_ul_sf_cfg_t()
                sf.tti = i % 10
                d_pl = torch.from_numpy(rng.integers(0, 256, tbs // 8 + 16, dtype=np.uint8)).cuda()
                d_out = torch.zeros(2 * ue.sf_len, dtype=torch.float32, device="cuda")
                keep.extend([u, sf, d_pl, d_out])
                ent["grid"].append((ue, sf, u, None, d_pl.data_ptr(), None, None))
                ent["samples"].append((ue, sf, u, None, d_pl.data_ptr(), d_out.data_ptr(), None))
            res = {k: timed(lambda st, e=e: UL.tx_batch(e, st)) for k, e in ent.items()}
            torch.cuda.synchronize()
            assert float(keep[3].abs().max()) > 0
            M, nsym = 12 * L, 12
            runs.append(dict(cell_prb=nprb, L_prb=L, Qm=Qm, tbs=tbs, ues=n, loop=LOOP, reps=REPS, warmup=WARMUP,
                             grid_only=res["grid"], to_samples=res["samples"],
                             # what the stages move per call: one byte a coded bit in and out of the multiplexer, 8 B a
                             # symbol, the grid written once and read once by the modulator, the samples three times
                             bytes_mux=n * (2 * nsym * M * Qm + 8 * nsym * M),
                             bytes_grid=n * (8 * nsym * M + 8 * 14 * 12 * nprb),
                             bytes_samples=n * 8 * (14 * 12 * nprb + 4 * ue.sf_len)))
        ue.free()
    res = dict(note="us_per_call: device-event time around LOOP back-to-back srsran_ue_ul_gpu_tx_batch calls on one "
                    "stream, divided by LOOP; host planning and uploads included; kernel_trace (when present): a "
                    "kernel trace of one configuration taken in a run of its own",
               runs=runs)
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
