"""Time the two PHICH batch calls on a 100-PRB, Ng = 2 cell (25 groups): a transmit batch of 200 items, every
sequence of every group of one subframe, and a receive batch of the same 200 resources on device grids and
estimates.  Each sample is the time between two device events on one stream around LOOP back-to-back calls, divided
by LOOP: it covers the library's staging of the items (validation, grouping), their upload and the one launch, as a
caller that keeps the stream busy sees them; the item array is built once, outside the timed calls.  Median and
spread of REPS samples after WARMUP calls.  Writes profiles/phich_batch.json.

    python tools/phich_bench.py
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srsran_4g_amd import pdcch as PD  # noqa: E402
from srsran_4g_amd import phich as PH  # noqa: E402

NPRB, GROUPS, NSEQ, LOOP, REPS, WARMUP = 100, 25, 8, 50, 20, 5


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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("phich_bench: no HIP device")
    out = []
    for ports, nrx in ((1, 1), (2, 2), (4, 2)):
        cell = PD.cell(NPRB, ports, 150, phich_res=3)
        regs = PD.Regs(cell)
        ph = PH.Phich(cell, regs, nrx)
        assert ph.ngroups() == GROUPS
        n = 14 * 12 * NPRB
        rng = np.random.default_rng(5)
        sent = [(0, 4, g, s, int(rng.integers(0, 2))) for g in range(GROUPS) for s in range(NSEQ)]
        items = PH.make_items(sent)
        d_tx = torch.zeros((1, ports, n, 2), dtype=torch.float32, device="cuda")
        tx = timed(lambda st: ph.encode_batch(items, 1, d_tx.data_ptr(), st))
        torch.cuda.synchronize()
        # receive: the transmitted grids through a flat channel per (port, rx), estimates exact
        h = (rng.standard_normal((ports, nrx)) + 1j * rng.standard_normal((ports, nrx))).astype(np.complex64)
        grid = d_tx.cpu().numpy().view(np.complex64).reshape(ports, n)
        rx = np.einsum("pr,pk->rk", h, grid).astype(np.complex64)
        ce = np.broadcast_to(h[:, :, None], (ports, nrx, n)).astype(np.complex64)
        d_rx = torch.from_numpy(rx.view(np.float32).copy()).cuda()
        d_ce = torch.from_numpy(ce.view(np.float32).copy()).cuda()
        d_noise = torch.zeros(4, dtype=torch.float32, device="cuda")
        d_res = torch.zeros((len(items), 2), dtype=torch.float32, device="cuda")
        rxt = timed(lambda st: ph.decode_batch(items, 1, d_rx.data_ptr(), d_ce.data_ptr(), n, d_noise.data_ptr(), 4,
                                               d_res.data_ptr(), st))
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(PH.RES_DTYPE).ravel()
        assert np.array_equal(res["ack_value"], np.array([i[4] for i in sent], np.uint32))  # what was sent comes back
        out.append(dict(cell_prb=NPRB, ports=ports, nof_rx=nrx, groups=GROUPS, items=len(items), loop=LOOP, reps=REPS,
                        warmup=WARMUP, transmit=tx, receive=rxt,
                        # what the launches move: 12 REs a port per unit written; 12 REs a (rx, port x rx) read per item
                        tx_bytes_written=GROUPS * 12 * ports * 8, rx_bytes_read=len(items) * 12 * nrx * (1 + ports) * 8))
        ph.free()
        regs.free()
    res = dict(note="us_per_call: device-event time around LOOP back-to-back calls on one stream, divided by LOOP; a "
                    "call stages and uploads its items and enqueues one launch (25 workgroups transmit, 200 receive)",
               runs=out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "phich_batch.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
