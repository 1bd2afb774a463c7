"""Time the PBCH decoder's batch call: 64 objects with nof_ports = 0 (ports 1, 2, 4 searched) on 25-PRB cells of
different ids, each receiving noise, so that after three calls every object holds three stored frames and each further
call is the full case: four frames, 30 hypotheses a port count, 90 an object, 5760 a batch, all missing, the history
shifted.  Timed between two device events on one stream around LOOP back-to-back calls, divided by LOOP:
  batch:  one srsran_pbch_gpu_decode_batch of the 64 entries (three launches);
  single: the same 64 entries as 64 one-entry calls (192 launches).
A call covers the library's staging of the entries, their upload and the launches, as a caller that keeps the stream
busy sees them; the entry arrays are built once.  Median and spread of REPS samples after WARMUP calls.  Writes
profiles/pbch_batch.json.

    python tools/pbch_bench.py
"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srsran_4g_amd import pbch as B  # noqa: E402
from srsran_4g_amd import ue_dl as U  # noqa: E402

NPRB, NOBJ, LOOP, REPS, WARMUP = 25, 64, 20, 20, 5


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
        raise SystemExit("pbch_bench: no HIP device")
    n = 14 * 12 * NPRB
    rng = np.random.default_rng(5)
    objs = [B.Pbch(U.cell(NPRB, 0, 3 * i + i % 3)) for i in range(NOBJ)]
    grid = (rng.standard_normal((NOBJ, n)) + 1j * rng.standard_normal((NOBJ, n))).astype(np.complex64)
    ce = (rng.standard_normal((NOBJ, 4, n)) + 1j * rng.standard_normal((NOBJ, 4, n))).astype(np.complex64)
    d_grid = torch.from_numpy(grid.view(np.float32)).cuda()
    d_ce = torch.from_numpy(ce.view(np.float32)).cuda()
    d_noise = torch.ones(NOBJ, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(NOBJ * B.RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ents = [o.entry(d_grid[i].data_ptr(), d_ce[i].data_ptr(), n, 1, d_noise[i:].data_ptr()) for i, o in enumerate(objs)]
    arr = (B.srsran_pbch_gpu_entry_t * NOBJ)(*ents)
    ones = [(B.srsran_pbch_gpu_entry_t * 1)(e) for e in ents]
    L = B.lib()
    step = B.RES_DTYPE.itemsize

    def batch(st):
        return L.srsran_pbch_gpu_decode_batch(NOBJ, arr, d_out.data_ptr(), st)

    def single(st):
        r = 0
        for i in range(NOBJ):
            r |= L.srsran_pbch_gpu_decode_batch(1, ones[i], d_out.data_ptr() + i * step, st)
        return r

    tb = timed(batch)
    ts = timed(single)
    torch.cuda.synchronize()
    res = d_out.cpu().numpy().view(B.RES_DTYPE)
    idx = [o.last_llr()[1] for o in objs]
    assert not res["found"].any() and idx == [3] * NOBJ, "noise decoded, or the history is not full"
    for o in objs:
        o.free()
    out = dict(note="us_per_call: device-event time around LOOP back-to-back calls on one stream, divided by LOOP; "
                    "batch = one call of 64 entries (3 launches, 5760 hypothesis workgroups), single = the same "
                    "entries as 64 one-entry calls (192 launches)",
               cell_prb=NPRB, objects=NOBJ, hypotheses_per_object=B.NOF_HYP, loop=LOOP, reps=REPS, warmup=WARMUP,
               batch=tb, single=ts)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pbch_batch.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
