"""Time PRACH detection of a 100-PRB cell at N = 1536 and N = 2048 with zero_corr_zone 1 (one root, 64 windows) and
0 (64 roots): one srsran_prach_gpu_detect_batch over 16 occasions whose signals are already on the device, and the
host-synchronous srsran_prach_detect_offset of one occasion from host memory.  Median of 20 calls after 3 warm-up
calls: wall time of the call (both return with the results on the host, after a device synchronise, so this includes
the descriptor or sample upload, the two launches, the record copy and the host's threshold pass) and the time
between two device events recorded on the object's own stream around the two kernels (srsran_prach_gpu_detect_time;
the uploads and the record copy lie outside that pair).  Writes profiles/prach_batch.json.

    python tools/prach_bench.py
"""
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

import prach_np as R  # noqa: E402
from srsran_4g_amd import prach as P  # noqa: E402
from srsran_4g_amd import ue_dl as U  # noqa: E402

NOCC, CALLS, WARMUP = 16, 20, 3


def timed(p, fn):
    """wall time with the event hook off, then the kernels' event time in calls of their own with it on"""
    wall, dev, last = [], [], None
    for it in range(CALLS + WARMUP):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        t1 = time.perf_counter()
        if it >= WARMUP:
            wall.append((t1 - t0) * 1e6)
    p.detect_time(True)
    for it in range(CALLS + WARMUP):
        fn()
        us = p.detect_time(True)
        assert us > 0
        if it >= WARMUP:
            dev.append(us)
    p.detect_time(False)
    return dict(wall_us_median=statistics.median(wall), wall_us_min=min(wall), wall_us_max=max(wall),
                kernels_event_us_median=statistics.median(dev), kernels_event_us_min=min(dev),
                kernels_event_us_max=max(dev)), last


def main():
    out = []
    for standard in (False, True):
        U.use_standard_symbol_size(standard)
        N = U.symbol_sz_for(100)
        for zczc in (1, 0):
            p = P.Prach(2048).configure(P.cfg(0, 22, zczc), 100)
            p.set_detect_factor(60)
            ref = R.Params(N, 0, 22, zczc, standard=standard)
            sigs = [R.channel(ref, [((5 * k + 3) % 64, 1.0, k), ((9 * k + 40) % 64, 0.7, 2 * k)], 4, -10.0, 50 + k)
                    for k in range(NOCC)]
            dev = [torch.from_numpy(x.view(np.float32)).cuda() for x in sigs]
            entries = [(p, 4, d.data_ptr(), ref.M) for d in dev]
            tb, (ret, res, _) = timed(p, lambda: P.detect_batch(entries))
            assert ret == 0
            th, one = timed(p, lambda: p.detect_offset(4, sigs[0]))
            assert one[0] == 0 and np.array_equal(one[1], res[0][0])
            roots = p.q.num_ra_preambles
            out.append(dict(cell_prb=100, N=N, zero_corr_zone=zczc, roots=roots, occasions=NOCC, calls=CALLS, warmup=WARMUP,
                            batch=tb, host_sync_one_occasion=th, detected=int(sum(len(r[0]) for r in res)),
                            # algorithmic work of the batch: samples read once, 12 N-point FFTs (5 N log2 N flops each),
                            # the 12-term combine, and 839^2 complex MACs (8 flops) per root
                            bytes_in=NOCC * ref.M * 8,
                            flops=int(NOCC * (12 * 5 * N * np.log2(N) + 12 * 839 * 8 + roots * 839 * 839 * 8))))
            p.free()
    U.use_standard_symbol_size(False)
    res = dict(note="both calls are host-synchronous: wall covers upload, the two launches, the record copy and the "
                    "host's threshold pass; kernels_event_us is the time between events on the object's stream around the "
                    "two kernels alone, taken in separate calls",
               runs=out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "prach_batch.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
