"""Time srsran_sch_nr_gpu_encode_batch next to its receiver on the shape DESIGN 4.3 quotes: 64 full-carrier NR TBs
(273 PRB, 256QAM, R 948/1024, 1 layer), new transmissions (rv 0).  In the same run the receiver
(srsran_sch_nr_gpu_decode_batch, new data every call) decodes the noise-free output of that encode, LLR = 10 (1 - 2 bit),
which stops every code block after one iteration.  Each sample is the time between two device events on one stream
around LOOP back-to-back calls, divided by LOOP: it covers the host part of every call (TB info, descriptors, upload)
and its launches, as a caller that keeps the stream busy sees them.  Encode and decode samples alternate; median and
spread of REPS samples each, after WARMUP calls.  Writes profiles/nr_sch_tx.json.

    python tools/nr_sch_tx_bench.py [--out FILE] [--tbs N]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from srsran_4g_amd import sch_nr as S  # noqa: E402
from synth.nr_tx import aligned_tbs  # noqa: E402

LOOP, REPS, WARMUP = 50, 11, 5
NR_PRB, NR_QM, NR_R = 273, 8, 948.0 / 1024.0
NR_NRE = 12 * 12 * NR_PRB


def sample(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(LOOP):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / LOOP


def stats(us):
    return dict(us_per_call_median=statistics.median(us), us_per_call_min=min(us), us_per_call_max=max(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nr_sch_tx.json"))
    ap.add_argument("--tbs", type=int, default=64, help="transport blocks per call")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nr_sch_tx_bench: no HIP device")
    ntb = args.tbs
    tbs = aligned_tbs(NR_NRE, NR_R, NR_QM, 1)
    G = NR_NRE * NR_QM
    t = S.tb_info(tbs, NR_R, NR_QM, G, 1, nof_prb=NR_PRB, mcs256=True)
    rng = np.random.default_rng(5)
    pl = rng.integers(0, 256, (ntb, tbs // 8)).astype(np.uint8)
    d_pl = torch.from_numpy(pl).cuda()
    d_e = torch.zeros((ntb, G), dtype=torch.uint8, device="cuda")
    d_llr = torch.zeros((ntb, G), dtype=torch.int8, device="cuda")
    d_out = torch.zeros((ntb, tbs // 8 + 8), dtype=torch.uint8, device="cuda")
    d_crc = torch.zeros(ntb, dtype=torch.uint8, device="cuda")
    d_avg = torch.zeros(ntb, dtype=torch.float32, device="cuda")
    tx = S.SchNr(nof_prb=NR_PRB, tx=True)
    rx = S.SchNr(nof_prb=NR_PRB, scaling=0.8, max_nof_iter=10)
    sbtx = S.nr_softbuffer_tx(max_cb=t.C)
    sbrx = [S.SoftbufferRx(max_cb=t.C, max_cb_size=S.MAX_CB_SIZE) for _ in range(ntb)]
    cfg = S.make_cfg(mcs256=True)
    tbt = [S.make_tb(tbs, NR_R, NR_QM, G, 1, 0, sbtx) for _ in range(ntb)]
    tbr = [S.make_tb(tbs, NR_R, NR_QM, G, 1, 0, sb) for sb in sbrx]
    enc = (S.srsran_sch_nr_gpu_enc_t * ntb)()
    dec = (S.srsran_sch_nr_gpu_tb_t * ntb)()
    for i in range(ntb):
        enc[i].sch_cfg, enc[i].tb = S.ctypes.pointer(cfg), S.ctypes.pointer(tbt[i])
        enc[i].d_payload, enc[i].d_e_bits = d_pl[i].data_ptr(), d_e[i].data_ptr()
        dec[i].sch_cfg, dec[i].tb = S.ctypes.pointer(cfg), S.ctypes.pointer(tbr[i])
        dec[i].d_e_bits, dec[i].d_payload, dec[i].new_data = d_llr[i].data_ptr(), d_out[i].data_ptr(), 1
    L = S.lib()
    stream = torch.cuda.current_stream()
    sp = stream.cuda_stream

    def encode():
        if L.srsran_sch_nr_gpu_encode_batch(S.ctypes.byref(tx.q), ntb, enc, sp):
            raise RuntimeError("srsran_sch_nr_gpu_encode_batch failed")

    def decode():
        if L.srsran_sch_nr_gpu_decode_batch(S.ctypes.byref(rx.q), ntb, dec, d_crc.data_ptr(), d_avg.data_ptr(), sp):
            raise RuntimeError("srsran_sch_nr_gpu_decode_batch failed")

    encode()
    d_llr.copy_((10 - 20 * d_e.to(torch.int16)).to(torch.int8))  # noise-free: bit 1 -> -10
    for _ in range(WARMUP):
        encode()
        decode()
    torch.cuda.synchronize()
    us_e, us_d = [], []
    for _ in range(REPS):
        us_e.append(sample(encode, stream))
        us_d.append(sample(decode, stream))
    torch.cuda.synchronize()
    ok = bool((d_crc == 1).all()) and np.array_equal(d_out.cpu().numpy()[:, : tbs // 8], pl)
    avg = d_avg.cpu().numpy()
    e, d = stats(us_e), stats(us_d)
    res = dict(note="us_per_call: device-event time around LOOP back-to-back calls on one stream, divided by LOOP; host "
                    "planning and descriptor uploads included; encode and decode samples alternate in one run",
               shape=f"{ntb} TBs x {tbs} bits (273 PRB, 256QAM, R 948/1024, 1 layer, G={G}; BG{t.bg + 1} Z={t.Z}, "
                     f"C={t.C}), rv 0",
               loop=LOOP, reps=REPS, warmup=WARMUP,
               encode=dict(e, gbit_per_s=ntb * tbs / e["us_per_call_median"] / 1e3),
               decode_noise_free=dict(d, gbit_per_s=ntb * tbs / d["us_per_call_median"] / 1e3,
                                      avg_iterations=float(avg.mean()), max_nof_iter=10),
               loop_payloads_equal_and_crc_ok=ok,
               encode_over_decode=e["us_per_call_median"] / d["us_per_call_median"],
               # payload bytes in, one byte per rate-matched bit out
               encode_bytes=ntb * (tbs // 8 + G))
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if not ok:
        raise SystemExit("nr_sch_tx_bench: the loop did not return the payloads")


if __name__ == "__main__":
    main()
