"""The GPU eNB's PBCH read back by the GPU UE's MIB decoder: srsran_enb_dl with put_base transmits subframe 0 of
consecutive radio frames, the samples pass through a multipath channel with AWGN, and srsran_ue_mib_decode with
nof_ports = 0 must return the eNB's bandwidth, PHICH configuration, port count and the SFN of the frame just received,
(unpacked sfn + sfn_offset) mod 1024, starting at each of the four positions of the 40 ms period -- as srsUE's
sfn_sync does (srsue/src/phy/sfn_sync.cc:59-137).

The SNR is not tuned on the decoder.  The test's own numpy model (an FFT of the noise-free samples and of the noise at
the PBCH symbols' windows) gives the SNR of every one of the 240 / 216 PBCH REs and from it the raw error rate of the
QPSK soft bits, mean Q(sqrt(SNR_k)); the test requires it below RAW_BER_MAX = 2 %.  One frame carries the 40 coded
bits 12 times over (480 soft bits), and the fixtures' low-SNR cases show the reference decoding a single frame down to
about -8 dB per RE, a raw error rate above 30 %: 2 % leaves the decision a margin that float rounding cannot touch."""
import math

import numpy as np
import pytest
import torch

from srsran_4g_amd import enb_dl as E
from srsran_4g_amd import pbch as B
from srsran_4g_amd import ue_dl as U

pytestmark = pytest.mark.gpu
SNR_DB = 10.0  # per sample, relative to the mean power of the almost empty subframe 0
RAW_BER_MAX = 0.02
TAPS = ((0, 1.0), (2, 0.35j), (5, -0.2))

CELLS = [
    dict(name="p25_2p", nof_prb=25, ports=2, cell_id=150, cp=0, phich_res=2, phich_len=0),
    dict(name="p6_1p", nof_prb=6, ports=1, cell_id=301, cp=0, phich_res=1, phich_len=1),
    dict(name="p50_4p_ext", nof_prb=50, ports=4, cell_id=503, cp=1, phich_res=3, phich_len=0),
]


def transmit(cell, sfns):
    enb = E.EnbDl(cell)
    N = U.lib().srsran_symbol_sz(cell.nof_prb)
    d_tx = torch.zeros((len(sfns), cell.nof_ports, 15 * N, 2), dtype=torch.float32, device="cuda")
    assert enb.tx_batch([(10 * s, 1, None, [], (True, [])) for s in sfns], d_tx.data_ptr()) == 0
    torch.cuda.synchronize()
    tx = d_tx.cpu().numpy().view(np.complex64)[..., 0]
    enb.free()
    return tx, N


def multipath(tx):
    F, P, n = tx.shape
    y = np.zeros((F, n), np.complex128)
    for p in range(P):
        for d, a in TAPS:
            y += a * np.exp(0.7j * p * (d + 1)) * np.roll(tx[:, p].astype(np.complex128), d, axis=1)
    return y


def pbch_re_snr(clean, noise, N, ext, cell_id):
    """SNR of the PBCH REs (the 72 centre subcarriers of slot 1's symbols 0..3 without the REs reserved for CRS,
    k mod 3 = cell id mod 3 in symbols 0, 1 and, with the extended CP, 3; the centre starts at a multiple of 6):
    |FFT of the clean samples|^2 over the mean |FFT of the noise|^2 on the same windows"""
    bins = np.r_[np.arange(N - 36, N), np.arange(1, 37)]
    snr = []
    for l in range(4):
        if ext:
            cp = N // 4
            start = 6 * (N + cp) + l * (N + cp) + cp
        else:
            cp0, cp = 160 * N // 2048, 144 * N // 2048
            start = (7 * N + cp0 + 6 * cp) + cp0 + l * (N + cp)
        s = np.fft.fft(clean[start:start + N])[bins]
        w = np.fft.fft(noise[:, start:start + N], axis=1)[:, bins]
        v = np.abs(s) ** 2 / np.mean(np.abs(w) ** 2)
        if l < 2 or (l == 3 and ext):
            v = v[np.arange(72) % 3 != cell_id % 3]
        snr.append(v)
    return np.concatenate(snr)


@pytest.mark.parametrize("cfg", CELLS, ids=lambda c: c["name"])
def test_ue_reads_the_enbs_mib(cfg):
    cell = U.cell(cfg["nof_prb"], cfg["ports"], cfg["cell_id"], phich_res=cfg["phich_res"], cp=cfg["cp"],
                  phich_len=cfg["phich_len"])
    rng = np.random.default_rng(cfg["cell_id"])
    sfns = [(1020 + i) % 1024 for i in range(8)]  # across the SFN wrap; starts at positions 0..3 below
    tx, N = transmit(cell, sfns)
    clean = multipath(tx)
    sigma2 = np.mean(np.abs(clean) ** 2) * 10.0 ** (-SNR_DB / 10.0)
    w = np.sqrt(sigma2 / 2.0) * (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape))
    # the margin condition on the numpy model, before the decoder sees anything
    snr = pbch_re_snr(clean[0], w, N, bool(cfg["cp"]), cfg["cell_id"])
    raw_ber = float(np.mean([0.5 * math.erfc(math.sqrt(s / 2.0)) for s in snr if s > 0]))
    print("%s: PBCH RE SNR median %.1f dB, modelled raw bit error rate %.4f" % (
        cfg["name"], 10 * np.log10(np.median(snr[snr > 0])), raw_ber))
    assert raw_ber <= RAW_BER_MAX
    rx = (clean + w).astype(np.complex64)
    mib = B.UeMib(U.cell(cfg["nof_prb"], 0, cfg["cell_id"], cp=cfg["cp"]))
    for start in range(4):
        mib.reset()
        for i in range(start, start + 3):
            ret, pl, nports, off = mib.decode(rx[i])
            assert ret == 1, (start, i)  # every clean frame decodes on its own; the history is reset each time
            prb, plen, pres, sfn = B.mib_unpack(pl)
            assert (prb, plen, pres, nports) == (cfg["nof_prb"], cfg["phich_len"], cfg["phich_res"], cfg["ports"])
            assert (sfn + off) % 1024 == sfns[i], (start, i, sfn, off)
            assert off == sfns[i] % 4 and mib.q.frame_cnt == 0 and mib.q.pbch.frame_idx == 0
    mib.free()
