"""UE -> eNB uplink loop on the GPU: srsran_ue_ul_encode's samples through a 3-tap channel, a timing offset and AWGN
at 20 dB (numpy), then the library's own receiver: srsran_ofdm_rx with freq_shift_f = -0.5,
srsran_chest_ul_estimate_pusch and srsran_pusch_decode.  The payload, the CRC and every UCI decision must equal what
was sent, for t2, t4, t6 and t9; eight UEs of two cells go through both batch entry points
(srsran_ue_ul_gpu_tx_batch, srsran_pusch_gpu_decode_batch).  The rv 0 -> rv 2 pair departs from 20 dB on purpose: rv 0
is sent at -1 dB so that its CRC fails and the soft buffer it leaves is what rv 2 (at 10 dB) is combined with."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import pusch as OP  # noqa: E402
import pusch_tx_cases as TC  # noqa: E402
import uci_cases as UC  # noqa: E402

pytestmark = pytest.mark.gpu
SNR_DB = 20.0
TAPS = np.array([1.0, 0.25 * np.exp(1.1j), 0.12 * np.exp(-0.6j)])  # at delays 0, 1, 3 samples
DELAYS = (0, 1, 3)
TIMING = 2  # samples late, inside the cyclic prefix


@pytest.fixture(scope="module")
def env():
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.fail("no HIP device on a GPU test run")
    if not OP.ref_available():
        pytest.fail("oracle/_ref/libsrsref.so missing: the reference checker of this module was not built")
    return OP.PuschOracle()


def channel(x, snr_db):
    """3-tap channel and TIMING samples of delay -> (samples, noise variance snr_db below their mean power)"""
    x = np.asarray(x, np.complex128)
    y = np.zeros_like(x)
    for t, dly in zip(TAPS, DELAYS):
        y[dly + TIMING:] += t * x[:x.size - dly - TIMING]
    return y, np.mean(np.abs(y) ** 2) * 10 ** (-snr_db / 10)


def front_end(c, x, rng, snr_db=SNR_DB):
    """channel, noise and the library's OFDM demodulator (freq_shift_f = -0.5) -> the received grid"""
    from srsran_4g_amd import ue_dl as U
    y, sigma2 = channel(x, snr_db)
    N = x.size // 15
    sigma2 *= N / (12.0 * c["L"])  # the signal sits in 12 L of the N bins: snr_db per RE inside the grant
    y = y + np.sqrt(sigma2 / 2) * (rng.standard_normal(y.size) + 1j * rng.standard_normal(y.size))
    rx = U.OfdmRx(c["nof_prb"], normalize=True, cp=c["cp"], freq_shift_f=-0.5)
    try:
        return rx.rx(y.astype(np.complex64))
    finally:
        rx.free()


def receive(c, cell, d, sf, rx_cfg, x, rng, snr_db=SNR_DB):
    """front end, estimation and decode of one subframe -> (res, data)"""
    from srsran_4g_amd import pusch as P
    grid = front_end(c, x, rng, snr_db)
    ch, pu = P.ChestUl(cell, d, max_prb=c["nof_prb"]), P.Pusch(cell, max_prb=c["nof_prb"])
    try:
        assert ch.estimate(sf, rx_cfg, grid) == 0
        ret, out, data = pu.decode(sf, rx_cfg, ch.res, grid, max(rx_cfg.grant.tb.tbs // 8, 1))
        assert ret == 0
        return out, data
    finally:
        ch.free()
        pu.free()


def check_sent(c, rx_cfg, out, data, payload, u):
    tbs = rx_cfg.grant.tb.tbs
    if tbs:
        assert out.crc and np.array_equal(data[:tbs // 8], payload)
    if c["nack"]:
        assert list(out.uci.ack.ack_value[:c["nack"]]) == list(u.ack.ack_value[:c["nack"]]) and out.uci.ack.valid
    if c["ri"]:
        assert out.uci.ri == u.ri
    if c["cqi"]:
        assert out.uci.cqi.data_crc and UC.cqi_fields(rx_cfg, out.uci.cqi) == UC.cqi_fields(rx_cfg, u.cqi)


@pytest.mark.parametrize("name", ["t2", "t4", "t6", "t9"])
def test_loop_decodes_what_was_sent(env, name):
    from srsran_4g_amd import sch as S
    from srsran_4g_amd import ue_ul as UL
    c = TC.BY_NAME[name]
    cell, d, sf, cfg = TC.make(c)
    payload, u = TC.payload_uci(c, cfg)
    ue = UL.UeUl(cell)
    sb = S.SoftbufferRx(nof_prb=c["nof_prb"])
    try:
        ret, x = ue.encode(sf, TC.ue_cfg(c, cfg, d), payload, u)
        assert ret == 1
        rx_cfg = TC.make(c, softbuffer=sb)[3]
        rx_cfg.max_nof_iterations = 10
        out, data = receive(c, cell, d, sf, rx_cfg, x, np.random.default_rng(500 + c["seed"]))
        check_sent(c, rx_cfg, out, data, payload, u)
    finally:
        ue.free()
        sb.free()


def test_rv0_then_rv2_on_the_kept_soft_buffer(env):
    """t11a (rv 0) at -1 dB: log2(1 + 0.79) = 0.84 bit per symbol is below the 1.08 this grant carries (16QAM at rate
    0.27), so its CRC fails; then t11b (rv 2 of the same payload, re-encoded from the data) at 10 dB on the same soft
    buffer: the two combined decode"""
    from srsran_4g_amd import sch as S
    from srsran_4g_amd import ue_ul as UL
    a, b = TC.BY_NAME["t11a"], TC.BY_NAME["t11b"]
    cell, d, sf, cfg_a = TC.make(a)
    cfg_b = TC.make(b)[3]
    payload, u = TC.payload_uci(a, cfg_a)
    ue = UL.UeUl(cell)
    sb = S.SoftbufferRx(nof_prb=25)
    try:
        xa = ue.encode(sf, TC.ue_cfg(a, cfg_a, d), payload, u)[1].copy()
        xb = ue.encode(sf, TC.ue_cfg(b, cfg_b, d), payload, u)[1].copy()
        assert not np.array_equal(xa, xb)
        rx_a, rx_b = TC.make(a, softbuffer=sb)[3], TC.make(b, softbuffer=sb)[3]
        out, data = receive(a, cell, d, sf, rx_a, xa, np.random.default_rng(61), snr_db=-1.0)
        assert not out.crc
        out, data = receive(b, cell, d, sf, rx_b, xb, np.random.default_rng(62), snr_db=10.0)
        check_sent(b, rx_b, out, data, payload, u)
    finally:
        ue.free()
        sb.free()


def test_batch_of_eight_ues_of_two_cells(env):
    import ctypes

    import torch
    from srsran_4g_amd import pusch as P
    from srsran_4g_amd import sch as S
    from srsran_4g_amd import ue_ul as UL
    names = ["t2", "t9", "t2", "t9", "t9", "t2", "t2", "t9"]  # a 15-PRB and a 25-PRB cell
    ues = {n: UL.UeUl(TC.make(TC.BY_NAME[n])[0]) for n in ("t2", "t9")}
    keep, sent, frees = [], [], []
    try:
        for i, n in enumerate(names):
            c = dict(TC.BY_NAME[n], rnti=0x50 + i, seed=100 + i, name=f"{n}_{i}")
            cell, d, sf, cfg = TC.make(c)
            payload, u = TC.payload_uci(c, cfg)
            ucfg = TC.ue_cfg(c, cfg, d)
            d_pl = torch.from_numpy(np.concatenate([payload, np.zeros(16, np.uint8)])).cuda()
            d_out = torch.zeros(2 * ues[n].sf_len, dtype=torch.float32, device="cuda")
            keep.extend([ucfg, sf, u, d_pl])
            sent.append((c, cell, d, sf, payload, u, d_out, (ues[n], sf, ucfg, u, d_pl.data_ptr(), d_out.data_ptr(), None)))
        assert UL.tx_batch([s[-1] for s in sent]) == 0
        torch.cuda.synchronize()
        # the receive side through its batch entry point as well: one srsran_pusch_gpu_decode_batch over the 8 grids
        n = len(sent)
        arr, res, cres = (P.srsran_pusch_gpu_ue_t * n)(), (P.srsran_pusch_res_t * n)(), (P.srsran_chest_ul_res_t * n)()
        rx_cfgs, datas = [], []
        for i, (c, cell, d, sf, payload, u, d_out, _) in enumerate(sent):
            grid = front_end(c, d_out.cpu().numpy().view(np.complex64), np.random.default_rng(900 + c["seed"]))
            sb, ch = S.SoftbufferRx(nof_prb=c["nof_prb"]), P.ChestUl(cell, d, max_prb=c["nof_prb"])
            d_grid = torch.from_numpy(grid.view(np.float32).reshape(-1).copy()).cuda()
            rx_cfgs.append(TC.make(c, softbuffer=sb)[3])
            datas.append(np.zeros(rx_cfgs[i].grant.tb.tbs // 8 + 64, np.uint8))
            frees.extend([sb, ch])
            keep.append(d_grid)
            arr[i].chest, arr[i].sf, arr[i].cfg = ctypes.pointer(ch.q), ctypes.pointer(sf), ctypes.pointer(rx_cfgs[i])
            arr[i].d_sf_symbols, arr[i].new_data = d_grid.data_ptr(), 1
            res[i].data = datas[i].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        pu = P.Pusch(sent[0][1])
        frees.append(pu)
        assert P.lib().srsran_pusch_gpu_decode_batch(ctypes.byref(pu.q), n, arr, cres, res) == 0
        for i, (c, cell, d, sf, payload, u, d_out, _) in enumerate(sent):
            check_sent(c, rx_cfgs[i], res[i], datas[i], payload, u)
    finally:
        for x in list(ues.values()) + frees:
            x.free()
