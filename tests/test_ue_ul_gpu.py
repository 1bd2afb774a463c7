"""srsran_ue_ul_encode on the GPU (ue_ul.c:246-351, 618-659): the subframe's samples against a float64 model on the
library's own grid (read back through srsran_ue_ul_gpu_last): oracle/ofdm_np.ofdm_tx_opts with freq_shift = 0.5 and
normalize = true, ofdm_np.ref_apply_cfo (the reference's srsran_vec_apply_cfo), and apply_norm's factor written out.
Bound: the 2e-6 of the largest sample that tests/test_ofdm_opts_gpu.py applies to its modulator cases (TOL there): it
is the same modulator; the CFO product and the scale add two float roundings, which that bound already covers for
the option tables.  Both normalize modes, cfo_en on and off, the 0.1 floor (t1: a 6-PRB cell starts from factor 0),
the no-grant branch."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import ofdm_np  # noqa: E402
import pusch as OP  # noqa: E402
import pusch_tx_cases as TC  # noqa: E402
from test_ofdm_opts_gpu import TOL  # noqa: E402  (2e-6 of the largest sample)

pytestmark = pytest.mark.gpu

# (case, normalize mode, force_peak_amplitude, cfo_value or None)
RUNS = [("t1", 0, 0.0, None), ("t2", 0, 0.0, 0.21), ("t3", 1, 0.6, None), ("t4", 1, 0.0, -0.4), ("t10", 0, 0.0, None),
        ("t8", 0, 0.0, 0.05)]


@pytest.fixture(scope="module")
def env():
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.fail("no HIP device on a GPU test run")
    if not OP.ref_available():
        pytest.fail("oracle/_ref/libsrsref.so missing: the reference checker of this module was not built")
    return OP.PuschOracle()


def norm_factor(mode, peak_amp, nof_prb, L, peak):
    """apply_norm / limit_norm_factor (ue_ul.c:246-299) in the reference's types"""
    f32 = np.float32
    peak = f32(peak)
    if mode == 1:
        return f32((f32(peak_amp) if peak_amp > 0 else f32(1.0)) / peak)
    f = f32(f32(nof_prb // 15) / np.sqrt(f32(L)) / f32(2))
    if float(peak * f) > 0.95:
        f = f32(0.95 / float(peak))
    if float(peak * f) < 0.1:
        f = f32(0.1 / float(peak))
    return f


@pytest.mark.parametrize("run", RUNS, ids=[f"{r[0]}_mode{r[1]}_cfo{r[3]}" for r in RUNS])
def test_samples_match_model(env, run):
    from srsran_4g_amd import ue_ul as UL
    name, mode, amp, cfo = run
    c = TC.BY_NAME[name]
    cell, d, sf, cfg = TC.make(c)
    payload, u = TC.payload_uci(c, cfg)
    ue = UL.UeUl(cell)
    try:
        ucfg = TC.ue_cfg(c, cfg, d, mode=mode, peak=amp, cfo=cfo)
        ret, x = ue.encode(sf, ucfg, payload, u)
        assert ret == 1
        x = x.copy()
        _, _, grid = ue.last()
        N, nre = ue.q.fft.cfg.symbol_sz, 12 * c["nof_prb"]
        assert x.size == 15 * N == ofdm_np.sf_len(N, c["cp"])
        y = ofdm_np.ofdm_tx_opts(grid, N, nre, normalize=True, ext=c["cp"], freq_shift=0.5)
        if cfo is not None:
            f = float(np.float32(np.float32(cfo) / np.float32(N)))
            y = ofdm_np.ref_apply_cfo(np.asarray(y, np.complex64), f).astype(np.complex128)
        peak = max(np.abs(y.real).max(), np.abs(y.imag).max())
        fac = norm_factor(mode, amp, c["nof_prb"], c["L"], peak)
        want = y * float(fac)
        err = float(np.abs(x - want).max() / np.abs(want).max())
        got_peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
        print(name, "samples: distance %.3e, bound %.3e; factor %.6g, peak %.6g" % (err, TOL, fac, got_peak))
        assert err <= TOL
        if name == "t1":  # 6 // 15 = 0: the factor starts from 0 and the 0.1 floor sets it
            assert got_peak == pytest.approx(0.1, rel=1e-5)
        if mode == 1:
            assert got_peak == pytest.approx(amp if amp > 0 else 1.0, rel=1e-5)
        if mode == 0:
            assert 0.1 * (1 - 1e-5) <= got_peak <= 0.95 * (1 + 1e-5)
    finally:
        ue.free()


def test_no_grant_zeroes_the_buffer(env):
    from srsran_4g_amd import ue_ul as UL
    c = TC.BY_NAME["t2"]
    cell, d, sf, cfg = TC.make(c)
    payload, u = TC.payload_uci(c, cfg)
    ue = UL.UeUl(cell)
    try:
        ucfg = TC.ue_cfg(c, cfg, d)
        assert ue.encode(sf, ucfg, payload, u)[0] == 1 and np.abs(ue.out).max() > 0
        ucfg.grant_available = False
        ret, x = ue.encode(sf, ucfg, payload, UL.srsran_uci_value_t())
        assert ret == 0 and not np.any(x)
    finally:
        ue.free()
    fresh = UL.UeUl(cell)
    try:
        with pytest.raises(RuntimeError):  # before the first encode there is nothing to read
            fresh.last()
    finally:
        fresh.free()
