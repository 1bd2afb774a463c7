"""One-layer spatial multiplexing in the GPU predecoder (eq_kernel.hip scheme 5: 2 ports x 2 rx antennas, codebooks
0..3), the receive side of the TM4 one-layer transmission: srsran_predecoding_multiplex_2x1_mrc_csi
(precoding.c:1727-1812) with float division where its SIMD loop uses rcp.

Checked against (a) the formula in float64, x = norm sum_r conj(h_r) y_r / sum_r |h_r|^2 and csi = sum_r |h_r|^2 /
norm / sqrt 2 with h_r = h[0][r] + {1, -1, j, -j} h[1][r] and norm = sqrt 2 / scaling, within 1e-5 relative (float32
rounding of ~20 operations), and (b) the reference's own srsran_predecoding_type compiled into oracle/_ref, whose
SIMD loop goes through rcp_ps once for x and twice for csi: rcp_ps is specified to 1.5 x 2^-12 relative, so x is held
to 4e-4 and csi to 8e-4 relative.  Lengths with a scalar tail (the reference divides exactly there) included."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = (1, -1, 1j, -1j)
SPATIALMUX = 2


@pytest.fixture(scope="module")
def env():
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.fail("no HIP device on a GPU test run")
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    if not O.ref_available():
        pytest.fail("oracle/_ref/libsrsref.so missing: the reference checker of this module was not built")
    from srsran_4g_amd import phch
    return phch, O.Reference()


@pytest.mark.parametrize("cb", [0, 1, 2, 3])
def test_one_layer_sm_predecoder(env, cb):
    P, ref = env
    rng = np.random.default_rng(60 + cb)
    for n, scaling in ((1203, 1.0), (792, float(np.float32(np.sqrt(2.0)))), (5, 0.6)):
        h = ((rng.standard_normal((2, 2, n)) + 1j * rng.standard_normal((2, 2, n))) / np.sqrt(2)).astype(np.complex64)
        y = ((rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n)))).astype(np.complex64)
        xg, cg = P.predecode(SPATIALMUX, y, h, 1, cb, scaling, 0.05)
        assert xg.shape == (1, n) and cg.shape == (1, n)
        hx = h[0].astype(np.complex128) + Q[cb] * h[1].astype(np.complex128)  # [rx, n]
        hh = np.sum(np.abs(hx) ** 2, axis=0)
        norm = np.sqrt(2.0) / scaling
        xw = np.sum(np.conj(hx) * y.astype(np.complex128), axis=0) * norm / hh
        cw = hh / norm / np.sqrt(2.0)
        assert np.max(np.abs(xg[0] - xw) / np.abs(xw)) < 1e-5
        assert np.max(np.abs(cg[0] - cw) / cw) < 1e-5
        xr, cr = ref.predecode(SPATIALMUX, y, h, 1, cb, scaling, 0.05)
        assert np.max(np.abs(xg[0] - xr[0]) / np.abs(xr[0])) < 4e-4
        assert np.max(np.abs(cg[0] - cr[0]) / cr[0]) < 8e-4


def test_one_layer_sm_refusals(env):
    """codebook 4 and a single rx antenna stay refused (the reference reads a second antenna's buffers regardless)"""
    P, ref = env
    h = np.ones((2, 2, 8), np.complex64)
    y = np.ones((2, 8), np.complex64)
    with pytest.raises(RuntimeError):
        P.predecode(SPATIALMUX, y, h, 1, 4, 1.0, 0.0)
    with pytest.raises(RuntimeError):
        P.predecode(SPATIALMUX, y[:1], h[:, :1], 1, 0, 1.0, 0.0)
