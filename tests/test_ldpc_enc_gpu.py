"""GPU NR LDPC encoder parity through the C-ABI (srsran_ldpc_encoder_*) against the reference's own encoder
compiled into oracle/_ref (RefLdpc.encode = srsran_ldpc_encoder_encode of ldpc_encoder.c / ldpc_enc_c.c).
Everything is bits: every output byte must be equal."""
import ctypes

import numpy as np
import pytest
import torch

import ldpc as OL
from ldpc import LIFT_SIZES, RefLdpc, lift
from srsran_4g_amd import ldpc as G
from srsran_4g_amd import tdec

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ref():
    if not tdec.gpu_available():
        pytest.skip("no HIP device")
    if not OL.ref_available():  # on a HIP box the parity checker must be there: fail, never skip
        pytest.fail("oracle/_ref/libsrsref.so missing: run build()")
    return RefLdpc()


def _messages(rng, K, ls):
    """random message without filler bits; its last 8 bits fillers; its last Z + 3 bits fillers"""
    m = rng.integers(0, 2, (3, K)).astype(np.uint8)
    m[1, K - 8:] = 254
    m[2, K - (ls + 3):] = 254
    return m


@pytest.mark.parametrize("bg", [0, 1])
def test_every_lifting_size_matches_reference(ref, bg):
    rng = np.random.default_rng(40 + bg)
    for ls in LIFT_SIZES:
        K, N, n = lift(bg, ls)
        msgs = _messages(rng, K, ls)
        want = np.stack([ref.encode(bg, ls, m) for m in msgs])
        enc = G.LdpcEncoder(bg, ls, (G.ENC_C, G.ENC_AVX2, G.ENC_AVX512)[ls % 3])
        assert (enc.q.bgK * ls, enc.q.liftN, enc.q.bgM) == (K, N, OL.BG_SHAPE[bg][0])
        d_msg = torch.from_numpy(msgs).cuda()
        d_cw = torch.full((3, n + 5), SENTINEL, dtype=torch.uint8, device="cuda")
        assert enc.encode_batch(d_msg.data_ptr(), K, 3, d_cw.data_ptr(), n + 5) == 0
        torch.cuda.synchronize()
        got = d_cw.cpu().numpy()
        assert np.array_equal(got[:, :n], want), (bg, ls)
        assert np.all(got[:, n:] == SENTINEL), (bg, ls)
        for m, w in zip(msgs, got[:, :n]):
            r, one = enc.encode(m)
            assert r == 0 and np.array_equal(one, w), (bg, ls)
        enc.free()


def _rounded(bg, ls, length):
    """ldpc_encoder.c:63-78"""
    K, N, n = lift(bg, ls)
    length = max(min(length, n), K + 2 * ls)
    return -(-length // ls) * ls


# the four high-rate solutions (BG1 set index 6 / other, BG2 set index 3, 7 / other) and the largest size
@pytest.mark.parametrize("bg,ls", [(0, 208), (0, 384), (1, 10), (1, 7), (1, 15)])
def test_encode_rm_prefix_and_untouched_tail(ref, bg, ls):
    rng = np.random.default_rng(ls)
    K, N, n = lift(bg, ls)
    msg = _messages(rng, K, ls)[1]
    full = ref.encode(bg, ls, msg)
    enc = G.LdpcEncoder(bg, ls)
    for length in (0, K + 2 * ls, K + 2 * ls + 1, n - 1, n, N):
        L = _rounded(bg, ls, length)
        r, out = enc.encode_rm(msg, length, fill=SENTINEL)
        assert r == 0 and np.array_equal(out[:L], full[:L]), (bg, ls, length)
        assert np.all(out[L:] == SENTINEL), (bg, ls, length)
    enc.free()


def test_refusals():
    if not tdec.gpu_available():
        pytest.skip("no HIP device")
    L = G._lib()
    q = G.srsran_ldpc_encoder_t()
    assert L.srsran_ldpc_encoder_init(ctypes.byref(q), G.ENC_C, 0, 17) == -1  # no lifting size 17
    assert not q.ptr
    enc = G.LdpcEncoder(0, 16)
    msg = np.zeros(enc.liftK, np.uint8)
    assert enc.encode(msg, input_length=enc.liftK + 22)[0] == -1  # input_length / bgK != ls
    assert enc.encode(msg)[0] == 0
    enc.free()
