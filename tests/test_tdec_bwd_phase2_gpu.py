"""Phase 2 of the backward wave in the fused 16-step launch (tdec16s_multi_kernel): the backward recursion of a
window runs first and keeps its stored states, then one forward walk from the window's checkpoint builds one
candidate set a position for both the LLR and the forward step.  Every case is one srsran_tdec_gpu_run_multi call
forced onto the single-lane kernels on 16-step windows (as test_tdec_fused16_gpu.py), outputs compared exactly
with the oracle.

Sizes by crossover h and window shape: K = 816 (L = 51, h = 2: windows 0 and 1, window 0 without its first
normalisation), 1120 (L = 70: five windows of which four are full, h = 3), 1536 (L = 96: full windows only, h = 3),
2048 (L = 128, h = 4), 6144 (L = 384, h = 12).  Batches of 1 and 5 blocks (5: a partly filled workgroup); 1, 2, 3
and 8 half-iterations (the DEC1 and DEC2 bit variants, a checkpoint slot reused across half-iterations).  Inputs:
AWGN rows, and four rows of uniformly random int16 over the full range, with which every add and every
normalisation of both phase-2 loops saturates somewhere.  The oracle's outputs are computed once per case."""
import numpy as np
import pytest

from oracle import Oracle, make_llrs

pytestmark = pytest.mark.gpu

SIZES = (816, 1120, 1536, 2048, 6144)
_cache = {}


@pytest.fixture(scope="module")
def ora():
    return Oracle()


@pytest.fixture(scope="module")
def fused():
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.skip("no HIP device")
    with tdec.single_threshold(0), tdec.w8_max_k(0), tdec.w8_fused_max_k(0):
        yield tdec


def _awgn(ora, K, ncb, nit):
    key = ("awgn", K, ncb, nit)
    if key not in _cache:
        rng = np.random.default_rng(7100 + K + 17 * ncb + nit)
        _, llr = make_llrs(K, 0.8, rng, ncb, ora)
        sb = np.stack([ora.natural_to_sb(K, x) for x in llr])
        want = ora.run_batch(K, sb, True, nit)
        want.setflags(write=False)
        _cache[key] = (sb, want)
    return _cache[key]


def _uniform(ora, tdec, K, nit):
    key = ("uniform", K, nit)
    if key not in _cache:
        rng = np.random.default_rng(7300 + K + nit)
        sb = rng.integers(-32768, 32768, (4, tdec.input_len(K, True)), dtype=np.int64).astype(np.int16)
        want = ora.run_batch(K, sb, True, nit)
        want.setflags(write=False)
        _cache[key] = (sb, want)
    return _cache[key]


def _run(tdec, cases, nit):
    import torch
    ins = [torch.from_numpy(sb).cuda() for sb, _ in cases]
    outs = [torch.zeros((t.shape[0], K // 8), dtype=torch.uint8, device="cuda") for K, t in zip(SIZES, ins)]
    tdec.gpu_run_multi(list(SIZES), [t.data_ptr() for t in ins], [t.shape[1] for t in ins], True,
                       [t.data_ptr() for t in outs], [t.shape[0] for t in ins], nit, None)
    assert tdec.last_kernel() == "tdec16s_multi_kernel"
    torch.cuda.synchronize()
    return [K for K, o, (_, want) in zip(SIZES, outs, cases) if not np.array_equal(o.cpu().numpy(), want)]


@pytest.mark.parametrize("nit", [1, 2, 3, 8])
@pytest.mark.parametrize("ncb", [1, 5])
def test_awgn_rows(ora, fused, ncb, nit):
    bad = _run(fused, [_awgn(ora, K, ncb, nit) for K in SIZES], nit)
    assert not bad, bad


@pytest.mark.parametrize("nit", [1, 2, 3, 8])
def test_uniform_full_range_rows(ora, fused, nit):
    bad = _run(fused, [_uniform(ora, fused, K, nit) for K in SIZES], nit)
    assert not bad, bad
