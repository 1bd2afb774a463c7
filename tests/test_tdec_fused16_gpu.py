"""The fused 16-step launch of the 16-sub-block class (tdec16s_multi_kernel): window checkpoints in the device
scratch, two waves a SIMD, launches cut by residency.  Every case is one srsran_tdec_gpu_run_multi call with
all launches forced onto the single-lane kernels on 16-step windows, outputs compared exactly with the oracle.

Sizes: K = 816 (L = 51: three full windows and a partial one, crossover h = 2), 1024 (full windows only), 1056
(odd window count), 3136 (13 windows), 4416 and 4800 (the largest size of which four workgroups fit a CU), 4864
(the smallest of which three fit) and 6144 (the largest scratch region): with the default mid cut at 2048 that is
three fused launches of at least two sizes each.  Batches of 1, 5 and 9 blocks (a partly filled last workgroup);
1, 2, 3 and 8 half-iterations (from three on a checkpoint slot holds the previous half-iteration of the same
direction until phase 1 overwrites it); the four extreme rows of test_tdec_loops_gpu.test_extreme_rows; two calls
in a row on one stream of which the second needs more scratch (this test comes first: in a process of its own the
scratch grows between its calls).  The oracle's outputs are computed once per (K, blocks, half-iterations)."""
import numpy as np
import pytest

from oracle import Oracle, make_llrs

pytestmark = pytest.mark.gpu

SIZES = (816, 1024, 1056, 3136, 4416, 4800, 4864, 6144)
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


def _case(ora, K, ncb, nit):
    key = (K, ncb, nit)
    if key not in _cache:
        rng = np.random.default_rng(9000 + K + 17 * ncb + nit)
        _, llr = make_llrs(K, 0.8, rng, ncb, ora)
        sb = np.stack([ora.natural_to_sb(K, x) for x in llr])
        want = ora.run_batch(K, sb, True, nit)
        want.setflags(write=False)
        _cache[key] = (sb, want)
    return _cache[key]


def _launch(tdec, Ks, sbs, nit):
    """one fused call; returns the output tensors (not yet synchronised)"""
    import torch
    ins = [torch.from_numpy(sb).cuda() for sb in sbs]
    outs = [torch.zeros((sb.shape[0], K // 8), dtype=torch.uint8, device="cuda") for K, sb in zip(Ks, sbs)]
    tdec.gpu_run_multi(list(Ks), [t.data_ptr() for t in ins], [t.shape[1] for t in ins], True,
                       [t.data_ptr() for t in outs], [t.shape[0] for t in ins], nit, None)
    assert tdec.last_kernel() == "tdec16s_multi_kernel"
    return ins, outs


def test_second_call_needs_more_scratch(ora, fused):
    import torch
    small = [_case(ora, K, 1, 3) for K in (816, 1024)]
    large = [_case(ora, K, 9, 3) for K in (4864, 6144)]
    keep1, outs1 = _launch(fused, (816, 1024), [c[0] for c in small], 3)
    keep2, outs2 = _launch(fused, (4864, 6144), [c[0] for c in large], 3)
    torch.cuda.synchronize()
    for K, o, c in zip((816, 1024, 4864, 6144), outs1 + outs2, small + large):
        assert np.array_equal(o.cpu().numpy(), c[1]), K


@pytest.mark.parametrize("nit", [1, 2, 3, 8])
@pytest.mark.parametrize("ncb", [1, 5, 9])
def test_sizes(ora, fused, ncb, nit):
    import torch
    cases = [_case(ora, K, ncb, nit) for K in SIZES]
    _, outs = _launch(fused, SIZES, [c[0] for c in cases], nit)
    torch.cuda.synchronize()
    bad = [K for K, o, c in zip(SIZES, outs, cases) if not np.array_equal(o.cpu().numpy(), c[1])]
    assert not bad, bad


def test_extreme_rows(ora, fused):
    import torch
    Ks = (816, 1024)
    cases = []
    for K in Ks:
        n = fused.input_len(K, True)
        llr = np.stack([np.zeros(n, np.int16), np.full(n, 32767, np.int16), np.full(n, -32768, np.int16),
                        np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)])
        cases.append((llr, ora.run_batch(K, llr, True, 8)))
    _, outs = _launch(fused, Ks, [c[0] for c in cases], 8)
    torch.cuda.synchronize()
    for K, o, c in zip(Ks, outs, cases):
        assert np.array_equal(o.cpu().numpy(), c[1]), K
