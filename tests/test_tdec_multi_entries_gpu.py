"""One srsran_tdec_gpu_run_multi call that occupies every launch entry of the all-188 step: the two large 16-step
parts cut by residency (K = 4864, 6144 | 2112, 4800), the mid part (1568, 2048), the 8-step part (816, 1536), the
8-sub-block class (408, 800) and the generic class (40, 400).  Five blocks a size, three half-iterations; the 16- and
8-sub-block classes are forced onto the single-lane kernels they take at the step's 1024 blocks a size
(single_threshold(0)), the window cuts and the generic class's quad kernel are the defaults.  The call is issued
twice back to back on one stream with different inputs and no synchronise between: the second call's fork, gate and
staging uploads meet the first call's launches still in flight.  Outputs equal the oracle's."""
import numpy as np
import pytest

from oracle import Oracle, make_llrs

pytestmark = pytest.mark.gpu

SIZES = (40, 400, 408, 800, 816, 1536, 1568, 2048, 2112, 4800, 4864, 6144)
NCB, NIT = 5, 3


def _inputs(ora, seed):
    cases = []
    for K in SIZES:
        rng = np.random.default_rng(seed + K)
        _, llr = make_llrs(K, 0.8, rng, NCB, ora)
        sb = np.stack([ora.natural_to_sb(K, x) for x in llr])
        cases.append((sb, ora.run_batch(K, sb, True, NIT)))
    return cases


def test_every_entry_twice_back_to_back():
    import torch
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.skip("no HIP device")
    ora = Oracle()
    calls = [_inputs(ora, 8100), _inputs(ora, 8200)]
    outs = []
    with tdec.single_threshold(0):
        assert tdec.load_library().srsran_tdec_gpu_get_w8_fused_max_k() == 1536  # the cuts the sizes are chosen by
        stream = torch.cuda.current_stream().cuda_stream
        keep = []
        for cases in calls:
            ins = [torch.from_numpy(sb).cuda() for sb, _ in cases]
            out = [torch.zeros((NCB, K // 8), dtype=torch.uint8, device="cuda") for K in SIZES]
            keep.append(ins)
            outs.append(out)
        for ins, out in zip(keep, outs):
            tdec.gpu_run_multi(list(SIZES), [t.data_ptr() for t in ins], [t.shape[1] for t in ins], True,
                               [t.data_ptr() for t in out], [NCB] * len(SIZES), NIT, stream)
        torch.cuda.synchronize()
    bad = [(n, K) for n, (cases, out) in enumerate(zip(calls, outs))
           for K, o, (_, want) in zip(SIZES, out, cases) if not np.array_equal(o.cpu().numpy(), want)]
    assert not bad, bad
