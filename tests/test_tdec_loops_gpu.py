"""The window loops of the single-lane decoders (tdecs_kernel.hip) at the edges of each class, bit-exact against
the oracle decoder: every launch forced onto the single-lane kernels (single_threshold 0), once on 16-step
windows and once on 8-step windows (w8_max_k 6144).

Sizes: K = 816 and 408 (L = 51: three full windows and a 3-position last one on 16 steps), 1024 and 512 (full
windows only), 1056, 800, 3136 and 6144; batches of 5 and 9 blocks (a partly filled last workgroup in both
classes); 1, 2, 3 and 8 half-iterations (decision bits out of DEC1 and out of DEC2); the extreme rows of
test_tdec_gpu.test_degenerate_inputs; one fused multi-size launch; one DL-SCH transport block per class with
CRC early stop.  The oracle's outputs are computed once per case and shared by both window modes."""
import numpy as np
import pytest

from oracle import Oracle, make_llrs

pytestmark = pytest.mark.gpu

SIZES = (816, 408, 1024, 512, 1056, 800, 3136, 6144)
_cache = {}


@pytest.fixture(scope="module")
def ora():
    return Oracle()


@pytest.fixture(scope="module", params=["w16", "w8"])
def mode(request):
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.skip("no HIP device")
    if request.param == "w16":
        with tdec.single_threshold(0), tdec.w8_max_k(0), tdec.w8_fused_max_k(0):
            yield "s_"
    else:
        with tdec.single_threshold(0), tdec.w8_max_k(6144):
            yield "sw8_"


def _case(ora, K, ncb, nit):
    """inputs (SB layout) and the oracle's decisions of one plain batch, computed once"""
    key = (K, ncb, nit)
    if key not in _cache:
        rng = np.random.default_rng(7000 + K + 17 * ncb + nit)
        _, llr = make_llrs(K, 0.8, rng, ncb, ora)
        sb = np.stack([ora.natural_to_sb(K, x) for x in llr])
        want = ora.run_batch(K, sb, True, nit)
        want.setflags(write=False)
        _cache[key] = (sb, want)
    return _cache[key]


@pytest.mark.parametrize("nit", [1, 2, 3, 8])
@pytest.mark.parametrize("ncb", [5, 9])
def test_edge_sizes(ora, mode, ncb, nit):
    from srsran_4g_amd import tdec
    dec = tdec.TurboDecoder()
    bad = []
    for K in SIZES:
        sb, want = _case(ora, K, ncb, nit)
        if not np.array_equal(dec.run_all_batch(sb, nit, K), want):
            bad.append(K)
        assert tdec.last_kernel() == f"tdec{tdec.nof_subblocks(K)}{mode}kernel<false>"
    dec.free()
    assert not bad, bad


@pytest.mark.parametrize("K", [816, 408])
def test_extreme_rows(ora, mode, K):
    from srsran_4g_amd import tdec
    key = ("ext", K)
    if key not in _cache:
        n = tdec.input_len(K, True)
        llr = np.stack([np.zeros(n, np.int16), np.full(n, 32767, np.int16), np.full(n, -32768, np.int16),
                        np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)])
        _cache[key] = (llr, ora.run_batch(K, llr, True, 8))
    llr, want = _cache[key]
    dec = tdec.TurboDecoder()
    got = dec.run_all_batch(llr, 8, K)
    assert tdec.last_kernel() == f"tdec{tdec.nof_subblocks(K)}{mode}kernel<false>"
    dec.free()
    assert np.array_equal(got, want)


def test_fused_multi_size(ora, mode):
    import torch
    from srsran_4g_amd import tdec
    Ks = [816, 1056, 6144]
    ins, outs, wants = [], [], []
    for i, K in enumerate(Ks):
        sb, want = _case(ora, K, 5 + 4 * (i % 2), 8)
        ins.append(torch.from_numpy(sb).cuda())
        outs.append(torch.zeros((sb.shape[0], K // 8), dtype=torch.uint8, device="cuda"))
        wants.append(want)
    tdec.gpu_run_multi(Ks, [t.data_ptr() for t in ins], [t.shape[1] for t in ins], True,
                       [t.data_ptr() for t in outs], [t.shape[0] for t in ins], 8, None)
    torch.cuda.synchronize()
    assert tdec.last_kernel() == f"tdec16{mode}multi_kernel"
    for K, o, w in zip(Ks, outs, wants):
        assert np.array_equal(o.cpu().numpy(), w), K


def test_dlsch_early_stop(ora, mode):
    from srsran_4g_amd import sch, tdec
    rng = np.random.default_rng(7100)
    q = sch.Sch()
    for tbs, Qm, G in ((600, 2, 1440), (6120, 4, 9000), (30576, 6, 38000)):
        rc, s = sch.cbsegm(tbs)
        tb = rng.integers(0, 256, tbs // 8, dtype=np.uint8)
        sb = sch.SoftbufferRx(nof_prb=100)
        state = None
        for rv, sigma in ((0, 0.9), (2, 0.9), (3, 0.5)):
            e = ora.dlsch_encode(tbs, Qm, rv, G, tb, 0).astype(np.float32) * 2 - 1
            llr = np.trunc(100 * (e + rng.standard_normal(e.shape).astype(np.float32) * sigma)).astype(np.int16)
            q.set_max_noi(8)
            ret, data, avg = q.decode(sb, tbs, Qm, rv, llr)
            assert tdec.last_kernel().endswith(mode + "kernel<true>"), tdec.last_kernel()
            oret, odata, _, oavg, state = ora.dlsch_decode(tbs, Qm, rv, llr, 8, state)
            assert ret == oret, (tbs, rv)
            assert np.array_equal(data[: len(odata)], odata), (tbs, rv)
            assert avg == pytest.approx(oavg, abs=0), (tbs, rv)
            assert sb.cb_crc(s.C) == [bool(x) for x in state[1][: s.C]], (tbs, rv)
        sb.free()
    q.free()
