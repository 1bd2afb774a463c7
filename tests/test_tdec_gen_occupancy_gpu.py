"""The generic class (K <= 400) on the quad decoder's NSB = 1 kernels (csrc/tdec_kernel.hip): one int16 array S
in LDS, 16-step windows whose inputs come from the natural-layout input a window ahead, decisions through a
bitmap.  Bit-exact against the reference decoder where it is built (the oracle, pinned to it, elsewhere) at the
sizes where this kernel can go wrong:

* K = 40 (two and a half windows), 48, 56 and 104 (a top window of eight positions and the tail), 136 (odd
  window count), 200, 392 and 400 (the LDS maximum);
* 1, 15, 16, 17 and 33 blocks a launch (a partial wave, a partial last workgroup);
* 1, 2, 3 and 8 half-iterations (odd counts end on DEC1);
* the fused multi-size launch, a DL-SCH batch (CRC early stop) and srsran_tdec_iteration one half-iteration
  a launch (S saved and restored in between).
"""
import numpy as np
import pytest

from oracle import Oracle, Reference, make_llrs, ref_available

pytestmark = pytest.mark.gpu

KS = [40, 48, 56, 104, 136, 200, 392, 400]
NCB = [1, 15, 16, 17, 33]
NIT = [1, 2, 3, 8]


@pytest.fixture(scope="module")
def ora():
    return Oracle()


@pytest.fixture(scope="module")
def ref(ora):
    return Reference() if ref_available() else ora


def inputs(ora, K, rng, n):
    """n blocks: AWGN code blocks, then full-range noise (the int16 wrap matters), then extremes"""
    _, llr = make_llrs(K, 0.5, rng, n, ora)
    llr[n // 2:] = rng.integers(-32768, 32768, size=(n - n // 2, 3 * K + 12), dtype=np.int16)
    if n >= 4:
        llr[-1] = 32767
        llr[-2] = -32768
    return llr


def want_batch(ref, K, llr, nit):
    return np.stack([ref.tdec_run(K, x, False, nit) for x in llr])


@pytest.mark.parametrize("K", KS)
def test_sizes_batches_and_half_iterations(ora, ref, K):
    from srsran_4g_amd import tdec
    rng = np.random.default_rng(4000 + K)
    llr = inputs(ora, K, rng, max(NCB))
    dec = tdec.TurboDecoder()
    bad = []
    for nit in NIT:
        want = want_batch(ref, K, llr, nit)
        for n in NCB:
            got = dec.run_all_batch(llr[:n], nit, K)
            assert tdec.last_kernel() == "tdec_kernel<1>"
            if not np.array_equal(got, want[:n]):
                bad.append((nit, n))
    dec.free()
    assert not bad, bad


def test_multi_size_launch(ora, ref):
    """five generic sizes with different block counts, one 8- and one 16-sub-block size, in one gpu_run_multi"""
    torch = pytest.importorskip("torch")
    from srsran_4g_amd import tdec
    rng = np.random.default_rng(4500)
    Ks = [40, 400, 56, 136, 392, 416, 832]
    ncbs = [17, 33, 1, 16, 15, 3, 2]
    ins, outs, want = [], [], []
    for K, n in zip(Ks, ncbs):
        llr = inputs(ora, K, rng, n)
        ins.append(torch.from_numpy(llr).cuda())
        outs.append(torch.zeros((n, K // 8), dtype=torch.uint8, device="cuda"))
        want.append(want_batch(ref, K, llr, 8))
    stream = torch.cuda.current_stream().cuda_stream
    tdec.gpu_run_multi(Ks, [t.data_ptr() for t in ins], [t.shape[1] for t in ins], False,
                       [t.data_ptr() for t in outs], ncbs, 8, stream)
    assert tdec.last_kernel() == "tdec_multi_kernel<1>"  # the generic class is issued last
    torch.cuda.current_stream().synchronize()
    for K, o, w in zip(Ks, outs, want):
        assert np.array_equal(o.cpu().numpy(), w), K


def test_dlsch_batch_early_stop(ora, ref):
    """a DL-SCH batch of single-block TBs with K <= 400 (CRC24A over the TB): some decode at once, some after a
    few half-iterations, some never -- payload, CRC flag and the half-iterations run against dlsch_decode"""
    torch = pytest.importorskip("torch")
    from srsran_4g_amd import sch, tdec
    rng = np.random.default_rng(4600)
    cases = []
    for i in range(20):  # tbs 376 -> K = 400; two workgroups, the second partly filled
        cases.append((376, 2, 1200, (0.3, 0.95, 1.25, 3.0)[i % 4]))
    cases += [(16, 2, 120, 0.9), (120, 2, 360, 1.1), (208, 6, 540, 0.5), (368, 4, 1000, 1.0)]
    q = sch.Sch()
    q.set_max_noi(8)
    keep, entries, want = [], [], []
    for tbs, Qm, G, sigma in cases:
        rc, s = sch.cbsegm(tbs)
        assert s.C == 1 and s.K1 <= 400, (tbs, s.K1)
        tb = rng.integers(0, 256, tbs // 8, dtype=np.uint8)
        e = ora.dlsch_encode(tbs, Qm, 0, G, tb, 0).astype(np.float32) * 2 - 1
        llr = np.trunc(100 * (e + rng.standard_normal(e.shape).astype(np.float32) * sigma)).astype(np.int16)
        d_e = torch.from_numpy(llr).cuda()
        d_data = torch.zeros(tbs // 8 + 64, dtype=torch.uint8, device="cuda")
        sb = sch.SoftbufferRx(nof_prb=100)
        keep.append((d_e, d_data, sb))
        entries.append((tbs, Qm, 0, len(llr), d_e.data_ptr(), d_data.data_ptr(), sb))
        want.append(ref.dlsch_decode(tbs, Qm, 0, llr, 8))
    d_res = torch.full((len(entries),), 77, dtype=torch.int32, device="cuda")
    d_avg = torch.zeros(len(entries), dtype=torch.float32, device="cuda")
    assert q.decode_batch(entries, d_res.data_ptr(), d_avg.data_ptr()) == 0
    torch.cuda.synchronize()
    assert tdec.last_kernel() == "tdec_kernel<1>"
    res, avg = d_res.cpu().numpy(), d_avg.cpu().numpy()
    iters = set()
    for i, ((tbs, Qm, G, sigma), (oret, odata, onoi, oavg, state)) in enumerate(zip(cases, want)):
        assert res[i] == oret, (i, tbs, sigma)
        assert avg[i] == oavg, (i, tbs, sigma)
        assert np.array_equal(keep[i][1].cpu().numpy()[: len(odata)], odata), (i, tbs, sigma)
        keep[i][2].sync()  # the batch leaves the CRC flags on the device
        assert keep[i][2].cb_crc(1) ==[bool(state[1][0])], (i, tbs, sigma)
        iters.add((oret, onoi[0]))
    # the batch does exercise the early stop: passes at different half-iterations and a failure
    assert len({n for r, n in iters if r == 0}) >= 2 and any(r != 0 for r, n in iters), iters
    for _, _, sb in keep:
        sb.free()
    q.free()


@pytest.mark.parametrize("K", [40, 400])
def test_iteration_api_per_half_iteration(ora, ref, K):
    """srsran_tdec_iteration: one half-iteration a launch, the decision after each"""
    from srsran_4g_amd import tdec
    rng = np.random.default_rng(4700 + K)
    llr = inputs(ora, K, rng, 2)
    dec = tdec.TurboDecoder()
    for x in llr:
        _, trace = ref.tdec_run(K, x, False, 10, trace=True)
        want = np.packbits((np.asarray(trace) > 0).astype(np.uint8), axis=-1)
        assert dec.new_cb(K) == 0
        for n in range(10):
            got = dec.iteration(x)
            assert tdec.last_kernel() == "tdec_kernel<1>"
            assert np.array_equal(got, want[n]), f"K={K} half-iteration {n}"
        assert dec.get_nof_iterations() == 10
    dec.free()
