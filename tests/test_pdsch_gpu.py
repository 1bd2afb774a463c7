"""GPU srsran_pdsch_decode / srsran_ue_dl_* against the oracle chain (oracle/pdsch_chain.py,
composed from pieces pinned to the reference) on synthetic eNB subframes (synth/).

Bit-exact tier: the GPU PDSCH stage is fed the oracle's own grids and channel estimates, so
predecode (IEEE float, no contraction), demap, descramble, CSI correction and DL-SCH decode must
agree exactly -- decode_tb's return, every payload byte it writes, avg iterations.
Chain tier: GPU OFDM + channel estimation differ from numpy / the oracle by float rounding
(FFT and reductions in another order; FFT parity is unpinned), so the full GPU chain
is checked by decoding (CRC pass, payload == transmitted) and by agreement with the oracle chain.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from oracle import Oracle
import pdsch_chain as PC
from synth import synth as S

pytestmark = pytest.mark.gpu

TBS = 75376  # C3: MCS 28, 100 PRB (grant_probe)


@pytest.fixture(scope="module")
def ora():
    return Oracle()


@pytest.fixture(scope="module")
def U():
    from srsran_4g_amd import ue_dl
    return ue_dl


@pytest.fixture(scope="module", autouse=True)
def standard_rates(U):
    """these cases run at standard rates (N = 2048 at 100 PRB, as srsUE / C3); the reference
    default (3/4 rates) is restored afterwards and tested on its own"""
    U.use_standard_symbol_size(True)
    yield
    U.use_standard_symbol_size(False)


@pytest.fixture(scope="module")
def SCH():
    from srsran_4g_amd import sch
    return sch


def _case(ora, rng, nof_prb=100, cell_id=1, nports=2, tti=1, cfi=1, tbs=(TBS, TBS), Qm=(6, 6), scheme="cdd",
          pmi=0, snr_db=30.0, **kw):
    assert len(set(tbs)) == 1 and len(set(Qm)) == 1  # synth sends one TBS / modulation per subframe
    pls = [rng.integers(0, 256, t // 8, dtype=np.uint8) for t in tbs]
    cb = pmi + 1 if len(tbs) == 2 else pmi
    x, nre = S.pdsch_subframe(nof_prb, cell_id, nports, tti, cfi, 0x1234, tbs[0], Qm[0], 0, pls, scheme=scheme,
                              codebook=cb, snr_db=snr_db, rng=rng, **kw)
    grids, ce, st = PC.fft_estimate(ora, x, nof_prb, cell_id, nports, tti, N=kw.get("N"))
    return pls, x, nre, grids, ce, st


CASES = [
    dict(),                                                 # C3, subframe 1
    dict(tti=5),                                            # PSS / SSS subframe
    dict(tti=10),                                           # subframe 0 (PBCH)
    dict(snr_db=13.0, fail=True),                           # CB CRC failures / early-stop spread
    dict(tti=10, cfi=2, fail=True),                         # code rate > 0.98: undecodable, fails alike
    dict(scheme="sm", pmi=0),                               # TM4 codebook 1
    dict(scheme="sm", pmi=1, cell_id=7),                    # TM4 codebook 2
    dict(nports=1, scheme="port0", tbs=(30576,), Qm=(4,), cell_id=3, channel=[[1], [0.5 + 0.5j]]),
    dict(scheme="diversity", tbs=(TBS,), Qm=(6,), tti=5, cell_id=4),       # TM2 SFBC, layer demap fused
    dict(scheme="diversity", tbs=(TBS,), Qm=(6,), snr_db=12.0, fail=True),  # TM2 with CB failures
    dict(nof_prb=50, cell_id=11, tbs=(36696, 36696), tti=3, cfi=1),
    dict(nof_prb=50, cell_id=11, tbs=(25456, 25456), tti=4, cfi=3),
    dict(nof_prb=6, cell_id=2, tbs=(1800, 1800), Qm=(4, 4), cfi=2, tti=7),
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("opts", [dict(), dict(csi_enable=False), dict(power_scale=True, p_a=-3.0, p_b=2),
                                  dict(zf=True)])
def test_pdsch_decode_bitexact(U, SCH, ora, case, opts):
    kw = dict(CASES[case])
    if opts and case not in (0, 3, 7, 8):
        pytest.skip("options exercised on a subset of grants")
    rng = np.random.default_rng(100 + case)
    fail = kw.pop("fail", False)
    nof_prb = kw.pop("nof_prb", 100)
    cell_id = kw.pop("cell_id", 1)
    nports = kw.pop("nports", 2)
    tti = kw.pop("tti", 1)
    cfi = kw.pop("cfi", 1)
    tbs = kw.pop("tbs", (TBS, TBS))
    Qm = kw.pop("Qm", (6, 6))
    scheme = kw.pop("scheme", "cdd")
    pmi = kw.pop("pmi", 0)
    pls, x, nre, grids, ce, st = _case(ora, rng, nof_prb, cell_id, nports, tti, cfi, tbs, Qm, scheme, pmi, **kw)
    noise = st["noise"]
    ref = PC.pdsch_decode(ora, grids, ce, noise, nof_prb, cell_id, nports, tti, cfi, 0x1234, list(tbs), list(Qm),
                          [0] * len(tbs), scheme=scheme, pmi=pmi, csi_enable=opts.get("csi_enable", True),
                          power_scale=opts.get("power_scale", False), p_a=opts.get("p_a", 0.0),
                          p_b=opts.get("p_b", 0)) if not opts.get("zf") else \
        PC.pdsch_decode(ora, grids, ce, 0.0, nof_prb, cell_id, nports, tti, cfi, 0x1234, list(tbs), list(Qm),
                        [0] * len(tbs), scheme=scheme, pmi=pmi)
    sbs = [SCH.SoftbufferRx(nof_prb=nof_prb) for _ in tbs]
    cfg = U.pdsch_cfg(nof_prb, nre, tbs, Qm, scheme=scheme, pmi=pmi, softbuffers=sbs, **opts)
    pd = U.Pdsch(U.cell(nof_prb, nports, cell_id), grids.shape[0])
    ret, out = pd.decode(cfg, tti, cfi, grids, ce, noise)
    assert ret == 0
    for q, (crc, payload, avg) in enumerate(out):
        r = ref[q]
        assert crc == (r["ret"] == 0), q
        n = tbs[q] // 8 + 6
        assert np.array_equal(payload[:n], r["data"][:n]), q
        assert avg == pytest.approx(r["avg"], abs=1e-6), q
        if not fail:
            assert crc and np.array_equal(payload[: tbs[q] // 8], pls[q])
    pd.free()


def test_pdsch_work_area_regrowth_is_bit_identical(U, SCH, ora):
    """One PDSCH object: the 6-PRB grant (grids and work area under the 64 KB floor), the 100-PRB C3 grant (both
    above it), the 6-PRB grant again -- every result equal to a fresh object's on the same input."""
    rng = np.random.default_rng(55)
    small = dict(nof_prb=6, cell_id=2, tbs=(1800, 1800), Qm=(4, 4), cfi=2, tti=7)
    large = dict(nof_prb=100, cell_id=1, tbs=(TBS, TBS), Qm=(6, 6), cfi=1, tti=1)
    data = {id(k): _case(ora, rng, **k) for k in (small, large)}

    def run(pd, k):
        pls, x, nre, grids, ce, st = data[id(k)]
        sbs = [SCH.SoftbufferRx(nof_prb=k["nof_prb"]) for _ in k["tbs"]]
        cfg = U.pdsch_cfg(k["nof_prb"], nre, k["tbs"], k["Qm"], softbuffers=sbs)
        ret, out = pd.decode(cfg, k["tti"], k["cfi"], grids, ce, st["noise"])
        assert ret == 0
        for q, (crc, payload, avg) in enumerate(out):
            assert crc and np.array_equal(payload[: k["tbs"][q] // 8], pls[q])
        return [np.concatenate([[crc, avg], payload]) for crc, payload, avg in out]

    one = U.Pdsch(U.cell(100, 2, 1), 2)
    for k in (small, large, small):
        c = U.cell(k["nof_prb"], 2, k["cell_id"])
        assert U.lib().srsran_pdsch_set_cell(ctypes.byref(one.q), c) == 0
        fresh = U.Pdsch(c, 2)
        want = run(fresh, k)
        fresh.free()
        got = run(one, k)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), k["nof_prb"]
    one.free()


def test_pdsch_already_acked_is_skipped(U, SCH, ora):
    rng = np.random.default_rng(5)
    pls, x, nre, grids, ce, st = _case(ora, rng)
    sbs = [SCH.SoftbufferRx(nof_prb=100) for _ in range(2)]
    cfg = U.pdsch_cfg(100, nre, (TBS, TBS), (6, 6), softbuffers=sbs)
    pd = U.Pdsch(U.cell(100, 2, 1), 2)
    ret, out = pd.decode(cfg, 1, 1, grids, ce, st["noise"], acked=(True, False))
    assert ret == 0
    assert out[0][0] and not out[0][1][:16].any()  # TB0 untouched
    assert out[1][0] and np.array_equal(out[1][1][: TBS // 8], pls[1])
    pd.free()


def test_pdsch_rejects_wrong_nof_re(U, SCH, ora):
    rng = np.random.default_rng(6)
    pls, x, nre, grids, ce, st = _case(ora, rng)
    sbs = [SCH.SoftbufferRx(nof_prb=100) for _ in range(2)]
    cfg = U.pdsch_cfg(100, nre + 12, (TBS, TBS), (6, 6), softbuffers=sbs)
    pd = U.Pdsch(U.cell(100, 2, 1), 2)
    ret, _ = pd.decode(cfg, 1, 1, grids, ce, st["noise"])
    assert ret != 0
    pd.free()


def test_ue_dl_host_sync_decodes(U, SCH, ora):
    """srsran_ue_dl_decode_fft_estimate_noguru + srsran_ue_dl_decode_pdsch on time samples"""
    rng = np.random.default_rng(7)
    ue = U.UeDl(U.cell(100, 2, 1), 2)
    for tti in (1, 5, 10):
        pls, x, nre, grids, ce, st = _case(ora, rng, tti=tti)
        assert ue.fft_estimate(x, tti, 1) == 0
        g = ue.grids()
        assert np.abs(g - grids).max() < 1e-3 * np.abs(grids).max()
        sbs = [SCH.SoftbufferRx(nof_prb=100) for _ in range(2)]
        cfg = U.pdsch_cfg(100, nre, (TBS, TBS), (6, 6), softbuffers=sbs)
        ret, out = ue.decode_pdsch(cfg, tti, 1)
        assert ret == 0
        for q in range(2):
            assert out[q][0] and np.array_equal(out[q][1][: TBS // 8], pls[q])
    ue.free()


def test_ue_dl_batch_matches_host_sync(U, SCH, ora):
    """srsran_ue_dl_gpu_decode_batch over 10 subframes (all subframe types, 2 grants) == the
    host-synchronous UE DL path subframe by subframe, and decodes what was sent."""
    rng = np.random.default_rng(8)
    ue = U.UeDl(U.cell(100, 2, 1), 2)
    nsf = 10
    samples, cfgs, payloads, entries, sbs = [], [], [], [], []
    d_pl = torch.zeros((nsf, 2, TBS // 8 + 64), dtype=torch.uint8, device="cuda")
    for b in range(nsf):
        tti = 21 + b
        cfi = 2 if b % 3 == 1 else 1  # CFI 2 on subframes 2, 5, 8
        pls, x, nre, _, _, _ = _case(ora, rng, tti=tti, cfi=cfi)
        sb = [SCH.SoftbufferRx(nof_prb=100) for _ in range(2)]
        cfg = U.pdsch_cfg(100, nre, (TBS, TBS), (6, 6), softbuffers=sb)
        samples.append(x)
        cfgs.append(cfg)
        payloads.append(pls)
        sbs.append(sb)
        entries.append((tti, cfi, cfg, [d_pl[b, 0].data_ptr(), d_pl[b, 1].data_ptr()], [1, 1]))
    d_x = torch.from_numpy(np.stack(samples).view(np.float32)).cuda()
    d_res = torch.full((2 * nsf,), 7, dtype=torch.int32, device="cuda")
    d_avg = torch.zeros(2 * nsf, dtype=torch.float32, device="cuda")
    n = ue.gpu_decode_batch(entries, d_x.data_ptr(), d_res.data_ptr(), d_avg.data_ptr(), 0.0, None)
    assert n == 2 * nsf
    torch.cuda.synchronize()
    res = d_res.cpu().numpy()
    avg = d_avg.cpu().numpy()
    pl = d_pl.cpu().numpy()
    ue2 = U.UeDl(U.cell(100, 2, 1), 2)
    for b in range(nsf):
        tti, cfi = entries[b][0], entries[b][1]
        assert ue2.fft_estimate(samples[b], tti, cfi) == 0
        sb = [SCH.SoftbufferRx(nof_prb=100) for _ in range(2)]
        cfg = U.pdsch_cfg(100, cfgs[b].grant.nof_re, (TBS, TBS), (6, 6), softbuffers=sb)
        ret, out = ue2.decode_pdsch(cfg, tti, cfi)
        for q in range(2):
            assert res[2 * b + q] == 0 and out[q][0]
            assert np.array_equal(pl[b, q, : TBS // 8], payloads[b][q])
            assert np.array_equal(pl[b, q, : TBS // 8 + 6], out[q][1][: TBS // 8 + 6])
            assert avg[2 * b + q] == pytest.approx(out[q][2], abs=0.2)
    ue.free()
    ue2.free()


def test_ue_dl_batches_on_several_streams(U, SCH, ora):
    """Batch workers (bench --pdsch-workers): two UE DL objects on two created streams take six batches in turn
    with no host synchronisation between them, then one object's batches switch streams (the stream hand-over of
    its staging ring and scratch, stage_copy.h); every batch decodes what was sent, with the same results as
    a single batch on the default stream.  Also the deferred launches with a mixed iteration limit (in line)."""
    rng = np.random.default_rng(11)
    nsf = 4
    samples, nres, payloads = [], [], []
    for b in range(nsf):
        pls, x, nre, _, _, _ = _case(ora, rng, tti=31 + b)
        samples.append(x)
        nres.append(nre)
        payloads.append(pls)
    d_x = torch.from_numpy(np.stack(samples).view(np.float32)).cuda()

    def make(limits=None):
        ue = U.UeDl(U.cell(100, 2, 1), 2)
        sbs = [[SCH.SoftbufferRx(nof_prb=100) for _ in range(2)] for _ in range(nsf)]
        cfgs = [U.pdsch_cfg(100, nres[b], (TBS, TBS), (6, 6), softbuffers=sbs[b],
                            max_iterations=(limits[b] if limits else 8)) for b in range(nsf)]
        d_pl = torch.zeros((nsf, 2, TBS // 8 + 64), dtype=torch.uint8, device="cuda")
        d_res = torch.full((2 * nsf,), 7, dtype=torch.int32, device="cuda")
        d_avg = torch.zeros(2 * nsf, dtype=torch.float32, device="cuda")
        entries = [(31 + b, 1, cfgs[b], [d_pl[b, 0].data_ptr(), d_pl[b, 1].data_ptr()], [1, 1]) for b in range(nsf)]
        return dict(ue=ue, sbs=sbs, cfgs=cfgs, pl=d_pl, res=d_res, avg=d_avg, entries=entries)

    def run(w, stream):
        w["pl"].zero_()
        w["res"].fill_(7)
        sp = stream.cuda_stream if stream is not None else None
        assert w["ue"].gpu_decode_batch(w["entries"], d_x.data_ptr(), w["res"].data_ptr(), w["avg"].data_ptr(), 0.0,
                                        sp) == 2 * nsf

    def check(w):
        res, pl = w["res"].cpu().numpy(), w["pl"].cpu().numpy()
        for b in range(nsf):
            for q in range(2):
                assert res[2 * b + q] == 0, (b, q)
                assert np.array_equal(pl[b, q, : TBS // 8], payloads[b][q]), (b, q)
        return w["avg"].cpu().numpy().copy()

    ref = make()
    run(ref, None)
    torch.cuda.synchronize()
    want_avg = check(ref)
    ws = [make(), make()]
    st = [torch.cuda.Stream(), torch.cuda.Stream()]
    for i in range(6):  # the two workers in turn, nothing synchronised in between (zeroing is stream-ordered too)
        with torch.cuda.stream(st[i % 2]):
            run(ws[i % 2], st[i % 2])
    torch.cuda.synchronize()
    for w in ws:
        assert np.array_equal(check(w), want_avg)
    for i in range(4):  # one object, its batches alternating between the two streams
        with torch.cuda.stream(st[i % 2]):
            run(ws[0], st[i % 2])
        torch.cuda.synchronize()
        assert np.array_equal(check(ws[0]), want_avg)
    mixed = make(limits=[8, 6, 8, 6])  # two DL-SCH groups: the in-line launch order
    run(mixed, None)
    torch.cuda.synchronize()
    check(mixed)
    for w in [ref, mixed] + ws:
        w["ue"].free()
        for pair in w["sbs"]:
            for sb in pair:
                sb.free()


def test_ue_dl_batch_cfo(U, SCH, ora):
    """a CFO on the samples, removed by the batch's fused rotation"""
    rng = np.random.default_rng(9)
    ue = U.UeDl(U.cell(100, 2, 1), 2)
    f = 150.0 / 30.72e6
    pls, x, nre, _, _, _ = _case(ora, rng, tti=2, cfo=f)
    sb = [SCH.SoftbufferRx(nof_prb=100) for _ in range(2)]
    cfg = U.pdsch_cfg(100, nre, (TBS, TBS), (6, 6), softbuffers=sb)
    d_pl = torch.zeros((2, TBS // 8 + 64), dtype=torch.uint8, device="cuda")
    d_x = torch.from_numpy(x[None].view(np.float32)).cuda()
    d_res = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    d_avg = torch.zeros(2, dtype=torch.float32, device="cuda")
    n = ue.gpu_decode_batch([(2, 1, cfg, [d_pl[0].data_ptr(), d_pl[1].data_ptr()], [1, 1])], d_x.data_ptr(),
                            d_res.data_ptr(), d_avg.data_ptr(), -f, None)
    assert n == 2
    torch.cuda.synchronize()
    assert (d_res.cpu().numpy() == 0).all()
    for q in range(2):
        assert np.array_equal(d_pl[q].cpu().numpy()[: TBS // 8], pls[q])
    ue.free()


def _ref_evm(sym, demod, mod, nof_bits, max_bits):
    """srsran_evm_run_s of the reference (modem/evm.h, compiled into oracle/_ref: ref_pdsch_tx_harness.c)"""
    import ctypes
    L = ctypes.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref",
                                 "libsrsref.so"), mode=os.RTLD_LAZY)
    f = L.ref_evm_run_s
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    f.restype = ctypes.c_float
    sym = np.ascontiguousarray(sym, np.complex64)
    demod = np.ascontiguousarray(demod, np.int16)
    return float(f(mod, sym.ctypes.data, demod.ctypes.data, nof_bits, max_bits))


@pytest.mark.parametrize("case", [0, 3, 5, 7, 8, 12])
def test_pdsch_evm_matches_reference(U, SCH, ora, case):
    """cfg->meas_evm_en (pdsch.c:698-713, srsUE phy.meas_evm): srsran_pdsch_res_t.evm of every TB (host-synchronous
    srsran_pdsch_decode) and srsran_pdsch_gpu_last_evm (batch) against the reference's own srsran_evm_run_s
    (modem/evm.h:175-212, compiled into _ref) on the oracle chain's equalised symbols and demodulated LLRs of the
    same grids: the same hard decisions, remodulated symbols and bit limit (the EVM buffer's max_bits,
    pdsch.c:297, 468-471); the squared errors are summed in another order (GPU block tree vs AVX2 lanes): rtol 5e-5.
    q->avg_evm follows the reference's EMA (pdsch.c:945-951)."""
    kw = dict(CASES[case])
    rng = np.random.default_rng(300 + case)
    kw.pop("fail", False)
    nof_prb = kw.pop("nof_prb", 100)
    cell_id = kw.pop("cell_id", 1)
    nports = kw.pop("nports", 2)
    tti = kw.pop("tti", 1)
    cfi = kw.pop("cfi", 1)
    tbs = kw.pop("tbs", (TBS, TBS))
    Qm = kw.pop("Qm", (6, 6))
    scheme = kw.pop("scheme", "cdd")
    pmi = kw.pop("pmi", 0)
    pls, x, nre, grids, ce, st = _case(ora, rng, nof_prb, cell_id, nports, tti, cfi, tbs, Qm, scheme, pmi, **kw)
    ref = PC.pdsch_decode(ora, grids, ce, st["noise"], nof_prb, cell_id, nports, tti, cfi, 0x1234, list(tbs),
                          list(Qm), [0] * len(tbs), scheme=scheme, pmi=pmi)
    max_bits = max(U.lib().srsran_ra_tbs_from_idx(33, 6), U.lib().srsran_ra_tbs_from_idx(33, nof_prb))
    mods = {2: 1, 4: 2, 6: 3, 8: 4}
    want = [_ref_evm(r["sym"], r["demod"], mods[Qm[q]], nre * Qm[q], max_bits) for q, r in enumerate(ref)]
    assert all(np.isfinite(w) and w > 0 for w in want)
    sbs = [SCH.SoftbufferRx(nof_prb=nof_prb) for _ in tbs]
    cfg = U.pdsch_cfg(nof_prb, nre, tbs, Qm, scheme=scheme, pmi=pmi, softbuffers=sbs, meas_evm=True,
                      nof_ports=nports)
    pd = U.Pdsch(U.cell(nof_prb, nports, cell_id), grids.shape[0])
    avg0 = pd.q.avg_evm
    ret, _ = pd.decode(cfg, tti, cfi, grids, ce, st["noise"])
    assert ret == 0
    for q in range(len(tbs)):
        assert pd.last_evm[q] == pytest.approx(want[q], rel=5e-5), q
    ema = avg0
    for q in range(len(tbs)):
        ema = 0.1 * pd.last_evm[q] + 0.9 * ema
    assert pd.q.avg_evm == pytest.approx(ema, rel=1e-6)
    # without meas_evm_en the result stays NAN
    cfg0 = U.pdsch_cfg(nof_prb, nre, tbs, Qm, scheme=scheme, pmi=pmi, softbuffers=sbs, nof_ports=nports)
    pd.decode(cfg0, tti, cfi, grids, ce, st["noise"])
    assert all(np.isnan(e) for e in pd.last_evm)
    pd.free()
    for sb in sbs:
        sb.free()


LLR_STATS = {}


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            return next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), "?")
    except OSError:
        return "?"


@pytest.mark.parametrize("pred", ["restated", "reference"])
@pytest.mark.parametrize("N,snr,cfo", [(2048, 30.0, 0.0), (1536, 30.0, 0.0), (2048, 17.0, 0.0), (2048, 20.0, 3e-5)])
def test_chain_llrs_match_oracle_chain(U, SCH, ora, N, snr, cfo, pred):
    """Soft-output agreement of the whole chain from time samples (north_star: LLRs within 1e-4): every
    TB's descrambled, CSI-corrected int16 LLRs from srsran_ue_dl_gpu_decode_batch (OFDM + CFO, CRS estimate,
    MMSE, demap, descramble, CSI -- read back by srsran_pdsch_gpu_last_llr) against the oracle chain on the same
    samples: numpy FFT, the reference's srsran_vec_apply_cfo, the chest restatement, then the MMSE predecoder --

      pred = "restated":  the oracle's exact-division restatement of precoding.c (oracle_predecode), which the
                          GPU predecoder equals bit for bit on the same inputs (test_eq_gpu.py).  The GPU FFT and
                          estimator reductions round in another order (FFT parity unpinned), so a few LLRs sit
                          one LSB apart: >= 99.9 % equal and |delta| <= 1 LSB per TB.
      pred = "reference": the reference's own precoding.c compiled into oracle/_ref (Reference.predecode), run
                          on this host's CPU.  Its AVX2 MMSE bodies divide by _mm256_rcp_ps (precoding.c:1123-1194,
                          simd.h:321-338: a 12-bit reciprocal estimate, whose exact bits differ between CPU
                          vendors), so ~4 % of the LLRs land one LSB away from exact division: >= 95 % equal and
                          |delta| <= 2 LSB per TB (1 from rcp_ps, 1 from the FFT order), decode results equal.

    then the demapper / scrambler / CSI correction (demod_soft.c:569-644, pdsch.c:662-762, pinned to _ref).  The
    figures go to DESIGN.md section 2 (written to $SRSRAN_AMD_LLR_STATS)."""
    pre = None
    if pred == "reference":
        from oracle import Reference, ref_available
        if not ref_available():  # on a HIP box the checker must be there: fail, never skip
            pytest.fail("oracle/_ref/libsrsref.so missing: the reference predecoder (the checker) was not built")
        pre = Reference()
    eq_min, d_max = (0.999, 1) if pred == "restated" else (0.95, 2)
    U.use_standard_symbol_size(N == 2048)
    try:
        rng = np.random.default_rng(int(N + 10 * snr))
        ue = U.UeDl(U.cell(100, 2, 1), 2)
        ttis = (1, 5, 10, 13)
        entries, samples, wants, keep = [], [], [], []
        d_pl = torch.zeros((len(ttis), 2, TBS // 8 + 64), dtype=torch.uint8, device="cuda")
        for b, tti in enumerate(ttis):
            pls, x, nre, _, _, _ = _case(ora, rng, tti=tti, snr_db=snr, N=N, cfo=cfo)
            grids, ce, st = PC.fft_estimate(ora, x, 100, 1, 2, tti, cfo=-cfo, N=N)
            wants.append(PC.pdsch_decode(ora, grids, ce, st["noise"], 100, 1, 2, tti, 1, 0x1234, [TBS, TBS], [6, 6],
                                         [0, 0], pre=pre))
            sb = [SCH.SoftbufferRx(nof_prb=100) for _ in range(2)]
            cfg = U.pdsch_cfg(100, nre, (TBS, TBS), (6, 6), softbuffers=sb)
            keep += [sb, cfg]
            samples.append(x)
            entries.append((tti, 1, cfg, [d_pl[b, 0].data_ptr(), d_pl[b, 1].data_ptr()], [1, 1]))
        d_x = torch.from_numpy(np.stack(samples).view(np.float32)).cuda()
        d_res = torch.full((2 * len(ttis),), 7, dtype=torch.int32, device="cuda")
        d_avg = torch.zeros(2 * len(ttis), dtype=torch.float32, device="cuda")
        assert ue.gpu_decode_batch(entries, d_x.data_ptr(), d_res.data_ptr(), d_avg.data_ptr(), -cfo, None) == \
            2 * len(ttis)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy()
        tot = eq = 0
        worst = 0
        for b in range(len(ttis)):
            for q in range(2):
                dp, n = ue.last_llr(b, q)
                want = wants[b][q]["llr"]
                assert n == want.size
                got = torch.empty(n, dtype=torch.int16)
                SCH._memcpy_d2h(got, dp, 2 * n)
                d = np.abs(got.numpy().astype(np.int32) - want.astype(np.int32))
                tot += n
                eq += int((d == 0).sum())
                worst = max(worst, int(d.max()))
                assert (d == 0).mean() >= eq_min, (b, q, (d == 0).mean())
                assert d.max() <= d_max, (b, q, int(d.max()), int((d > d_max).sum()))
                assert (res[2 * b + q] == 0) == (wants[b][q]["ret"] == 0), (b, q)
        LLR_STATS[f"{pred}_N{N}_snr{snr:g}_cfo{cfo:g}"] = dict(llrs=tot, equal_frac=eq / tot, max_abs_delta=worst,
                                                               cpu=_cpu_model())
        out = os.environ.get("SRSRAN_AMD_LLR_STATS")
        if out:
            with open(out, "w") as f:
                json.dump(LLR_STATS, f, indent=1)
        ue.free()
    finally:
        U.use_standard_symbol_size(True)


@pytest.mark.parametrize("nof_prb,N,tbs,cell_id", [(100, 1536, TBS, 1), (50, 768, 36696, 11), (25, 384, 18336, 5)])
def test_ue_dl_reference_default_rates(U, SCH, ora, nof_prb, N, tbs, cell_id):
    """the reference's default sampling rates (phy_common.c:31-35): an unmodified caller that never
    calls srsran_use_standard_symbol_size gets N = 1536 / 768 / 384 at 100 / 50 / 25 PRB.  The GPU
    UE DL chain (host-synchronous and batched) decodes like the oracle chain at that N: decode_tb
    return, payload bytes and average iterations."""
    U.use_standard_symbol_size(False)
    try:
        assert U.lib().srsran_symbol_sz(nof_prb) == N
        rng = np.random.default_rng(N)
        tti = 3
        pls, x, nre, grids, ce, st = _case(ora, rng, nof_prb=nof_prb, cell_id=cell_id, tti=tti, tbs=(tbs, tbs), N=N)
        assert x.shape[1] == 15 * N
        want = PC.pdsch_decode(ora, grids, ce, st["noise"], nof_prb, cell_id, 2, tti, 1, 0x1234, [tbs, tbs], [6, 6],
                               [0, 0])
        ue = U.UeDl(U.cell(nof_prb, 2, cell_id), 2)
        # host-synchronous path
        assert ue.fft_estimate(x, tti, 1) == 0
        sbs = [SCH.SoftbufferRx(nof_prb=nof_prb) for _ in range(2)]
        cfg = U.pdsch_cfg(nof_prb, nre, (tbs, tbs), (6, 6), softbuffers=sbs)
        ret, out = ue.decode_pdsch(cfg, tti, 1)
        assert ret == 0
        for q in range(2):
            assert want[q]["ret"] == 0 and out[q][0]
            assert np.array_equal(out[q][1][: tbs // 8], pls[q])
            assert np.array_equal(out[q][1][: tbs // 8 + 6], want[q]["data"][: tbs // 8 + 6])
            assert out[q][2] == pytest.approx(want[q]["avg"], abs=1e-6)
        # batched path
        sbs2 = [SCH.SoftbufferRx(nof_prb=nof_prb) for _ in range(2)]
        cfg2 = U.pdsch_cfg(nof_prb, nre, (tbs, tbs), (6, 6), softbuffers=sbs2)
        d_pl = torch.zeros((2, tbs // 8 + 64), dtype=torch.uint8, device="cuda")
        d_x = torch.from_numpy(x[None].view(np.float32)).cuda()
        d_res = torch.full((2,), 7, dtype=torch.int32, device="cuda")
        d_avg = torch.zeros(2, dtype=torch.float32, device="cuda")
        n = ue.gpu_decode_batch([(tti, 1, cfg2, [d_pl[0].data_ptr(), d_pl[1].data_ptr()], [1, 1])], d_x.data_ptr(),
                                d_res.data_ptr(), d_avg.data_ptr(), 0.0, None)
        assert n == 2
        torch.cuda.synchronize()
        res, pl, avg = d_res.cpu().numpy(), d_pl.cpu().numpy(), d_avg.cpu().numpy()
        for q in range(2):
            assert res[q] == want[q]["ret"] == 0
            assert np.array_equal(pl[q, : tbs // 8 + 6], want[q]["data"][: tbs // 8 + 6])
            assert avg[q] == pytest.approx(want[q]["avg"], abs=1e-6)
        ue.free()
        for sb in sbs + sbs2:
            sb.free()
    finally:
        U.use_standard_symbol_size(True)


@pytest.mark.parametrize("scheme,pmi,snr", [("sm", 0, 30.0), ("sm", 1, 30.0), ("cdd", 0, 30.0), ("cdd", 0, 9.0)])
def test_pdsch_one_codeword_two_layers(U, SCH, ora, scheme, pmi, snr):
    """one TB on two layers (SM codebook pmi / CDD): the predecoder's two layers are layer-demapped
    over n/2 layer symbols (srsran_layerdemap_type, pdsch.c:838-863) and the codeword's CSI
    correction reads layer 0's CSI, as the reference does; frequency-domain grids and exact estimates
    fed to both the GPU and the oracle chain: return, payload and iterations equal"""
    rng = np.random.default_rng(31 + pmi + int(snr))
    nof_prb, cell_id, nports, tti, cfi = 100, 5, 2, 2, 1
    mask = S.pdsch_mask(nof_prb, nports, cell_id, cfi, tti % 10)
    nre = int(mask.sum())
    pl = rng.integers(0, 256, TBS // 8, dtype=np.uint8)
    G = nre * 6
    e = S.dlsch_encode(TBS, 6, 0, G, pl, Nl=2)
    d = S.modulate(e ^ S.gold(S.pdsch_seed(0x1234, 0, 2 * (tti % 10), cell_id), G), 6)
    half = nre // 2
    ports = S.precode([d[0:2 * half:2], d[1:2 * half:2]], scheme, codebook=pmi)
    H = (rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))) / np.sqrt(2) + np.eye(2)
    grids = np.zeros((2, 14 * 12 * nof_prb), np.complex128)
    for p in range(nports):
        g = S.crs_grid(cell_id, nof_prb, nports, p, tti % 10)
        v = np.zeros(nre, np.complex128)
        v[:half] = ports[p]  # the layer symbols fill the first n/2 PDSCH REs (the precoder's length)
        g[mask] = v
        for r in range(2):
            grids[r] += H[r, p] * g.reshape(-1)
    sd = np.sqrt(np.mean(np.abs(grids) ** 2) / 10 ** (snr / 10) / 2)
    grids = (grids + sd * (rng.standard_normal(grids.shape) + 1j * rng.standard_normal(grids.shape))).astype(np.complex64)
    ce = np.zeros((nports, 2, grids.shape[1]), np.complex64)
    for p in range(nports):
        for r in range(2):
            ce[p, r] = H[r, p]
    noise = float(2 * sd * sd)
    ref = PC.pdsch_decode(ora, grids, ce, noise, nof_prb, cell_id, nports, tti, cfi, 0x1234, [TBS], [6], [0],
                          scheme=scheme, pmi=pmi, layers=2)
    sb = SCH.SoftbufferRx(nof_prb=nof_prb)
    cfg = U.pdsch_cfg(nof_prb, nre, [TBS], [6], scheme=scheme, pmi=pmi, softbuffers=[sb])
    cfg.grant.nof_layers = 2
    pd = U.Pdsch(U.cell(nof_prb, nports, cell_id), 2)
    ret, out = pd.decode(cfg, tti, cfi, grids, ce, noise)
    assert ret == 0
    crc, payload, avg = out[0]
    assert crc == (ref[0]["ret"] == 0)
    assert np.array_equal(payload[:TBS // 8 + 6], ref[0]["data"][:TBS // 8 + 6])
    assert avg == pytest.approx(ref[0]["avg"], abs=1e-6)
    if snr > 20:
        assert crc and np.array_equal(payload[:TBS // 8], pl)
    pd.free()
    sb.free()


@pytest.mark.parametrize("nports,mix,opts", [
    (2, [("cdd", 0, 6), ("sm", 0, 6), ("sm", 1, 4), ("cdd", 0, 2)], dict()),
    (2, [("cdd", 0, 6), ("sm", 1, 6)], dict(csi_enable=False)),
    (2, [("sm", 0, 8), ("cdd", 0, 6)], dict(power_scale=True, p_a=-3.0, p_b=2)),
    (2, [("cdd", 0, 6), ("sm", 0, 4)], dict(zf=True)),
    (1, [("port0", 0, 4), ("port0", 0, 6), ("port0", 0, 2)], dict()),
])
def test_pdsch_fused_matches_two_kernel_path(U, SCH, ora, nports, mix, opts):
    """the opt-in fused predecode + LLR kernel (SRSRAN_AMD_PDSCH_FUSED=1: llr_kernel.hip fused_llr_batch_kernel after
    the CSI-pair pre-pass; eligible batches: PORT0, or SM / CDD with two codewords of one modulation, int16 LLRs, no
    EVM) against the default two-kernel path (predecoder -> symbols + CSI in HBM -> LLR kernel): every LLR
    bit-identical, the same decode results.  Mixed schemes and modulations in one batch, 256QAM included (Qm 8 is carried as MCS
    tables' 256QAM; synth sends one modulation a subframe)."""
    tbs_of = {2: 12576, 4: 30576, 6: 46888, 8: 63776}
    rng = np.random.default_rng(900 + nports + len(mix))
    ue = U.UeDl(U.cell(100, nports, 1), 2)
    entries, samples, keep = [], [], []
    ttis = [1, 2, 3, 4, 6, 7, 8][: len(mix)]
    ncw = [1 if s == "port0" else 2 for s, _, _ in mix]
    d_pl = torch.zeros((len(mix), 2, 63776 // 8 + 64), dtype=torch.uint8, device="cuda")
    for b, ((scheme, pmi, qm), tti) in enumerate(zip(mix, ttis)):
        tbs, Qm = (tbs_of[qm],) * ncw[b], (qm,) * ncw[b]
        kw = dict(channel=[[1], [0.5 + 0.5j]]) if scheme == "port0" else {}
        pls, x, nre, _, _, _ = _case(ora, rng, nports=nports, tti=tti, tbs=tbs, Qm=Qm, scheme=scheme, pmi=pmi,
                                     snr_db=25.0, **kw)
        sb = [SCH.SoftbufferRx(nof_prb=100) for _ in tbs]
        cfg = U.pdsch_cfg(100, nre, tbs, Qm, scheme=scheme, pmi=pmi, softbuffers=sb, nof_ports=nports, **opts)
        keep += [sb, cfg, pls]
        samples.append(x)
        entries.append((tti, 1, cfg, [d_pl[b, q].data_ptr() for q in range(ncw[b])], [1] * ncw[b]))
    d_x = torch.from_numpy(np.stack(samples).view(np.float32)).cuda()

    def run(fused):
        os.environ["SRSRAN_AMD_PDSCH_FUSED"] = "1" if fused else "0"
        try:
            d_res = torch.full((2 * len(mix),), 7, dtype=torch.int32, device="cuda")
            d_avg = torch.zeros(2 * len(mix), dtype=torch.float32, device="cuda")
            assert ue.gpu_decode_batch(entries, d_x.data_ptr(), d_res.data_ptr(), d_avg.data_ptr()) == sum(ncw)
            torch.cuda.synchronize()
            llrs = []
            for b in range(len(mix)):
                for q in range(ncw[b]):
                    dp, n = ue.last_llr(b, q)
                    got = torch.empty(n, dtype=torch.int16)
                    SCH._memcpy_d2h(got, dp, 2 * n)
                    llrs.append(got.numpy().copy())
            return d_res.cpu().numpy(), d_avg.cpu().numpy(), llrs, d_pl.cpu().numpy()
        finally:
            os.environ.pop("SRSRAN_AMD_PDSCH_FUSED", None)

    r0, a0, l0, p0 = run(False)
    r1, a1, l1, p1 = run(True)
    assert len(l0) == len(l1) == sum(ncw)
    for i, (x0, x1) in enumerate(zip(l0, l1)):
        assert x0.size == x1.size and np.array_equal(x0, x1), (i, int((x0 != x1).sum()))
    assert np.array_equal(r0, r1) and np.array_equal(a0, a1) and np.array_equal(p0, p1)
    assert (r1[r1 != 7] == 0).all()  # every TB decodes at 25 dB
    ue.free()


def _to_sc16(x, rng_bits=14):
    """quantise complex samples to int16 I/Q with the scale a radio driver would report: |x| max -> 2^14"""
    scale = np.float32(np.abs(np.concatenate([x.real, x.imag])).max() / (1 << rng_bits))
    q = np.empty(x.shape + (2,), np.int16)
    q[..., 0] = np.clip(np.rint(x.real / scale), -32768, 32767)
    q[..., 1] = np.clip(np.rint(x.imag / scale), -32768, 32767)
    return q, float(scale)


@pytest.mark.parametrize("cfo", [0.0, 150.0 / 30.72e6])
def test_ue_dl_batch_sc16_equals_float(U, SCH, ora, cfo):
    """srsran_ue_dl_gpu_decode_batch_sc16 on int16 I/Q samples == srsran_ue_dl_gpu_decode_batch on the same samples
    converted on the host as (float)x * scale: the same payloads, iteration counts and every LLR of every TB (the
    conversion in the OFDM load computes the host's single float product)"""
    rng = np.random.default_rng(31)
    nsf = 3
    samples, entries_f, entries_q, sbs, pls_all = [], [], [], [], []
    d_pl = torch.zeros((2, nsf, 2, TBS // 8 + 64), dtype=torch.uint8, device="cuda")
    for b in range(nsf):
        pls, x, nre, _, _, _ = _case(ora, rng, tti=3 + b, cfo=cfo)
        samples.append(x)
        pls_all.append(pls)
        for k, ent in enumerate((entries_f, entries_q)):
            sb = [SCH.SoftbufferRx(nof_prb=100) for _ in range(2)]
            sbs += sb
            cfg = U.pdsch_cfg(100, nre, (TBS, TBS), (6, 6), softbuffers=sb)
            ent.append((3 + b, 1, cfg, [d_pl[k, b, 0].data_ptr(), d_pl[k, b, 1].data_ptr()], [1, 1]))
    q, scale = _to_sc16(np.stack(samples))
    xf = (q[..., 0].astype(np.float32) * np.float32(scale) + 1j * (q[..., 1].astype(np.float32) * np.float32(scale)))
    xf = xf.astype(np.complex64)
    d_xf = torch.from_numpy(xf.view(np.float32)).cuda()
    d_xq = torch.from_numpy(q).cuda()
    out = []
    for k in range(2):
        ue = U.UeDl(U.cell(100, 2, 1), 2)
        d_res = torch.full((2 * nsf,), 7, dtype=torch.int32, device="cuda")
        d_avg = torch.zeros(2 * nsf, dtype=torch.float32, device="cuda")
        if k == 0:
            n = ue.gpu_decode_batch(entries_f, d_xf.data_ptr(), d_res.data_ptr(), d_avg.data_ptr(), -cfo, None)
        else:
            n = ue.gpu_decode_batch_sc16(entries_q, d_xq.data_ptr(), scale, d_res.data_ptr(), d_avg.data_ptr(), -cfo,
                                         None)
        assert n == 2 * nsf
        torch.cuda.synchronize()
        llrs = []
        for b in range(nsf):
            for t in range(2):
                p, cnt = ue.last_llr(b, t)
                h = torch.empty(cnt, dtype=torch.int16)
                SCH._memcpy_d2h(h, p, 2 * cnt)
                llrs.append(h.numpy().copy())
        out.append((d_res.cpu().numpy(), d_avg.cpu().numpy(), llrs))
        ue.free()
    pl = d_pl.cpu().numpy()
    assert (out[0][0] == 0).all() and np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    for b in range(nsf):
        for t in range(2):
            assert np.array_equal(pl[0, b, t], pl[1, b, t])
            assert np.array_equal(pl[1, b, t, : TBS // 8], pls_all[b][t])
            assert np.array_equal(out[0][2][2 * b + t], out[1][2][2 * b + t])
    for sb in sbs:
        sb.free()


@pytest.mark.gpu
def test_ue_dl_batches_on_worker_streams(U, SCH, ora):
    """srsran_gpu_worker_stream_create: two UE DL objects (two PHY workers) decode batches on streams with a hardware
    queue each, enqueued back to back without a host wait between them: both decode every TB of the same subframes
    like the oracle's payloads, with the same iteration counts"""
    rng = np.random.default_rng(37)
    nsf = 2
    samples, pls_all, nres = [], [], []
    for b in range(nsf):
        pls, x, nre, _, _, _ = _case(ora, rng, tti=5 + b, cfo=0.0)
        samples.append(x)
        pls_all.append(pls)
        nres.append(nre)
    d_x = torch.from_numpy(np.ascontiguousarray(np.stack(samples)).view(np.float32)).cuda()
    d_pl = torch.zeros((2, nsf, 2, TBS // 8 + 64), dtype=torch.uint8, device="cuda")
    d_res = torch.full((2, 2 * nsf), 7, dtype=torch.int32, device="cuda")
    d_avg = torch.zeros((2, 2 * nsf), dtype=torch.float32, device="cuda")
    sbs, ues, streams = [], [], []
    torch.cuda.synchronize()
    for w in range(2):
        ent = []
        for b in range(nsf):
            sb = [SCH.SoftbufferRx(nof_prb=100) for _ in range(2)]
            sbs += sb
            cfg = U.pdsch_cfg(100, nres[b], (TBS, TBS), (6, 6), softbuffers=sb)
            ent.append((5 + b, 1, cfg, [d_pl[w, b, 0].data_ptr(), d_pl[w, b, 1].data_ptr()], [1, 1]))
        ue = U.UeDl(U.cell(100, 2, 1), 2)
        ws = U.WorkerStream(torch.device("cuda", 0))
        assert ws.cuda_stream
        ues.append(ue)
        streams.append(ws)
        assert ue.gpu_decode_batch(ent, d_x.data_ptr(), d_res[w].data_ptr(), d_avg[w].data_ptr(), 0.0,
                                   ws.cuda_stream) == 2 * nsf
    for ws in streams:
        ws.stream.synchronize()
    res, avg, pl = d_res.cpu().numpy(), d_avg.cpu().numpy(), d_pl.cpu().numpy()
    assert (res == 0).all() and np.array_equal(avg[0], avg[1])
    for w in range(2):
        for b in range(nsf):
            for t in range(2):
                assert np.array_equal(pl[w, b, t, : TBS // 8], pls_all[b][t])
    for ue in ues:
        ue.free()
    for ws in streams:
        ws.free()
    for sb in sbs:
        sb.free()
