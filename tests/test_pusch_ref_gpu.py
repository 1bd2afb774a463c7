"""The GPU PUSCH receive path against fixtures recorded from the reference's own compiled chest_ul.c, pusch.c and sch.c
(tests/golden/make_pusch_golden.py; case table, tolerances and distances in tests/pusch_cases.py).  It reads the fixture
only: no result here is compared with oracle/pusch.py, and oracle/_ref is not opened.

* sync path, every case: srsran_chest_ul_estimate_pusch on an identity-prefilled result (the whole estimate grid and
  all ten scalars), then srsran_pusch_decode (crc, payload, UCI, avg_iterations_block, epre_dbfs, the cfg write-backs,
  and through srsran_pusch_gpu_last_soft the de-precoded symbols and the LLRs);
* the decoder alone: the fixture's reference estimate and noise in a srsran_chest_ul_res_t without device copy (the
  host-upload path of srsran_pusch_decode) must reproduce the recorded decisions and soft values;
* batch path: every decodable case of four cells in one srsran_pusch_gpu_decode_batch call (c11b, which needs c11a's
  soft buffer, in a second one).

Floats are allowed 4 x the distance the reference's own builds lie from the float64 evaluation (pusch_cases.TOL).  The
library generates its own DMRS, and at many PRBs single elements of a float DMRS differ between any two builds, the
reference's own included (pusch_cases.dmrs_exact).  So every float is compared twice: with pusch_cases.rx_f64 run on
the library's own DMRS, within TOL; and with the fixture, within TOL plus the distance between rx_f64 on the library's
DMRS and rx_f64 on the fixture's, which is zero where the two DMRS are equal and below 1e-3 up to 6 PRB.  The DMRS
itself is held to its per-case bound in tests/test_pusch_golden.py.  The decoder-alone test has no DMRS in it and
uses TOL as it is.

The retransmission c11b decodes only on the soft buffer that c11a left: the sync and decoder-alone tests decode it once
more on a reset soft buffer and expect the reference's failure there.

LLRs: every |difference| is at most 1 LSB and the share of unequal LLRs at most LLR_SHARE_TOL (in the decoder-alone
test, where the estimate is the reference's own, at most the 1e-3 this project applies to chain LLRs).  The HARQ-ACK decoder
zeroes its positions of the LLR buffer in place (as sch.c does), so LLRs are compared in the cases without HARQ-ACK.
"""
import ctypes
import os

import numpy as np
import pytest

import pusch_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDS = [c["name"] for c in C.CASES]
DECODE = [c for c in C.CASES if c["decode"]]


@pytest.fixture(scope="module")
def fx():
    return C.Fixture(GOLDEN)


@pytest.fixture(scope="module")
def env():
    from srsran_4g_amd import pusch as P
    from srsran_4g_amd import sch as S
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.skip("no HIP device")
    return P, S


class Check:
    """collects every distance of a test, prints it, and fails at the end with all that miss their tolerance"""

    def __init__(self, name):
        self.name, self.bad = name, []

    def __call__(self, quantity, kind, got, want, tol):
        d = C.err(kind, got, want)
        print(self.name, quantity, "%.3g (allowed %.3g)" % (d, tol))
        if not d <= tol:
            self.bad.append((quantity, d, tol))

    def same(self, quantity, got, want):
        print(self.name, quantity, got if np.size(got) < 12 else "...", "==", want if np.size(want) < 12 else "...")
        if not np.array_equal(got, want):
            self.bad.append((quantity, got, want))

    def llr(self, got, want, share_tol=C.LLR_SHARE_TOL):
        dl = np.abs(np.asarray(got, np.int32) - np.asarray(want, np.int32))
        share = float(np.mean(dl != 0))
        print(self.name, "llr max |d| %d share %.3g (allowed %d, %.3g)" % (dl.max(), share, C.LLR_MAX_LSB, share_tol))
        if dl.max() > C.LLR_MAX_LSB or share > share_tol:
            self.bad.append(("llr", int(dl.max()), share))

    def done(self):
        assert not self.bad, self.bad


def make_cell(c):
    from srsran_4g_amd.ue_dl import cell
    x = cell(nof_prb=c["nof_prb"], cell_id=c["cell_id"])
    x.cp = c["cp"]
    return x


def dmrs_cfg(P, c):
    d = P.srsran_refsignal_dmrs_pusch_cfg_t()
    d.cyclic_shift, d.delta_ss, d.group_hopping_en, d.sequence_hopping_en = c["dmrs"]
    return d


def new_chest(P, c):
    ch = P.ChestUl(make_cell(c), dmrs_cfg(P, c), max_prb=c["nof_prb"])
    if c["smooth"] != 3:
        ch.q.smooth_filter_len = c["smooth"]
    return ch


def sf_cfg(P, c):
    sf = P.srsran_ul_sf_cfg_t()
    sf.tti, sf.shortened = c["tti"], bool(c["shortened"])
    return sf


def models(P, fx, c):
    """rx_f64 on the library's own DMRS and on the fixture's"""
    ret, r = P.dmrs(make_cell(c), dmrs_cfg(P, c), c["L"], c["tti"] % 10, c["n_dmrs"])
    assert ret == 0
    grid = fx.grid(c)
    return C.rx_f64(grid, c, r, bool(c["decode"])), C.rx_f64(grid, c, fx.get(c, "dmrs"), bool(c["decode"]))


def check_float(ck, name, got, want, own, fixm):
    """got against the float64 model on the library's DMRS, and against the fixture with the models' distance added"""
    kind = C.KIND[name]
    ck(name + " (model)", kind, got, own, C.TOL[name])
    ck(name, kind, got, want, C.TOL[name] + C.err(kind, own, fixm))


def check_estimate(ck, c, fx, ce_rows, scal, own, fixm):
    check_float(ck, "ce", ce_rows, fx.get(c, "ce"), own["ce"], fixm["ce"])
    want = fx.scalars(c)
    for name in C.SCALARS:
        if name in scal:
            check_float(ck, name, scal[name], want[name], own[name], fixm[name])


def check_decisions(ck, c, fx, crc, data, uci, avg, cfg):
    ck.same("crc", int(crc), int(fx.get(c, "crc")))
    if int(fx.get(c, "crc")):
        ck.same("payload", np.asarray(data[:c["tbs"] // 8]), fx.get(c, "payload"))
    ck.same("uci", C.uci_fields(c, uci), list(fx.get(c, "uci")))
    ck.same("avg_iterations_block", float(avg), float(fx.get(c, "res")[0]))
    ck.same("cfg write-backs", [cfg.last_O_cqi, cfg.grant.tb.mod, cfg.grant.tb.nof_bits], list(fx.get(c, "writeback")))


def check_alone(ck, env, fx, c, pu, sf, chest_res, grid):
    """a retransmission once more on a reset soft buffer: the reference fails there (the generator refuses to write
    otherwise), so a decode that ignores, resets or corrupts what the first transmission left cannot pass both"""
    P, S = env
    if not c["harq_after"]:
        return
    sb = S.SoftbufferRx(nof_prb=c["nof_prb"])
    cfg = C.build_cfg(c, S)
    cfg.softbuffers.rx = ctypes.pointer(sb.s)
    ret, out, _ = pu.decode(sf, cfg, chest_res, grid, max(c["tbs"] // 8, 1))
    assert ret == 0
    crc, avg = fx.get(c, "alone")
    assert int(crc) == 0 and int(fx.get(c, "crc")) == 1
    ck.same("on a reset soft buffer: crc", int(out.crc), int(crc))
    ck.same("on a reset soft buffer: avg_iterations_block", float(out.avg_iterations_block), float(avg))


def rows_of(c, ce):
    ns, M, p0 = C.nsymb_slot(c["cp"]), 12 * c["L"], 12 * c["n_prb"]
    return np.stack([ce[s * ns, p0:p0 + M] for s in (0, 1)])


def soft_buffer(env, fx, c, run):
    """a fresh soft buffer; for a retransmission, the one the first transmission (run here too) has left"""
    P, S = env
    sb = S.SoftbufferRx(nof_prb=c["nof_prb"])
    if c["harq_after"]:
        run(env, fx, C.by_name()[c["harq_after"]], sb)
    return sb


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_sync_path(env, fx, c):
    sync_path(env, fx, c, soft_buffer(env, fx, c, sync_path))


def sync_path(env, fx, c, sb):
    P, S = env
    grid, sf, ck = fx.grid(c), sf_cfg(P, c), Check(c["name"])
    own, fixm = models(P, fx, c)
    cfg = C.build_cfg(c, S)
    cfg.softbuffers.rx = ctypes.pointer(sb.s)
    ch = new_chest(P, c)
    P.lib().srsran_chest_ul_res_set_identity(ctypes.byref(ch.res))
    assert ch.estimate(sf, cfg, grid) == 0
    ce = ch.ce(grid.size).reshape(grid.shape)
    # the whole grid: every symbol of a slot holds the slot's row at n_prb, the prefill everywhere else
    whole = fx.ce_grid(c)
    p0, M = 12 * c["n_prb"], 12 * c["L"]
    outside = np.ones(ce.shape, bool)
    outside[:, p0:p0 + M] = False
    ck.same("prefill outside the allocation", ce[outside], whole[outside])
    ns = C.nsymb_slot(c["cp"])
    for s in (0, 1):
        blk = ce[s * ns:(s + 1) * ns, p0:p0 + M]
        ck.same("slot %d: every symbol holds the row" % s, blk, np.broadcast_to(blk[:1], blk.shape))
    check_estimate(ck, c, fx, rows_of(c, ce), {n: getattr(ch.res, n) for n in C.SCALARS}, own, fixm)
    if c["decode"]:
        pu = P.Pusch(make_cell(c), max_prb=c["nof_prb"])
        ret, out, data = pu.decode(sf, cfg, ch.res, grid, max(c["tbs"] // 8, 1))
        assert ret == 0
        check_decisions(ck, c, fx, out.crc, data, out.uci, out.avg_iterations_block, cfg)
        check_float(ck, "epre_dbfs", out.epre_dbfs, fx.get(c, "res")[1], own["epre_dbfs"], fixm["epre_dbfs"])
        assert np.isnan(out.evm)
        sym, llr = pu.read_soft()
        assert sym.size == cfg.grant.nof_re and llr.size == cfg.grant.tb.nof_bits
        if c["soft"]:
            check_float(ck, "sym", sym, fx.get(c, "sym"), own["sym"], fixm["sym"])
            if not c["nack"]:
                ck.llr(llr, fx.get(c, "llr"))
        check_alone(ck, env, fx, c, pu, sf, ch.res, grid)
        pu.free()
    ch.free()
    ck.done()


@pytest.mark.parametrize("c", DECODE, ids=[c["name"] for c in DECODE])
def test_decoder_on_reference_estimate(env, fx, c):
    """srsran_pusch_decode fed the reference's own estimate through a result that has no device copy"""
    decoder_alone(env, fx, c, soft_buffer(env, fx, c, decoder_alone))


def decoder_alone(env, fx, c, sb):
    P, S = env
    grid, sf, ck = fx.grid(c), sf_cfg(P, c), Check(c["name"])
    cfg = C.build_cfg(c, S)
    cfg.softbuffers.rx = ctypes.pointer(sb.s)
    ce = np.ascontiguousarray(fx.ce_grid(c))
    res = P.srsran_chest_ul_res_t()  # host memory only: gpu stays NULL
    res.ce = ce.view(np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    res.nof_re = ce.size
    res.noise_estimate = float(fx.scalars(c)["noise_estimate"])
    pu = P.Pusch(make_cell(c), max_prb=c["nof_prb"])
    ret, out, data = pu.decode(sf, cfg, res, grid, max(c["tbs"] // 8, 1))
    assert ret == 0
    check_decisions(ck, c, fx, out.crc, data, out.uci, out.avg_iterations_block, cfg)
    ck("epre_dbfs", "db", out.epre_dbfs, fx.get(c, "res")[1], C.TOL["epre_dbfs"])
    if c["soft"]:
        sym, llr = pu.read_soft()
        ck("sym", "rms", sym, fx.get(c, "sym"), C.TOL["sym"])
        if not c["nack"]:  # same estimate and noise as the reference had: the project's bound for chain LLRs
            ck.llr(llr, fx.get(c, "llr"), min(C.LLR_SHARE_TOL, C.LLR_SHARE_CHAIN))
    check_alone(ck, env, fx, c, pu, sf, res, grid)
    pu.free()
    ck.done()


def test_batch_path(env, fx):
    import torch
    P, S = env
    first = [c for c in DECODE if not c["harq_after"]]
    second = [c for c in DECODE if c["harq_after"]]
    assert len({(c["nof_prb"], c["cell_id"]) for c in first}) >= 4  # several cells at once
    pu = P.Pusch(make_cell(first[0]), max_prb=100)
    sbs, keep, bad = {}, [], []
    for group in (first, second):
        n = len(group)
        arr = (P.srsran_pusch_gpu_ue_t * n)()
        res = (P.srsran_pusch_res_t * n)()
        cres = (P.srsran_chest_ul_res_t * n)()
        per = []
        for i, c in enumerate(group):
            ch, sf, cfg = new_chest(P, c), sf_cfg(P, c), C.build_cfg(c, S)
            sb = sbs[c["harq_after"]] if c["harq_after"] else S.SoftbufferRx(nof_prb=c["nof_prb"])
            sbs[c["name"]] = sb
            cfg.softbuffers.rx = ctypes.pointer(sb.s)
            grid = fx.grid(c)
            d_grid = torch.from_numpy(grid.view(np.float32).reshape(-1).copy()).cuda()
            data = np.zeros(max(c["tbs"] // 8, 1) + 64, np.uint8)
            ce = np.ones(grid.shape, np.complex64)
            arr[i].chest, arr[i].sf, arr[i].cfg = ctypes.pointer(ch.q), ctypes.pointer(sf), ctypes.pointer(cfg)
            arr[i].d_sf_symbols, arr[i].new_data = d_grid.data_ptr(), 0 if c["harq_after"] else 1
            res[i].data = data.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
            cres[i].ce = ce.view(np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))
            cres[i].nof_re = ce.size
            per.append((ch, cfg, data, ce))
            keep += [sf, d_grid]
        assert P.lib().srsran_pusch_gpu_decode_batch(ctypes.byref(pu.q), n, arr, cres, res) == 0
        with pytest.raises(RuntimeError):  # the soft-value accessor belongs to the host-sync decode
            pu.last_soft()
        for i, c in enumerate(group):
            ch, cfg, data, ce = per[i]
            ck = Check("batch " + c["name"])
            own, fixm = models(P, fx, c)
            check_estimate(ck, c, fx, rows_of(c, ce), {n: getattr(cres[i], n) for n in C.SCALARS}, own, fixm)
            check_decisions(ck, c, fx, res[i].crc, data, res[i].uci, res[i].avg_iterations_block, cfg)
            check_float(ck, "epre_dbfs", res[i].epre_dbfs, fx.get(c, "res")[1], own["epre_dbfs"], fixm["epre_dbfs"])
            bad += [(c["name"],) + b for b in ck.bad]
            ch.free()
    pu.free()
    assert not bad, bad
