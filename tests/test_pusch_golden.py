"""The PUSCH restatements and host code against fixtures recorded from the reference's own compiled pusch.c, sch.c,
chest_ul.c and refsignal_ul.c (tests/golden/make_pusch_golden.py; case table and tolerances in tests/pusch_cases.py).
No GPU.

tests/test_pusch_gpu.py compares the kernels with oracle/pusch.py; this module holds oracle/pusch.py itself (dmrs,
chest, symbols, llrs and the chain's decisions) to what the reference computed, so that those comparisons keep their
meaning, and the library's host DMRS (srsran_refsignal_dmrs_pusch_gen_cell) as well.

The DMRS.  Two builds of the reference disagree with each other where the float argument of the complex exponential is
large (pusch_cases.DMRS_DIST), so each DMRS is held to the exact float64 one within 1.5 float ulp at the largest argument
of the case (pusch_cases.dmrs_exact), and to the fixture's within twice that.  The estimator restatement is then fed
the fixture's DMRS, as the reference's estimator was.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)

import pusch as OP  # noqa: E402  (oracle/pusch.py)
import pusch_cases as C  # noqa: E402
from srsran_4g_amd import pusch as P  # noqa: E402
from srsran_4g_amd import sch as S  # noqa: E402
from srsran_4g_amd.ue_dl import cell as make_cell  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
needs_ref = pytest.mark.skipif(not OP.ref_available(), reason="oracle/_ref not built")
IDS = [c["name"] for c in C.CASES]


@pytest.fixture(scope="module")
def fx():
    return C.Fixture(GOLDEN)


@pytest.fixture(scope="module")
def po():
    return OP.PuschOracle()


def test_tables_match_fixture(fx):
    """the numbers written into pusch_cases.py are the ones the generator measured and stored"""
    assert fx.cases == json.loads(json.dumps(C.CASES))
    assert fx.allow["measured"] == pytest.approx(C.MEASURED, rel=1e-3) and set(fx.allow["measured"]) == set(C.KIND)
    assert fx.allow["llr_share"] == pytest.approx(C.LLR_SHARE_REF, rel=1e-3)
    assert set(fx.allow["dmrs"]) == set(C.DMRS_DIST) == {c["name"] for c in C.CASES}
    for name, d in fx.allow["dmrs"].items():
        assert d == pytest.approx(C.DMRS_DIST[name], rel=1e-3), name
        assert d["bound"] == pytest.approx(C.dmrs_exact(C.by_name()[name])[1], rel=1e-3)
    assert os.path.getsize(os.path.join(GOLDEN, C.FIXTURE)) <= __import__("chest_cases").MAX_FIXTURE_BYTES


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_float64_model_matches_reference(fx, c):
    """pusch_cases.rx_f64 (which tests/test_pusch_ref_gpu.py also uses) on the fixture's grid and DMRS: the values the
    generator stored, and the reference's results within the measured distances"""
    f = C.rx_f64(fx.grid(c), c, fx.get(c, "dmrs"), bool(c["decode"]))
    stored = fx.get(c, "f64")
    for i, name in enumerate(C.SCALARS):
        assert C.err("rel" if C.KIND[name] == "rel" else "abs", f[name], stored[i]) <= 1e-9, name
        assert C.err(C.KIND[name], fx.scalars(c)[name], f[name]) <= C.MEASURED[name], name
    assert C.err("rms", fx.get(c, "ce"), f["ce"]) <= C.MEASURED["ce"]
    if fx.has(c, "sym"):
        assert C.err("rms", fx.get(c, "sym"), f["sym"]) <= C.MEASURED["sym"]


def _dmrs_cfg(c):
    d = P.srsran_refsignal_dmrs_pusch_cfg_t()
    d.cyclic_shift, d.delta_ss, d.group_hopping_en, d.sequence_hopping_en = c["dmrs"]
    return d


def _cell(c):
    cell = make_cell(nof_prb=c["nof_prb"], cell_id=c["cell_id"])
    cell.cp = c["cp"]
    return cell


@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_library_dmrs(fx, c):
    ret, r = P.dmrs(_cell(c), _dmrs_cfg(c), c["L"], c["tti"] % 10, c["n_dmrs"])
    assert ret == 0
    exact, bound = C.dmrs_exact(c)
    d_exact, d_fix = C.err("abs", r, exact), C.err("abs", r, fx.get(c, "dmrs"))
    print(c["name"], "library DMRS: from exact %.3e, from the fixture %.3e, bound %.3e" % (d_exact, d_fix, bound))
    assert C.err("abs", fx.get(c, "dmrs"), exact) <= bound
    assert d_exact <= bound and d_fix <= 2 * bound


@needs_ref
@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_oracle_dmrs(fx, po, c):
    cs, dss, gh, sh = c["dmrs"]
    r = po.dmrs(c["cell_id"], c["cp"], cs, dss, bool(gh), bool(sh), c["L"], c["tti"] % 10, c["n_dmrs"])
    exact, bound = C.dmrs_exact(c)
    assert C.err("abs", r, exact) <= bound and C.err("abs", r, fx.get(c, "dmrs")) <= 2 * bound


@needs_ref
@pytest.mark.parametrize("c", C.CASES, ids=IDS)
def test_oracle_chest(fx, po, c):
    grid = fx.grid(c)
    est = po.chest(grid, c["nof_prb"], c["cp"], c["L"], [c["n_tilde"]] * 2, [c["n_prb"]] * 2, fx.get(c, "dmrs"),
                   meas_ta=bool(c["meas_ta"]), smooth=c["smooth"] == 3, ce_in=np.ones_like(grid))
    want = fx.scalars(c)
    assert C.err("rms", est["ce"], fx.ce_grid(c)) <= C.TOL["ce"]  # the whole grid: rows at n_prb, identity elsewhere
    for name, key in (("noise_estimate", "noise"), ("cfo_hz", "cfo_hz"), ("ta_us", "ta_us"), ("rsrp", "rsrp"), ("epre", "epre")):
        assert C.err(C.KIND[name], est[key], want[name]) <= C.TOL[name], (name, est[key], want[name])


SOFT = [c for c in C.CASES if c["soft"]]


@needs_ref
@pytest.mark.parametrize("c", SOFT, ids=[c["name"] for c in SOFT])
def test_oracle_symbols_and_llrs(fx, po, c):
    grid, want = fx.grid(c), fx.scalars(c)
    d = po.symbols(grid, fx.ce_grid(c), float(want["noise_estimate"]), c["cp"], bool(c["shortened"]), c["L"], [c["n_tilde"]] * 2)
    assert C.err("rms", d, fx.get(c, "sym")) <= C.TOL["sym"]
    mod = int(fx.get(c, "writeback")[1])
    # the compiled demapper / descrambler on the reference's own symbols: the reference's LLRs, bit for bit
    assert np.array_equal(po.llrs(fx.get(c, "sym"), mod, c["rnti"], c["tti"], c["cell_id"]), fx.get(c, "llr"))
    dl = np.abs(po.llrs(d, mod, c["rnti"], c["tti"], c["cell_id"]).astype(np.int32) - fx.get(c, "llr"))
    assert dl.max() <= C.LLR_MAX_LSB and np.mean(dl != 0) <= C.LLR_SHARE_TOL, (dl.max(), np.mean(dl != 0))


DECODE = [c for c in C.CASES if c["decode"]]


@needs_ref
def test_oracle_chain_decisions(fx, po):
    """oracle estimator -> equaliser / inverse DFT -> compiled demapper / descrambler -> compiled UCI receiver ->
    oracle UL-SCH decoder: crc, payload, UCI, iterations and write-backs of every decodable case, in table order (c11b
    runs on c11a's soft-buffer state)"""
    import uci as RU
    state = {}
    for c in DECODE:
        grid = fx.grid(c)
        est = po.chest(grid, c["nof_prb"], c["cp"], c["L"], [c["n_tilde"]] * 2, [c["n_prb"]] * 2, fx.get(c, "dmrs"),
                       meas_ta=bool(c["meas_ta"]), smooth=c["smooth"] == 3)
        d = po.symbols(grid, est["ce"], est["noise"], c["cp"], bool(c["shortened"]), c["L"], [c["n_tilde"]] * 2)
        cfg = C.build_cfg(c, S)
        lo, mod, nbits = (int(x) for x in fx.get(c, "writeback"))
        if not c["enable_64qam"] and c["Qm"] == 6:  # pusch.c:374-380
            cfg.grant.tb.mod, cfg.grant.tb.nof_bits = S.SRSRAN_MOD_16QAM, cfg.grant.nof_re * 4
        assert (cfg.grant.tb.mod, cfg.grant.tb.nof_bits) == (mod, nbits)
        assert S.lib().srsran_cqi_size(ctypes.byref(cfg.uci_cfg.cqi)) == lo
        Qm = nbits // cfg.grant.nof_re
        q = po.llrs(d, mod, c["rnti"], c["tti"], c["cell_id"])
        seq = po.ora.sequence_bits(OP.pusch_seed(c["rnti"], 2 * (c["tti"] % 10), c["cell_id"]), q.size)
        got = S.srsran_uci_value_t()
        _, _, g, (Qri, Qcqi, G, Qack) = RU.RefUci().rx(cfg, q, seq, got)
        oret, odata, _, oavg, st = po.ora.dlsch_decode(c["tbs"], Qm, c["rv"], g[Qcqi * Qm:(Qcqi + G) * Qm], c["maxit"],
                                                       state.get(c["harq_after"]))
        state[c["name"]] = st
        assert int(oret == 0) == int(fx.get(c, "crc")), c["name"]
        assert oavg == float(fx.get(c, "res")[0]), (c["name"], oavg)
        if oret == 0:
            assert np.array_equal(odata[:c["tbs"] // 8], fx.get(c, "payload")), c["name"]
        assert C.uci_fields(c, got) == list(fx.get(c, "uci")), c["name"]
        if c["sent"]:
            assert np.array_equal(fx.get(c, "payload"), fx.get(c, "tx_payload"))
        if c["harq_after"]:  # and without the first transmission's state it fails, as the reference does
            aret, _, _, aavg, _ = po.ora.dlsch_decode(c["tbs"], Qm, c["rv"], g[Qcqi * Qm:(Qcqi + G) * Qm], c["maxit"], None)
            assert (int(aret == 0), aavg) == tuple(fx.get(c, "alone")) and aret != 0 and oret == 0
