"""PUSCH transmit, host side, no GPU: the layouts of the structures include/srsran_ue_ul.h adds against the
reference's headers and against the ctypes mirrors, a C99 translation unit that includes the header and links
every new entry point, and the case table of tests/pusch_tx_cases.py held to what each case claims to exercise
(through the model: the reference's uci.c encoder in oracle/_ref), and the fixture recorded from the compiled reference
transmitter: its MEASURED copy against the cases file, a float64 restatement of the constellation, the transform
precoder, the mapper and the DMRS on its own bits, and the numpy transmitter (tests/pusch_tx.py's chain, tx_model) on
every case -- bits equal, grids within the measured distances -- so that fixture and tolerances are proven on the
CPU before any GPU run."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import pusch as OP  # noqa: E402  (oracle/pusch.py)
import pusch_tx_cases as TC  # noqa: E402
from srsran_4g_amd import sch as S  # noqa: E402
from srsran_4g_amd import tdec  # noqa: E402
from srsran_4g_amd import ue_ul as UL  # noqa: E402

INCLUDE = os.path.join(ROOT, "include")
REF_INCLUDE = "/root/reference/lib/include"
needs_ref = pytest.mark.skipif(not OP.ref_available(), reason="oracle/_ref not built")

TYPES = ["srsran_ue_ul_cfg_t", "srsran_ul_cfg_t", "srsran_refsignal_srs_cfg_t", "srsran_pusch_hopping_cfg_t",
         "srsran_ue_ul_powerctrl_t", "srsran_pusch_data_t"]
OFFSETS = [("srsran_ue_ul_cfg_t", "grant_available"), ("srsran_ue_ul_cfg_t", "cc_idx"),
           ("srsran_ue_ul_cfg_t", "normalize_mode"), ("srsran_ue_ul_cfg_t", "force_peak_amplitude"),
           ("srsran_ue_ul_cfg_t", "cfo_en"), ("srsran_ue_ul_cfg_t", "cfo_tol"), ("srsran_ue_ul_cfg_t", "cfo_value"),
           ("srsran_ul_cfg_t", "pusch"), ("srsran_ul_cfg_t", "hopping"), ("srsran_ul_cfg_t", "power_ctrl"),
           ("srsran_ul_cfg_t", "dmrs"), ("srsran_ul_cfg_t", "srs"), ("srsran_refsignal_srs_cfg_t", "configured"),
           ("srsran_pusch_hopping_cfg_t", "hopping_enabled"), ("srsran_ue_ul_powerctrl_t", "p_srs_offset"),
           ("srsran_pusch_data_t", "uci")]
PROBE = "#include <stddef.h>\n#include <stdio.h>\n%s\nint main(void) {\n%s\n  return 0;\n}\n"
SYMBOLS = ["srsran_ulsch_encode", "srsran_pusch_init_ue", "srsran_pusch_encode", "srsran_refsignal_dmrs_pusch_put_cell",
           "srsran_ue_ul_init", "srsran_ue_ul_free", "srsran_ue_ul_set_cell", "srsran_ue_ul_set_cfr",
           "srsran_ue_ul_pregen_signals", "srsran_ue_ul_encode", "srsran_ue_ul_gpu_tx_batch", "srsran_ue_ul_gpu_last"]


def _probe(includes, flags, extra="", libs=()):
    body = "\n".join(['  printf("%%zu\\n", sizeof(%s));' % t for t in TYPES] +
                     ['  printf("%%zu\\n", offsetof(%s, %s));' % o for o in OFFSETS]) + extra
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(PROBE % (includes, body))
        r = subprocess.run(["gcc", "-Wall", "-Werror", "-Wno-unused-variable"] + flags + [src, "-o", exe] + list(libs),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()


def _ctypes_layout():
    return [ctypes.sizeof(getattr(UL, t)) for t in TYPES] + [getattr(getattr(UL, t), f).offset for t, f in OFFSETS]


def test_header_compiles_as_c99_links_and_matches_ctypes():
    """a C99 translation unit that includes srsran_ue_ul.h, takes the address of every new entry point and links"""
    libdir = os.path.dirname(tdec.LIB_PATH)
    refs = "\n  void* syms[] = {%s};\n  printf(\"%%zu\\n\", sizeof(syms) / sizeof(syms[0]));" % ", ".join(
        "(void*)%s" % s for s in SYMBOLS)
    out = _probe('#include "srsran_ue_ul.h"', ["-std=c99", "-I", INCLUDE], refs,
                 ["-L", libdir, "-lsrsran_4g_amd", "-Wl,-rpath," + libdir, "-lm"])
    assert [int(v) for v in out[:-1]] == _ctypes_layout() and int(out[-1]) == len(SYMBOLS)


@pytest.mark.skipif(not os.path.isdir(REF_INCLUDE), reason="the reference headers are not on this machine")
def test_struct_layouts_match_reference_headers():
    inc = "\n".join('#include "srsran/phy/%s"' % h for h in ("ch_estimation/chest_ul.h", "phch/pucch.h", "phch/ra_ul.h",
                                                              "ue/ue_ul.h"))
    assert [int(v) for v in _probe(inc, ["-std=gnu99", "-I", REF_INCLUDE])] == _ctypes_layout()


def test_case_table_is_well_formed():
    names = [c["name"] for c in TC.CASES]
    assert len(set(names)) == len(names) and names[:3] == ["t1", "t2", "t3"]
    for c in TC.CASES:
        assert c["n_tilde"][0] + c["L"] <= c["nof_prb"] and c["n_tilde"][1] + c["L"] <= c["nof_prb"]
        cfg = TC.make(c)[3]
        assert cfg.grant.tb.nof_bits == cfg.grant.nof_re * c["Qm"] and cfg.grant.tb.tbs % 8 == 0


@needs_ref
def test_cases_exercise_what_they_claim():
    po = OP.PuschOracle()
    m = {}
    for c in TC.CASES:
        cell, d, sf, cfg = TC.make(c)
        if not c["enable_64qam"]:
            cfg.grant.tb.mod, cfg.grant.tb.nof_bits = S.MOD_FROM_QM[4], cfg.grant.nof_re * 4
        payload, u = TC.payload_uci(c, cfg)
        m[c["name"]] = (TC.tx_model(po, c, cfg, payload, u), cfg)
        mm = m[c["name"]][0]
        assert mm["q"].size == cfg.grant.tb.nof_bits and mm["d"].size == cfg.grant.nof_re
        data, dm = TC.grant_mask(c, mm)
        assert np.all(mm["grid"][~data] == 0) and data.sum() == cfg.grant.nof_re and dm.sum() == 2 * mm["M"]
    RU = __import__("uci")
    t2, t3, t4, t6, t7, t9 = (m[n][0] for n in ("t2", "t3", "t4", "t6", "t7", "t9"))
    assert (t2["types"] == RU.TYPE_REPETITION).sum() == t2["Qack"] and (t2["types"] == RU.TYPE_PLACEHOLDER).sum() > 0
    assert t3["Qri"] > 0 and t3["Qack"] > 0 and m["t3"][1].grant.nof_symb == 10
    assert (t4["Qcqi"] * t4["Qm"]) % 8 != 0 and m["t4"][1].grant.nof_symb == 11
    assert t6["Qri"] > 0 and t6["Qack"] > 0 and t6["Qcqi"] > 0
    assert S.lib().srsran_cqi_size(ctypes.byref(m["t6"][1].uci_cfg.cqi)) > 11
    assert m["t7"][1].grant.tb.tbs == 0 and t7["G"] == 0 and t7["Qcqi"] > 0 and t7["Qack"] > 0
    assert m["t8"][1].grant.tb.mod == S.MOD_FROM_QM[4]
    seg = m["t9"][1].grant.tb.tbs + 24
    assert seg > 6144 and t9["G"] % 2 == 1 and t9["Qack"] > 0  # two code blocks whose E differ
    assert m["t10"][0]["M"] == 1200
    assert not np.array_equal(m["t11a"][0]["s"], m["t11b"][0]["s"])
    assert TC.BY_NAME["t5"]["n_tilde"][0] != TC.BY_NAME["t5"]["n_tilde"][1] != TC.BY_NAME["t5"]["n_prb"]


# ---------------------------------------------------------------- the fixture of the compiled reference transmitter
IDS = [c["name"] for c in TC.CASES]


@pytest.fixture(scope="module")
def fx():
    return TC.Fixture()


def test_fixture_measured_copy_and_size(fx):
    import chest_cases
    assert fx.measured == TC.MEASURED
    assert TC.D_TOL == max(4 * TC.MEASURED["d"], 1e-6) and TC.GRID_TOL == 4 * TC.MEASURED["grid"]
    assert os.path.getsize(os.path.join(HERE, "golden", TC.FIXTURE)) <= chest_cases.MAX_FIXTURE_BYTES
    for c in TC.CASES:
        assert fx.has(c, "d") == (c["L"] <= 6)


@pytest.mark.parametrize("c", TC.CASES, ids=IDS)
def test_float64_restatement_matches_fixture(fx, c):
    """constellation, DFT / sqrt(M), mapper and exact DMRS in float64 on the fixture's own scrambled bits"""
    import pusch_cases as PC
    from synth.synth import modulate
    ret, K_segm, mod, nof_bits = (int(v) for v in fx.get(c, "out"))
    cfg = TC.make(c)[3]
    Qm = {1: 2, 2: 4, 3: 6}[mod]
    want_mod = S.MOD_FROM_QM[4] if not c["enable_64qam"] and c["Qm"] == 6 else cfg.grant.tb.mod
    assert (mod, nof_bits) == (want_mod, cfg.grant.nof_re * Qm)  # the write-back
    s = np.unpackbits(fx.get(c, "s"))
    assert s.size == nof_bits and fx.get(c, "q").size == nof_bits // 8 == fx.get(c, "g").size
    d64 = np.asarray(modulate(s, Qm), np.complex128)
    if fx.has(c, "d"):
        assert np.abs(fx.get(c, "d") - d64).max() / np.abs(d64).max() <= TC.MEASURED["d"]
    M, ns, rows = 12 * c["L"], PC.nsymb_slot(c["cp"]), TC.data_rows(c)
    grid = fx.grid(c)
    data, dm = TC.grant_mask(c, dict(nsym=ns, M=M, rows=rows))
    want = np.zeros(grid.shape, np.complex128)
    for i, row in enumerate(rows):
        n0 = c["n_tilde"][row // ns] * 12
        want[row, n0:n0 + M] = np.fft.fft(d64[i * M:(i + 1) * M]) / np.sqrt(M)
    assert PC.err("rms", grid[data], want[data]) <= TC.MEASURED["grid"]
    assert not np.any(grid[~(data | dm)])
    if c["shortened"]:
        assert not np.any(grid[-1])  # the last symbol of a shortened subframe stays untouched
    exact, bound = PC.dmrs_exact(dict(c, dmrs=[int(v) for v in c["dmrs"]]))
    got = np.concatenate([grid[(sl + 1) * ns - 4, c["n_tilde"][sl] * 12:c["n_tilde"][sl] * 12 + M] for sl in (0, 1)])
    assert np.array_equal(got, fx.get(c, "dmrs")) and PC.err("abs", got, exact) <= bound
    # scrambling: outside the placeholder / repetition positions the scrambled bits are q xor the Gold sequence
    seq = PC.gold(((c["rnti"] << 14) + ((c["tti"] % 10) << 9) + c["cell_id"]), nof_bits)
    diff = np.unpackbits(fx.get(c, "q")) ^ seq ^ s
    assert diff.sum() <= ret and (ret > 0 or not diff.any())


@needs_ref
@pytest.mark.parametrize("c", TC.CASES, ids=IDS)
def test_numpy_transmitter_matches_fixture(fx, c):
    """tx_model (the numpy transmitter around the reference's uci.c and the oracle's UL-SCH encoder) against what the
    compiled sch.c / pusch.c gave: return, K_segm, q, scrambled bits and the TB's part of g equal, grid within MEASURED"""
    import pusch_cases as PC
    po = OP.PuschOracle()
    cfg = TC.make(c)[3]
    if not c["enable_64qam"]:
        cfg.grant.tb.mod, cfg.grant.tb.nof_bits = S.MOD_FROM_QM[4], cfg.grant.nof_re * 4
    payload, u = TC.payload_uci(c, cfg)
    assert np.array_equal(payload, fx.get(c, "payload")) and bytes(u) == fx.get(c, "uci").tobytes()
    m = TC.tx_model(po, c, cfg, payload, u)
    ret, K_segm, mod, nof_bits = (int(v) for v in fx.get(c, "out"))
    assert (ret, K_segm) == (m["ret"], cfg.K_segm)
    assert np.array_equal(np.unpackbits(fx.get(c, "q")), m["q"]) and np.array_equal(np.unpackbits(fx.get(c, "s")), m["s"])
    o = m["Qcqi"] * m["Qm"]
    assert np.array_equal(np.unpackbits(fx.get(c, "g"))[o:o + m["e"].size], m["e"])
    data, dm = TC.grant_mask(c, m)
    grid = fx.grid(c)
    assert PC.err("rms", grid[data], m["grid"][data]) <= TC.MEASURED["grid"]
    bound = PC.dmrs_exact(dict(c, dmrs=[int(v) for v in c["dmrs"]]))[1]
    assert PC.err("abs", fx.get(c, "dmrs"), m["dmrs"]) <= 2 * bound
