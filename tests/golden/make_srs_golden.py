"""Generate tests/golden/srs_golden.npz from the reference's own sounding reference signal and its estimator.

Run where the reference tree exists (REF as in oracle/Makefile):
    python tests/golden/make_srs_golden.py [REF]
The build is tests/golden/make_pusch_golden.py's (its source list, stubs, DFT stand-in and temporary directory that is
removed afterwards), with the harness functions below added (our own code: they only call the reference's functions
srsran_refsignal_srs_M_sc / _srs_gen / _srs_put, srsran_refsignal_srs_pusch_shortened and
srsran_chest_ul_estimate_srs, and read fields of its structs).  Two builds: the flags of oracle/Makefile, and
-O1 -ffp-contract=off with SSE only.  The fixture stores build 1.

Per case of tests/srs_cases.py: CASES and per tti: srs_gen + srs_put on a grid full of a sentinel (the last symbol's
row is stored with the sentinel replaced by zero), and srs_put of the values 1, 2, .. M_sc on a zeroed grid, which
shows k0 (the static srs_k0_ue) as the position of the value 1.  Per case of EST_CASES: build 1's SRS row times a
3-tap channel and a delay ramp plus AWGN (numpy, rounded to float), then srsran_chest_ul_estimate_srs of both builds
on an identity-prefilled result: the ten scalars and the M_sc estimates at symbol L(0, cp).  SHORT_CASES: the
answers of srsran_refsignal_srs_pusch_shortened.

MEASURED, printed and stored (tests/srs_cases.py holds a copy): seq -- the largest distance of either build's SRS
values from a float64 evaluation at the reference's rounded-to-float arguments (srs_cases.srs_rounded); per estimator
case -- the largest relative distance of either build's estimator (the eight float scalars, and the estimates relative
to the largest one) from tests/srs_np.py on the same input with the build's own sequence.

No file is written unless
  (a) both builds agree in every integer (k0, M_sc, the shortened answers) and in ta_us;
  (b) every SRS row lies within srs_cases.srs_exact's bound (1.5 ulp32 at the case's largest argument plus 2^-22) of
      the exact sequence;
  (c) every float64 unrounded ta_us lies at least 0.02 us from a rounding boundary of the 0.1 us grid;
  (d) no RE outside the comb of the last symbol is written, by srs_put or (outside the M_sc estimates) by the estimator;
  (e) the file stays within chest_cases.MAX_FIXTURE_BYTES.
"""
import ctypes
import json
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_pusch_golden as MG  # noqa: E402
import srs_cases as SC  # noqa: E402
import srs_np  # noqa: E402
from srsran_4g_amd import sch as S  # noqa: E402
from srsran_4g_amd import ue_ul as UL  # noqa: E402

SENTINEL = np.complex64(7 + 5j)

HARNESS_SRS = r'''
int ph_srs_sizeof(void) { return (int)sizeof(srsran_refsignal_srs_cfg_t); }

/* r: 2 M_sc values; grid: the caller's prefill, the SRS put into it */
int ph_srs_tx(ph_t* q, srsran_refsignal_srs_cfg_t* cfg, uint32_t tti, cf_t* r, cf_t* grid, uint32_t* m_sc)
{
  *m_sc = srsran_refsignal_srs_M_sc(&q->sig, cfg);
  if (srsran_refsignal_srs_gen(&q->sig, cfg, &q->dmrs, tti % 10, r)) {
    return -1;
  }
  return srsran_refsignal_srs_put(&q->sig, cfg, tti, r, grid);
}

int ph_srs_put(ph_t* q, srsran_refsignal_srs_cfg_t* cfg, uint32_t tti, cf_t* r, cf_t* grid)
{
  return srsran_refsignal_srs_put(&q->sig, cfg, tti, r, grid);
}

int ph_srs_short(ph_t* q, srsran_refsignal_srs_cfg_t* cfg, uint32_t tti, srsran_pusch_cfg_t* pc, int before)
{
  srsran_ul_sf_cfg_t sf = sf_cfg(tti, before);
  srsran_refsignal_srs_pusch_shortened(&q->sig, &sf, cfg, pc);
  return sf.shortened ? 1 : 0;
}

/* the estimator on an identity-prefilled result; scal: the ten scalars of srsran_chest_ul_res_t in the struct's order */
int ph_srs_est(ph_t* q, srsran_refsignal_srs_cfg_t* cfg, uint32_t tti, uint32_t smooth_filter_len, cf_t* grid, cf_t* ce, float* scal)
{
  srsran_ul_sf_cfg_t sf = sf_cfg(tti, 0);
  q->chest.smooth_filter_len = smooth_filter_len;
  srsran_chest_ul_res_set_identity(&q->cres);
  int rc = srsran_chest_ul_estimate_srs(&q->chest, &sf, cfg, &q->dmrs, grid, &q->cres);
  memcpy(ce, q->cres.ce, q->nre * sizeof(cf_t));
  const srsran_chest_ul_res_t* e = &q->cres;
  scal[0] = e->noise_estimate, scal[1] = e->noise_estimate_dbFs, scal[2] = e->rsrp, scal[3] = e->rsrp_dBfs, scal[4] = e->epre;
  scal[5] = e->epre_dBfs, scal[6] = e->snr, scal[7] = e->snr_db, scal[8] = e->cfo_hz, scal[9] = e->ta_us;
  return rc;
}
'''

# srsran_refsignal_srs_pusch_shortened: (case, tti, n_prb_tilde, L_prb, is_rar); the 15 PRB cell's SRS region is PRB 1..12
# with bw_cfg 5 (m_SRS,0 = 12, start 7 - 6)
SHORT_CASES = [
    ("p15_seqhop", 5, (3, 3), 4, 0),    # the UE's own SRS subframe, overlapping
    ("p15_seqhop", 5, (13, 13), 2, 0),  # contiguous on the right: not shortened by the first rule, nor the second
    ("p15_seqhop", 5, (0, 0), 1, 0),    # contiguous on the left
    ("p15_seqhop", 5, (14, 14), 1, 0),  # disjoint, the UE's own SRS subframe: shortened
    ("p15_seqhop", 5, (3, 3), 4, 1),    # a RAR grant: never
    ("p15_seqhop", 10, (3, 3), 4, 0),   # a cell SRS subframe that is not the UE's, overlapping
    ("p15_seqhop", 10, (14, 14), 1, 0),  # ... disjoint
    ("p15_seqhop", 10, (0, 0), 15, 0),  # ... covering the region
    ("p15_seqhop", 10, (0, 0), 2, 0),   # ... reaching into it from the left
    ("p15_seqhop", 6, (3, 3), 4, 0),    # not an SRS subframe of the cell
    ("p15_seqhop", 5, (13, 3), 2, 0),   # contiguous in one slot only
]


def build(ref, d, scalar):
    if "ph_srs_tx" not in MG.HARNESS:
        MG.HARNESS = MG.HARNESS + HARNESS_SRS
    L = MG.build_reference(ref, d, scalar)
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.ph_srs_tx.argtypes = [vp, vp, u32, vp, vp, vp]
    L.ph_srs_put.argtypes = [vp, vp, u32, vp, vp]
    L.ph_srs_short.argtypes = [vp, vp, u32, vp, ci]
    L.ph_srs_est.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    assert L.ph_srs_sizeof() == ctypes.sizeof(UL.srsran_refsignal_srs_cfg_t)
    return L


def obj_of(L, objs, c):
    if c["name"] not in objs:
        dm = np.array(c["dmrs"], np.uint32)
        objs[c["name"]] = ctypes.c_void_p(L.ph_new(c["nof_prb"], c["cell_id"], c["cp"], MG.ptr(dm)))
        assert objs[c["name"]], c["name"]
    return objs[c["name"]]


def transmit(L, objs, c, tti, problems):
    """-> (k0, M_sc, r (2 M_sc), last row with zeros off the comb)"""
    q, cfg = obj_of(L, objs, c), SC.srs_cfg(c)
    nsym, nre = 2 * SC.nsymb_slot(c["cp"]), 12 * c["nof_prb"]
    m_sc = ctypes.c_uint32()
    r = np.zeros(2 * 600, np.complex64)
    grid = np.full(nsym * nre, SENTINEL, np.complex64)
    assert L.ph_srs_tx(q, ctypes.byref(cfg), tti, MG.ptr(r), MG.ptr(grid), ctypes.byref(m_sc)) == 0
    M = int(m_sc.value)
    idx = np.zeros(nsym * nre, np.complex64)
    ramp = np.arange(1, M + 1).astype(np.complex64)
    assert L.ph_srs_put(q, ctypes.byref(cfg), tti, MG.ptr(ramp), MG.ptr(idx)) == 0
    k0 = int(np.flatnonzero(idx == 1)[0]) - (nsym - 1) * nre
    on = np.zeros(nsym * nre, bool)
    on[(nsym - 1) * nre + k0 + 2 * np.arange(M)] = True
    if k0 < 0 or not np.array_equal(idx[on], ramp) or np.any(idx[~on] != 0):
        problems.append((c["name"], tti, "srs_put does not write the comb from k0"))
    if np.any(grid[~on] != SENTINEL) or np.any(grid[on] == SENTINEL):
        problems.append((c["name"], tti, "an RE outside the comb is written"))
    if not np.array_equal(grid[on], r[:M]):
        problems.append((c["name"], tti, "the comb does not hold the first of the two slot sequences"))
    row = np.where(on, grid, 0).astype(np.complex64)[(nsym - 1) * nre:]
    return k0, M, r[:2 * M].copy(), row


def channel(c, e, rng):
    """3 taps, a delay ramp of ta_us (a pure delay: the phase falls with the subcarrier): (cell subcarriers)"""
    k = np.arange(12 * c["nof_prb"])
    taps = np.array([1.0, 0.3 * np.exp(2j * np.pi * rng.random()), 0.12 * np.exp(2j * np.pi * rng.random())])
    taps = taps / np.sqrt((np.abs(taps) ** 2).sum()) * np.exp(2j * np.pi * rng.random())
    H = (taps[None, :] * np.exp(-2j * np.pi * np.outer(k, np.arange(3)) / 2048.0)).sum(axis=1)
    return H * np.exp(-2j * np.pi * 15e3 * k * e["ta_us"] * 1e-6)


def received(c, e, row):
    rng = np.random.default_rng(7000 + e["seed"])
    y = row.astype(np.complex128) * channel(c, e, rng)
    if e["snr_db"] is not None:
        sigma = np.sqrt(10 ** (-e["snr_db"] / 10) / 2)
        y = y + sigma * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))
    return y.astype(np.complex64)


def main(write=True):
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF")
    if not ref:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        ref = re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    if not os.path.exists(os.path.join(ref, "src/phy/ch_estimation/refsignal_ul.c")):
        sys.exit(f"reference tree not found at {ref}")
    out, problems = {}, []
    measured = dict(seq=0.0)
    measured.update({e["name"]: 0.0 for e in SC.EST_CASES})
    floats = [k for k in SC.SCALARS if k not in ("cfo_hz", "ta_us")]
    with tempfile.TemporaryDirectory() as tmp:
        Ls = [build(ref, os.path.join(tmp, "b1"), False), build(ref, os.path.join(tmp, "b2"), True)]
        objs = [{}, {}]
        seqs = {}
        for c in SC.CASES:
            k0s, rows = [], []
            for tti in c["ttis"]:
                o = [transmit(L, ob, c, tti, problems) for L, ob in zip(Ls, objs)]
                if o[0][:2] != o[1][:2]:
                    problems.append((c["name"], tti, "k0 / M_sc differ between the builds", o[0][:2], o[1][:2]))
                rex, bound, _ = SC.srs_exact(c, tti)
                r64 = SC.srs_rounded(c, tti)
                for k in (0, 1):
                    M = o[k][1]
                    d = float(np.abs(o[k][2][:M] - rex).max())
                    if d > bound:
                        problems.append((c["name"], tti, "SRS further from the exact one than the float formats explain", k, d, bound))
                    measured["seq"] = max(measured["seq"], float(np.abs(o[k][2][:M] - r64).max()))
                k0s.append(o[0][0])
                rows.append(o[0][3])
                seqs[(c["name"], tti)] = [o[0][2], o[1][2]]
            out["k0." + c["name"]] = np.array(k0s, np.int32)
            out["msc." + c["name"]] = np.int32(o[0][1])
            out["row." + c["name"]] = np.stack(rows)
        for e in SC.EST_CASES:
            c = SC.BY_NAME[e["of"]]
            tti, i = c["ttis"][0], 0
            nsym, nre = 2 * SC.nsymb_slot(c["cp"]), 12 * c["nof_prb"]
            k0, M = int(out["k0." + c["name"]][i]), int(out["msc." + c["name"]])
            y = received(c, e, out["row." + c["name"]][i])
            grid = np.zeros(nsym * nre, np.complex64)
            grid[(nsym - 1) * nre:] = y
            L0 = (3 if c["cp"] == 0 else 2) * nre
            got = []
            for k, (L, ob) in enumerate(zip(Ls, objs)):
                cfg = SC.srs_cfg(c)
                ce, scal = np.zeros(grid.size, np.complex64), np.zeros(10, np.float32)
                assert L.ph_srs_est(obj_of(L, ob, c), ctypes.byref(cfg), tti, e["smooth"], MG.ptr(grid), MG.ptr(ce), MG.ptr(scal)) == 0
                rest = np.ones(grid.size, bool)
                rest[L0:L0 + M] = False
                if np.any(ce[rest] != 1):
                    problems.append((e["name"], "the estimator writes outside the M_sc estimates", k))
                m = srs_np.estimate(srs_np.comb(y, k0, M), seqs[(c["name"], tti)][k][:M], e["smooth"])
                sc = dict(zip(SC.SCALARS, scal))
                if not np.isnan(sc["cfo_hz"]):
                    problems.append((e["name"], "cfo_hz is not NaN", k))
                if sc["ta_us"] != np.float32(m["ta_us"]):
                    problems.append((e["name"], "ta_us differs from the float64 model", k, sc["ta_us"], m["ta_us"]))
                frac = abs(m["ta_raw"]) * 10 % 1
                if abs(frac - 0.5) < 0.2:
                    problems.append((e["name"], "ta_us within 0.02 us of a rounding boundary", m["ta_raw"]))
                for key in floats:
                    want = m[key]
                    if np.isnan(want) or np.isinf(want) or (want == 0 and sc[key] == 0):
                        if not (np.isnan(want) and np.isnan(sc[key]) or want == sc[key]):
                            problems.append((e["name"], key, "special value differs", k, sc[key], want))
                        continue
                    measured[e["name"]] = max(measured[e["name"]], abs(float(sc[key]) - want) / abs(want))
                measured[e["name"]] = max(measured[e["name"]], float(np.abs(ce[L0:L0 + M] - m["ce"]).max() / np.abs(m["ce"]).max()))
                got.append((scal, ce[L0:L0 + M].copy(), m))
            if got[0][0][9] != got[1][0][9]:
                problems.append((e["name"], "ta_us differs between the builds", got[0][0][9], got[1][0][9]))
            out["rx." + e["name"]] = y
            out["scal." + e["name"]] = got[0][0]
            out["ce." + e["name"]] = got[0][1]
            print("%-14s ta_us %.1f (applied %.2f, unrounded %.4f)  noise %.3e  snr_db %.2f" %
                  (e["name"], got[0][0][9], e["ta_us"], got[0][2]["ta_raw"], got[0][0][0], got[0][0][7]))
        short = []
        for name, tti, nt, Lp, rar in SHORT_CASES:
            c = SC.BY_NAME[name]
            ans = []
            for L, ob in zip(Ls, objs):
                pc = S.srsran_pusch_cfg_t()
                pc.grant.n_prb_tilde[0], pc.grant.n_prb_tilde[1], pc.grant.L_prb, pc.grant.is_rar = nt[0], nt[1], Lp, bool(rar)
                cfg = SC.srs_cfg(c)
                ans.append([L.ph_srs_short(obj_of(L, ob, c), ctypes.byref(cfg), tti, ctypes.byref(pc), b) for b in (0, 1)])
            if ans[0] != ans[1] or ans[0][0] != ans[0][1]:
                problems.append((name, tti, "shortened differs between the builds or depends on its previous value", ans))
            short.append(ans[0][0])
        out["short"] = np.array(short, np.int32)
        for L, ob in zip(Ls, objs):
            for q in ob.values():
                L.ph_free(q)
    for key, v in measured.items():  # four significant digits, rounded up: never below what was measured
        if v > 0:
            step = 10.0 ** (np.floor(np.log10(v)) - 3)
            measured[key] = float("%.3e" % (np.ceil(v / step) * step))
    print("MEASURED = dict(")
    for key, v in measured.items():
        print("    %s=%.3e," % (key, v))
    print(")")
    out["measured"] = np.frombuffer(json.dumps({k: float("%.3e" % v) for k, v in measured.items()}).encode(), np.uint8)
    if problems:
        for p in problems:
            print("PROBLEM", p)
        sys.exit("nothing written")
    if write:
        path = os.path.join(HERE, SC.FIXTURE)
        MG.write_npz(path, out)
        size = os.path.getsize(path)
        assert size <= MG.MAX_BYTES, size
        print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
