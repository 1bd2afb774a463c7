"""PUCCH receive on the GPU against the reference, golden by golden (tests/golden/pucch_golden.npz: every format,
both CPs, shortened subframes, delta_pucch_shift 1..3, mixed PRB, group hopping, 25 PRB, multiplexed UEs, channel
selection, SR + ACK, CQI drop, DMRS detection, timing advance, 3 dB, noise only).  No case is skipped.

Bounds: ce within 2e-5 x max|ce| (the bound the project's estimators are held to); the estimator scalars and the
correlations within 4 x the largest distance the reference's own float result has from a float64 evaluation of the
same formulas on the same grids (recorded in the fixture, "allow"; at least 1e-5 for the correlation); ta_us equal
after the rounding to 0.1 us (the recorded float64 values lie 0.13 of a step from the nearest rounding boundary);
every decision and decoded field equal."""
import ctypes

import numpy as np
import pytest

import pucch_cases as C
import pucch_rx as R
from srsran_4g_amd import pucch as P
from srsran_4g_amd import tdec

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not tdec.gpu_available(), reason="needs a HIP device")]


@pytest.fixture(scope="module")
def G():
    return C.Golden.get()


@pytest.fixture(scope="module")
def rig():
    r = R.Rig()
    yield r
    r.free()


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def db_tol(allow_rel, v):
    """a power within (1 +- 4 allow) of the exact one, in dB, plus the float32 rounding of the logarithm"""
    return 10 * np.log10(1 + 4 * allow_rel) + 4e-6 * max(1.0, abs(float(v)))


def early_out(spec, ref_f, ref_i):
    """the reference's DMRS detection returned before decoding"""
    return C.full(spec)["thr_dmrs"] > 0 and ref_f[0] == 0.0 and ref_i[0] == 0


def test_estimator_and_direct_decode(G, rig):
    """srsran_chest_ul_estimate_pucch + srsran_pucch_decode with the true format / resource, every case"""
    A = G.allow
    bad, worst = [], dict(ce=0.0, epre=0.0, rsrp=0.0, noise=0.0, snr=0.0, corr=0.0, dmrs_corr=0.0)
    for i, spec in enumerate(G.cases):
        s = C.full(spec)
        _, chest, pucch = rig.get(s)
        cfg, sf, grid = R.direct_cfg(G, i), C.build_sf(s), G.grid(i)
        nsym2 = grid.shape[0]
        assert P.estimate(chest, sf, cfg, grid) == 0, spec["name"]
        ce = chest.ce(grid.size).reshape(grid.shape)
        want_ce = G.z[f"d_ce_{i}"]
        lib = P.lib()
        cell = rig.get(s)[0]
        prb = [lib.srsran_pucch_n_prb(ctypes.byref(cell), ctypes.byref(cfg), sl) for sl in range(2)]
        got_ce = np.stack([ce[sl * nsym2 // 2:(sl + 1) * nsym2 // 2, 12 * prb[sl]:12 * prb[sl] + 12] for sl in range(2)])
        e = np.abs(got_ce - want_ce).max() / np.abs(want_ce).max()
        worst["ce"] = max(worst["ce"], e)
        if not e <= 2e-5:
            bad.append((spec["name"], "ce", e))
        sc, f64 = G.z[f"d_scal_{i}"], G.z[f"d_f64_{i}"]
        r = chest.res
        for k, j, got in (("epre", 0, r.epre), ("rsrp", 1, r.rsrp), ("noise", 2, r.noise_estimate), ("snr", 3, r.snr)):
            d = rel(got, f64[j])
            worst[k] = max(worst[k], d)
            if not d <= 4 * A["rel_" + k]:
                bad.append((spec["name"], k, got, f64[j], d))
        for k, j, got in (("epre", 5, r.epre_dBfs), ("rsrp", 6, r.rsrp_dBfs), ("noise", 7, r.noise_estimate_dbFs),
                          ("snr", 8, r.snr_db)):
            if not abs(got - sc[j]) <= db_tol(A["rel_" + k], sc[j]):
                bad.append((spec["name"], k + "_dB", got, sc[j]))
        if s["meas_ta"] and r.ta_us != sc[4]:
            bad.append((spec["name"], "ta_us", r.ta_us, sc[4]))
        ret, res = pucch.decode(sf, cfg, chest.res, grid)
        assert ret == 0, spec["name"]
        gi, gf = C.res_arrays(res)
        ri, rf = G.z[f"d_res_i_{i}"], G.z[f"d_res_f_{i}"]
        if early_out(spec, rf, ri):
            if gf[0] != 0.0 or gi[0] != 0:
                bad.append((spec["name"], "DMRS detection", gf[0], gi[0]))
        else:
            d = abs(gf[0] - f64[5])
            worst["corr"] = max(worst["corr"], d)
            if not d <= max(4 * A["abs_corr"], 1e-5):
                bad.append((spec["name"], "correlation", gf[0], f64[5]))
        if s["thr_dmrs"] > 0:
            d = abs(gf[1] - f64[6])
            worst["dmrs_corr"] = max(worst["dmrs_corr"], d)
            if not d <= 4 * A["abs_dmrs_corr"]:
                bad.append((spec["name"], "dmrs_correlation", gf[1], f64[6]))
        nint = len(gi) if spec["tx"] is not None else 2  # noise only: the bits are ties of noise
        if not np.array_equal(gi[:nint], ri[:nint]):
            bad.append((spec["name"], "decoded fields", list(gi), list(ri)))
        if spec["tx"] is not None and not np.array_equal(C.cfg_arrays(cfg), G.z[f"d_cfg_{i}"]):
            bad.append((spec["name"], "cfg write-backs", list(C.cfg_arrays(cfg)), list(G.z[f"d_cfg_{i}"])))
    print("largest distances:", {k: float(v) for k, v in worst.items()}, "allowed x4 of", A)
    assert not bad, bad[:10]


def test_get_pucch_one_entry(G, rig):
    """the one-entry batch call against the reference's srsran_enb_ul_get_pucch sequence, every case"""
    A = G.allow
    bad = []
    tol_c = max(5 * A["abs_corr"], 1e-5)
    for i, spec in enumerate(G.cases):
        ret, res, cfg = R.get_one(rig, spec, G.grid(i))
        assert ret == 0, spec["name"]
        gi, gf = C.res_arrays(res)
        ri, rf = G.z[f"g_res_i_{i}"], G.z[f"g_res_f_{i}"]
        if not abs(gf[0] - rf[0]) <= tol_c:
            bad.append((spec["name"], "correlation", gf[0], rf[0]))
        if spec["tx"] is None:
            if not np.array_equal(gi[:2], ri[:2]):
                bad.append((spec["name"], "detected / ack.valid", list(gi[:2]), list(ri[:2])))
            continue
        if not np.array_equal(gi, ri):
            bad.append((spec["name"], "decoded fields", list(gi), list(ri)))
        if not np.array_equal(C.cfg_arrays(cfg), G.z[f"g_cfg_{i}"]):
            bad.append((spec["name"], "cfg write-backs", list(C.cfg_arrays(cfg)), list(G.z[f"g_cfg_{i}"])))
        # the chosen resource: the result carries the picked candidate's correlation (the others lie far from it)
        cand, chosen = G.z[f"g_cand_{i}"], G.z[f"g_chosen_{i}"]
        picked = [c for c in cand if c[3] == 1 and c[2] == chosen[1]]
        if not picked or not abs(gf[0] - picked[-1][0]) <= tol_c:
            bad.append((spec["name"], "chosen resource", gf[0], cand.tolist()))
        if C.full(spec)["thr_dmrs"] > 0 and not abs(gf[1] - rf[1]) <= 5 * A["abs_dmrs_corr"]:
            bad.append((spec["name"], "dmrs_correlation", gf[1], rf[1]))
        for k, j in (("snr", 2), ("epre", 3), ("noise", 4)):
            if not abs(gf[j] - rf[j]) <= db_tol(A["rel_" + k], rf[j]) + 10 * np.log10(1 + A["rel_" + k]):
                bad.append((spec["name"], C.RES_FLOATS[j], gf[j], rf[j]))
        if gf[5] != rf[5]:
            bad.append((spec["name"], "ta_us", gf[5], rf[5]))
    assert not bad, bad[:10]


def test_cedron_is_refused(G, rig):
    spec = G.cases[0]
    s = C.full(spec)
    _, chest, _ = rig.get(s)
    cfg = R.direct_cfg(G, 0)
    cfg.meas_ta_en = cfg.use_cedron_alg = True
    assert P.estimate(chest, C.build_sf(s), cfg, G.grid(0)) == -1
    cfg = R.get_cfg(spec)
    cfg.meas_ta_en = cfg.use_cedron_alg = True
    t, dptr = R.device_grid(G.grid(0))
    ret, _ = rig.get(s)[2].get_batch([(chest.q, C.build_sf(s), cfg, dptr)])
    assert ret == -1
