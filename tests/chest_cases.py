"""Case table of the DL channel estimator's reference fixtures (tests/golden/chest_golden.npz and
chest_mbsfn_tdd_golden.npz), shared by tests/golden/make_chest_golden.py, tests/test_chest_golden.py and
tests/test_chest_ref_gpu.py: plain numbers, then the tolerances, the distance each is measured in, and the
fixture's layout.

A SCENE is a sequence of three received subframes (one at 100 PRB) on one estimator object; several CASES -- estimator
configurations -- run on the same scene, so that the received grids are stored once and two cases that differ in one
knob see the same input.  The shapes are the smallest at which chest_kernel can still go wrong:
  6 PRB    one CRS symbol's 48 pilots (4 symbols x 12) fit in one wave and nre = 72 is smaller than the workgroup
           (row / column stepping of the RSSI loads)
  15 PRB   odd, nref = 30
  25 PRB
  50 PRB   400 LS estimates: more than one pass of the pilot-load loop
  100 PRB  one single-subframe AVERAGE case
cell ids with id % 6 = 0, 2 and 5 (with 5 the shifted CRS offset wraps past 5); ports 1, 2 and 4; 1 and 2 rx antennas.

FDD scenes run subframes (4, 5, 6): PSS / EMPTY noise is zero before the first subframe 5, estimated in it and kept
after it.  TDD scenes run subframes (0, 1, 4) of configuration 1 with special-subframe configurations 0 / 1 / 4, whose
DwPTS (normal CP) holds 1 / 3 / 4 CRS symbols of ports 0 / 1.  MBSFN scenes run a normal subframe 5 first (rows 12 / 13
of the estimate, RSRP / RSSI / CFO and the kept PSS noise come from it) and then two MBSFN subframes, each with its own
area id.

Left out, because the library refuses them (each refusal has its own test):
  * the WIENER estimator and rsrp_neighbour: not provided (test_ue_dl_batch_refused_config_then_good_batch);
  * INTERPOLATE with 2 CRS symbols in a DwPTS: the reference interpolates towards rows it did not estimate in that
    call (test_chest_interpolate_refused);
  * MBSFN with AVERAGE, with ports 2 / 3 or in subframes 0 / 5: the reference reads rows it did not write, or the
    subframe cannot be MBSFN (test_chest_mbsfn_refused);
  * Gauss filter orders above 7: longer than the kernel's filter registers (cfg_supported, chest_api.cpp).
Nothing else is left out, and neither test skips or filters a case.

4-port cells: the reference's res->cfo there is a product of port 3's estimates with stale rows of port 1
("4-port CFO"); the fixture keeps it as `cfo` and both tests compare with `cfo_expect`, the CFO a second
reference object with 2 ports finds on the same grids.  In a TDD special subframe `cfo_expect` is the last full
subframe's value (the library's other documented deviation)."""

SYMBOL_SZ = {6: 128, 15: 256, 25: 384, 50: 768, 100: 1536}  # srsran_symbol_sz at the reference's default rates

AVERAGE, INTERPOLATE = 0, 1
REFS, PSS, EMPTY = 0, 1, 2
GAUSS, TRIANGLE, NONE = 0, 1, 2

SNR_DB = 25.0       # AWGN
ROT = 0.02          # phase advance, cycles per OFDM symbol: the CFO estimate is far from 0
QSCALE = 32.0       # the received grids are stored as int16: value * QSCALE (what the reference ran on, exactly)

FILES = {"fdd": "chest_golden.npz", "mt": "chest_mbsfn_tdd_golden.npz"}
MAX_FIXTURE_BYTES = 650613  # each file: the size of the largest fixture committed before these (phy_golden.npz)


def scene(name, file, nof_prb, cell_id, ports, nrx, cp=0, ttis=(4, 5, 6), tdd=None, mbsfn=(0, 0, 0), areas=(0, 0, 0),
          delay=0.0, echo=1.0, seed=0):
    """delay: timing ramp, samples; echo: weight of the channel's two echoes (their own delay is a timing error too:
    the scene that must stay under correct_sync_error's threshold has a nearly flat channel)"""
    return dict(name=name, file=file, nof_prb=nof_prb, cell_id=cell_id, ports=ports, nrx=nrx, cp=cp, ttis=ttis,
                tdd=tdd, mbsfn=mbsfn[:len(ttis)], areas=areas[:len(ttis)], delay=delay, echo=echo, seed=seed)


SCENES = [
    # FDD
    scene("f6a", "fdd", 6, 11, 4, 2, delay=0.4, seed=1),        # id % 6 = 5, a timing error of 0.4 samples
    scene("f6b", "fdd", 6, 2, 4, 1, seed=2),                    # id % 6 = 2
    scene("f6c", "fdd", 6, 6, 1, 2, cp=1, seed=3),              # id % 6 = 0, extended CP, PSS noise
    scene("f15a", "fdd", 15, 5, 2, 1, seed=4),                  # id % 6 = 5
    scene("f15b", "fdd", 15, 12, 1, 1, cp=1, seed=5),           # PSS noise
    scene("f25a", "fdd", 25, 302, 2, 1, delay=0.01, echo=0.01, seed=6),  # id % 6 = 2, under the sync threshold
    scene("f50a", "fdd", 50, 17, 2, 1, seed=8),                 # id % 6 = 5
    scene("f100", "fdd", 100, 0, 2, 1, ttis=(5,), seed=10),
    # TDD configuration 1: subframe 1 is special
    scene("t50", "mt", 50, 17, 2, 1, ttis=(0, 1, 4), tdd=(1, 0), seed=11),          # 1 CRS symbol
    scene("t6", "mt", 6, 8, 4, 1, ttis=(0, 1, 4), tdd=(1, 1), seed=12),             # 3 / 2 CRS symbols
    scene("t15a", "mt", 15, 5, 2, 2, ttis=(0, 1, 4), tdd=(1, 4), seed=13),          # 4 / 2 CRS symbols
    scene("t15b", "mt", 15, 6, 1, 1, ttis=(0, 1, 4), tdd=(1, 0), seed=14),          # 1 CRS symbol
    scene("t25", "mt", 25, 302, 2, 1, cp=1, ttis=(0, 1, 4), tdd=(1, 1), seed=15),   # extended CP: 3 / 2 CRS symbols
    # MBSFN
    scene("m6", "mt", 6, 4, 2, 1, ttis=(5, 6, 7), mbsfn=(0, 1, 1), areas=(0, 1, 37), seed=16),
    scene("m15", "mt", 15, 9, 1, 2, ttis=(5, 6, 7), mbsfn=(0, 1, 1), areas=(0, 37, 1), seed=17),
]


def case(name, scene_, est=AVERAGE, noise=REFS, ftype=GAUSS, c0=4.0, c1=1.0, sync=0, zero=0):
    """zero: srsran_chest_dl_estimate, the zeroed configuration (AVERAGE, REFS, automatic Gauss, no CFO estimate)"""
    if zero:
        est, noise, ftype, c0, c1, sync = AVERAGE, REFS, GAUSS, 0.0, 0.0, 0
    return dict(name=name, scene=scene_, est=est, noise=noise, ftype=ftype, c0=c0, c1=c1, sync=sync, zero=zero)


CASES = [
    # 6 PRB, 4 ports, 2 rx
    case("f6a_avg", "f6a"),
    case("f6a_avg_sync", "f6a", sync=1),
    # 6 PRB, 4 ports, 1 rx: full grids
    case("f6b_int", "f6b", est=INTERPOLATE),
    case("f6b_avg", "f6b"),
    # 6 PRB, 1 port, 2 rx, extended CP
    case("f6c_int_pss_none", "f6c", est=INTERPOLATE, noise=PSS, ftype=NONE, c0=0.0, c1=0.0),
    case("f6c_int_empty_g2", "f6c", est=INTERPOLATE, noise=EMPTY, c0=2.0, c1=1.0),
    case("f6c_avg_pss", "f6c", noise=PSS),
    case("f6c_avg_refs", "f6c"),
    case("f6c_avg_empty", "f6c", noise=EMPTY),
    # 15 PRB: the Gauss orders with two stddevs each, the automatic filter, TRIANGLE, NONE
    case("f15a_zero", "f15a", zero=1),
    case("f15a_avg_auto", "f15a", c0=0.0, c1=0.0),
    case("f15a_g2_s1", "f15a", c0=2.0, c1=1.0),
    case("f15a_g2_s2", "f15a", c0=2.0, c1=2.0),
    case("f15a_g4_s1", "f15a", c0=4.0, c1=1.0),
    case("f15a_g4_s2", "f15a", c0=4.0, c1=2.0),
    case("f15a_g6_s1", "f15a", c0=6.0, c1=1.0),
    case("f15a_g6_s2", "f15a", c0=6.0, c1=2.0),
    case("f15a_avg_tri", "f15a", ftype=TRIANGLE, c0=0.25, c1=0.0),
    case("f15a_avg_none", "f15a", ftype=NONE, c0=0.0, c1=0.0),
    case("f15b_int_pss_auto", "f15b", est=INTERPOLATE, noise=PSS, c0=0.0, c1=0.0),
    case("f15b_avg_pss_auto", "f15b", noise=PSS, c0=0.0, c1=0.0),
    # 25 PRB
    case("f25a_avg", "f25a"),
    case("f25a_avg_sync_small", "f25a", sync=1),
    # 50 PRB
    case("f50a_avg", "f50a"),
    case("f50a_avg_empty_g6", "f50a", noise=EMPTY, c0=6.0, c1=2.0),
    # 100 PRB
    case("f100_avg", "f100"),
    # TDD
    case("t50_avg", "t50"),
    case("t6_avg", "t6"),
    case("t6_int", "t6", est=INTERPOLATE),
    case("t15a_avg", "t15a"),
    case("t15a_avg_auto", "t15a", c0=0.0, c1=0.0),
    case("t15b_int", "t15b", est=INTERPOLATE),
    case("t15b_avg_none", "t15b", ftype=NONE, c0=0.0, c1=0.0),
    case("t25_avg", "t25"),
    # MBSFN: srsUE's configuration (cc_worker.cc: TRIANGLE 0.1, INTERPOLATE, PSS noise) and a Gauss one
    case("m6_srsue", "m6", est=INTERPOLATE, noise=PSS, ftype=TRIANGLE, c0=0.1, c1=0.0),
    case("m6_gauss", "m6", est=INTERPOLATE, noise=REFS, ftype=GAUSS, c0=4.0, c1=1.0),
    case("m15_srsue", "m15", est=INTERPOLATE, noise=PSS, ftype=TRIANGLE, c0=0.1, c1=0.0),
]

# every knob is observable: the two cases differ in that knob alone and, in some recorded output, by at least 10 x
# the tolerance (the generator checks both)
KNOB_PAIRS = [
    ("estimator", "f6b_int", "f6b_avg"),
    ("noise algorithm", "f6c_avg_refs", "f6c_avg_empty"),
    ("noise algorithm", "f6c_avg_pss", "f6c_avg_refs"),
    ("filter type", "f15a_g4_s1", "f15a_avg_tri"),
    ("filter type", "f15a_g4_s1", "f15a_avg_none"),
    ("filter order/stddev", "f15a_g2_s1", "f15a_g4_s1"),
    ("filter order/stddev", "f15a_g4_s1", "f15a_g6_s1"),
    ("filter order/stddev", "f15a_g2_s1", "f15a_g2_s2"),
    ("filter order/stddev", "f15a_g4_s1", "f15a_g4_s2"),
    ("filter order/stddev", "f15a_g6_s1", "f15a_g6_s2"),
    ("automatic filter", "f15a_g4_s1", "f15a_avg_auto"),
    ("sync correction", "f6a_avg", "f6a_avg_sync"),
]
KNOB_FIELDS = {"estimator": ("est",), "noise algorithm": ("noise",), "filter type": ("ftype", "c0", "c1"),
               "filter order/stddev": ("c0", "c1"), "automatic filter": ("c0", "c1"), "sync correction": ("sync",)}

# ---- tolerances (the project's own: test_chest_gpu.py against the restatement, the soft-value tolerance) ----
TOL = {
    "ce": 2e-5,     # of the largest reference estimate of the call
    "lin": 1e-4,    # relative: noise_estimate, rsrp, rsrq, the per [rx][port] values, cfo
    "sync": 1e-4,   # relative, with absolute 1e-6 (= relative to max(|value|, 1e-2))
    "grid": 1e-5,   # of the largest sample
    "db": 1e-3,     # dB: 10 log10 of a ratio of two `lin` quantities, 10 / ln 10 x 2e-4 = 8.7e-4
}
CFO_FLOOR, SYNC_FLOOR = 1e-4, 0.05  # where a relative tolerance is used (as tests/test_chest_gpu.py)

# name -> (kind, where it lives); the order of the fixture's `spread` vector
SCALARS = ("noise_estimate", "noise_estimate_dbm", "snr_db", "rsrp", "rsrp_dbm", "rsrp_neigh", "rsrq", "rsrq_db",
           "rssi_dbm", "cfo", "sync_error")
KIND = {"ce": "ce", "grid": "grid", "noise_estimate": "lin", "noise_estimate_dbm": "db", "snr_db": "db", "rsrp": "lin",
        "rsrp_dbm": "db", "rsrp_neigh": "lin", "rsrq": "lin", "rsrq_db": "db", "rssi_dbm": "db", "cfo": "lin",
        "sync_error": "sync", "rsrp_port_dbm": "db", "snr_ant_port_db": "db", "rsrp_ant_port_dbm": "db",
        "rsrq_ant_port_db": "db", "q_noise": "lin", "q_rsrp": "lin", "q_rssi": "lin", "q_cfo": "lin",
        "cfo_ports01": "lin"}
QUANTITIES = tuple(KIND)


RES_LEN = 114  # one call's scalars and tables as the fixture stores them (`res`: [case][call][RES_LEN])


def res_fields(r, nrx, ports):
    """a `res` record (..., RES_LEN) by name: srsran_chest_dl_res_t's scalars (SCALARS order) and tables, the
    estimator object's per [rx][port] values (q_*), then cfo_expect and cfo_ports01"""
    f = {name: r[..., j] for j, name in enumerate(SCALARS)}
    f["rsrp_port_dbm"] = r[..., 11:11 + ports]
    for j, name in enumerate(("snr_ant_port_db", "rsrp_ant_port_dbm", "rsrq_ant_port_db", "q_noise", "q_rsrp", "q_rssi")):
        f[name] = r[..., 15 + 16 * j:31 + 16 * j].reshape(r.shape[:-1] + (4, 4))[..., :nrx, :ports]
    f["q_cfo"], f["cfo_expect"], f["cfo_ports01"] = r[..., 111], r[..., 112], r[..., 113]
    return f


def by_name(table):
    return {x["name"]: x for x in table}


def err(kind, got, exp):
    """distance of got from exp in the unit of TOL[kind] (the largest over the array); values that are not finite
    (the dB of a zero noise estimate) must be equal"""
    import numpy as np
    got, exp = np.asarray(got), np.asarray(exp)
    if kind in ("ce", "grid"):
        s, d = float(np.abs(exp).max()), float(np.abs(got - exp).max())
        return d / s if s > 0 else (0.0 if d == 0 else float("inf"))
    got, exp = got.astype(np.float64).ravel(), exp.astype(np.float64).ravel()
    fin = np.isfinite(exp)
    if not np.array_equal(got[~fin], exp[~fin], equal_nan=True) or not np.isfinite(got[fin]).all():
        return float("inf")
    got, exp = got[fin], exp[fin]
    if got.size == 0:
        return 0.0
    d = np.abs(got - exp)
    if kind == "db":
        return float(d.max())
    if kind == "sync":
        return float((d / np.maximum(np.abs(exp), 1e-2)).max())
    zero = exp == 0
    if (d[zero] != 0).any():
        return float("inf")
    return float((d[~zero] / np.abs(exp[~zero])).max()) if (~zero).any() else 0.0


def unpack_grids(q):
    """the stored int16 grids (nsf, nrx, n, 2) -> complex64 (nsf, nrx, n): exactly what the reference ran on"""
    import numpy as np
    v = q.astype(np.float32) / np.float32(QSCALE)
    return np.ascontiguousarray(v[..., 0] + 1j * v[..., 1]).astype(np.complex64)


def crs_nsym(sc, tti):
    """CRS symbols of ports 0-1 / 2-3 in subframe tti of a scene (refsignal_dl.c:169-226)"""
    if sc["tdd"] is None or tti % 10 not in (1, 6):
        return (4, 2)
    dw = {0: 3, 1: 9, 4: 12}[sc["tdd"][1]]  # DwPTS symbols (the reference's table, either cyclic prefix)
    if dw >= (10 if sc["cp"] else 12):
        return (4, 2)
    if dw >= (8 if sc["cp"] else 9):
        return (3, 2)
    if dw >= (4 if sc["cp"] else 5):
        return (2, 1)
    return (1, 1)


class Fixture:
    """the two fixture files; a missing file raises (a failure, not a skip)"""

    def __init__(self, golden_dir):
        import os
        import numpy as np
        self.z = {k: np.load(os.path.join(golden_dir, name)) for k, name in FILES.items()}
        self.index = {k: [str(n) for n in z["cases"]] for k, z in self.z.items()}
        self.scenes = by_name(SCENES)

    def inputs(self, sc):
        """(nsf, nrx, n) complex64"""
        return unpack_grids(self.z[sc["file"]]["in." + sc["name"]])

    def case(self, cs):
        """scene, inputs, and the reference's results by name (QUANTITIES, cfo_expect; `ce` (nsf, ports, nrx, rows
        or 1, nre); `grid` only where correct_sync_error rotated one) with the spreads between the two builds"""
        sc = self.scenes[cs["scene"]]
        z, j = self.z[sc["file"]], self.index[sc["file"]].index(cs["name"])
        nsf = len(sc["ttis"])
        ref = res_fields(z["res"][j][:nsf], sc["nrx"], sc["ports"])
        ce = z[cs["name"] + ".ce"]
        ref["ce"] = ce[:, :, :, None, :] if ce.ndim == 4 else ce
        if cs["name"] + ".grid" in z.files:
            ref["grid"] = z[cs["name"] + ".grid"]
        return sc, self.inputs(sc), ref, dict(zip(QUANTITIES, z["spread"][j]))
