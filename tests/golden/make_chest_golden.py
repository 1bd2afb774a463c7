"""Generate tests/golden/chest_golden.npz and chest_mbsfn_tdd_golden.npz from the reference's own compiled chest_dl.c.

Run where the reference tree exists (REF as in oracle/Makefile, the directory that holds include/ and src/):
    python tests/golden/make_chest_golden.py [REF]
The REFSRC list of oracle/Makefile plus ch_estimation/chest_dl.c, ch_estimation/refsignal_dl.c, resampling/interp.c
and sync/pss.c are compiled into a temporary directory together with the small harness below (our own code: it only
calls the reference's functions), an empty stand-in srsran/version.h and stubs for the four srsran_wiener_dl_*
functions and srsran_phy_log_print.  pss.c leaves srsran_dft_* undefined: the library is linked with
--unresolved-symbols=ignore-all and opened RTLD_LAZY (nothing called here reaches them).  The directory is removed
afterwards; only arrays are kept.

Two builds: (1) the flags of oracle/Makefile (-Ofast, AVX2, FMA) and (2) a plain scalar one (-O1 -ffp-contract=off,
no LV_HAVE_*).  Every recorded quantity is produced by both; the fixture stores build 1's values and, per case and
quantity, the largest distance between the builds in the unit of its tolerance (tests/chest_cases.py: TOL, err).

Inputs (tests/chest_cases.py: SCENES): the reference puts its own CRS / MBSFN reference signals and the PSS of
subframes 0 / 5 (FDD); numpy adds QPSK data on the other REs, a smooth 3-tap channel per (port, rx), a phase advance
of ROT cycles per symbol, the scene's timing ramp and AWGN at SNR_DB, and rounds to int16 / QSCALE, which is what
the reference then runs on and what the fixture stores.

No file is written unless
  (a) every spread is at most a quarter of its tolerance;
  (b) where a relative tolerance is used, |cfo| >= CFO_FLOOR and |sync_error| >= SYNC_FLOOR (the scene with a
      0.01-sample ramp must instead stay under the threshold and get its grids back untouched);
  (c) every knob of KNOB_PAIRS is observable: the two cases differ in that knob alone and in some recorded output by
      at least 10 x its tolerance.
"""
import concurrent.futures
import ctypes
import io
import os
import re
import subprocess
import sys
import tempfile
import zipfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chest_cases as C  # noqa: E402

EXTRA = ["src/phy/ch_estimation/chest_dl.c", "src/phy/ch_estimation/refsignal_dl.c", "src/phy/resampling/interp.c",
         "src/phy/sync/pss.c"]
SCALAR_FLAGS = ["-std=c99", "-D_GNU_SOURCE", "-O1", "-fPIC", "-fno-strict-aliasing", "-ffp-contract=off", "-w"]
MAX_BYTES = C.MAX_FIXTURE_BYTES
NOUT = 112

STUBS = r'''
#include <stdint.h>
int  srsran_wiener_dl_init(void* q, uint32_t max_prb, uint32_t max_tx_ports, uint32_t max_rx_ant) { return 0; }
int  srsran_wiener_dl_set_cell(void* q) { return 0; }
void srsran_wiener_dl_free(void* q) {}
int  srsran_wiener_dl_run(void* q) { return 0; }
void srsran_phy_log_print(int level, const char* format, ...) {}
'''

HARNESS = r'''
#include <complex.h>
#include <stdlib.h>
#include <string.h>
#include "srsran/srsran.h"
#include "srsran/phy/ch_estimation/chest_dl.h"
#include "srsran/phy/ch_estimation/refsignal_dl.h"
#include "srsran/phy/sync/pss.h"

typedef struct {
  srsran_chest_dl_t     q;
  srsran_chest_dl_res_t res;
  srsran_cell_t         cell;
  uint32_t              n;
} cg_t;

int cg_symbol_sz(uint32_t nof_prb) { return srsran_symbol_sz(nof_prb); }

cg_t* cg_open(uint32_t nof_prb, uint32_t id, uint32_t ports, uint32_t nrx, int cp, int tdd)
{
  cg_t* h = calloc(1, sizeof(cg_t));
  h->cell.nof_prb = nof_prb, h->cell.id = id, h->cell.nof_ports = ports;
  h->cell.cp = cp ? SRSRAN_CP_EXT : SRSRAN_CP_NORM, h->cell.phich_resources = SRSRAN_PHICH_R_1;
  h->cell.frame_type = tdd ? SRSRAN_TDD : SRSRAN_FDD;
  h->n = 2 * SRSRAN_CP_NSYMB(h->cell.cp) * 12 * nof_prb;
  if (srsran_chest_dl_init(&h->q, nof_prb, nrx) || srsran_chest_dl_res_init(&h->res, nof_prb) ||
      srsran_chest_dl_set_cell(&h->q, h->cell)) {
    return NULL;
  }
  return h;
}

int cg_set_area(cg_t* h, uint32_t area) { return srsran_chest_dl_set_mbsfn_area_id(&h->q, (uint16_t)area); }

void cg_close(cg_t* h)
{
  srsran_chest_dl_free(&h->q);
  srsran_chest_dl_res_free(&h->res);
  free(h);
}

static srsran_dl_sf_cfg_t sf_cfg(const uint32_t* s)
{
  srsran_dl_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  sf.tti = s[0], sf.tdd_config.sf_config = s[1], sf.tdd_config.ss_config = s[2], sf.tdd_config.configured = s[3] != 0;
  sf.sf_type = s[4] ? SRSRAN_SF_MBSFN : SRSRAN_SF_NORM;
  return sf;
}

/* the reference signals of one port (and the PSS of subframes 0 / 5, FDD) into a zeroed grid.
 * s: tti, sf_config, ss_config, configured, mbsfn, area */
int cg_tx(cg_t* h, const uint32_t* s, uint32_t port, cf_t* grid)
{
  srsran_dl_sf_cfg_t sf = sf_cfg(s);
  memset(grid, 0, h->n * sizeof(cf_t));
  if (s[4]) {
    return srsran_refsignal_mbsfn_put_sf(h->cell, port, h->q.csr_refs.pilots[port / 2][s[0] % 10],
                                         h->q.mbsfn_refs[s[5]]->pilots[port / 2][s[0] % 10], grid);
  }
  if (srsran_refsignal_cs_put_sf(&h->q.csr_refs, &sf, port, grid)) {
    return -1;
  }
  if (h->cell.frame_type == SRSRAN_FDD && (s[0] % 10 == 0 || s[0] % 10 == 5)) {
    srsran_pss_put_slot(h->q.pss_signal, grid, h->cell.nof_prb, h->cell.cp);
  }
  return 0;
}

/* c: estimator, noise algorithm, filter type, coef 0, coef 1, cfo estimate enable, sync error enable, zeroed
 * configuration (srsran_chest_dl_estimate).  grids [rx][n] (corrected in place), ce [port][rx][n], out[112] */
int cg_run(cg_t* h, const uint32_t* s, const float* c, cf_t* grids, cf_t* ce, float* out)
{
  srsran_dl_sf_cfg_t    sf = sf_cfg(s);
  srsran_chest_dl_cfg_t cfg;
  cf_t*                 in[SRSRAN_MAX_PORTS] = {0};
  const uint32_t        nrx = h->q.nof_rx_antennas, np = h->cell.nof_ports;
  memset(&cfg, 0, sizeof(cfg));
  cfg.estimator_alg = (srsran_chest_dl_estimator_alg_t)(int)c[0], cfg.noise_alg = (srsran_chest_dl_noise_alg_t)(int)c[1];
  cfg.filter_type = (srsran_chest_filter_t)(int)c[2], cfg.filter_coef[0] = c[3], cfg.filter_coef[1] = c[4];
  cfg.mbsfn_area_id = (uint16_t)s[5], cfg.cfo_estimate_enable = c[5] != 0, cfg.cfo_estimate_sf_mask = 1023;
  cfg.sync_error_enable = c[6] != 0;
  for (uint32_t r = 0; r < nrx; r++) {
    in[r] = grids + (size_t)r * h->n;
  }
  int rc = c[7] != 0 ? srsran_chest_dl_estimate(&h->q, &sf, in, &h->res)
                     : srsran_chest_dl_estimate_cfg(&h->q, &sf, &cfg, in, &h->res);
  for (uint32_t p = 0; p < np; p++) {
    for (uint32_t r = 0; r < nrx; r++) {
      memcpy(ce + ((size_t)p * nrx + r) * h->n, h->res.ce[p][r], h->n * sizeof(cf_t));
    }
  }
  const srsran_chest_dl_res_t* e = &h->res;
  out[0] = e->noise_estimate, out[1] = e->noise_estimate_dbm, out[2] = e->snr_db, out[3] = e->rsrp, out[4] = e->rsrp_dbm;
  out[5] = e->rsrp_neigh, out[6] = e->rsrq, out[7] = e->rsrq_db, out[8] = e->rssi_dbm, out[9] = e->cfo;
  out[10] = e->sync_error;
  memcpy(out + 11, e->rsrp_port_dbm, 4 * sizeof(float));
  memcpy(out + 15, e->snr_ant_port_db, 16 * sizeof(float));
  memcpy(out + 31, e->rsrp_ant_port_dbm, 16 * sizeof(float));
  memcpy(out + 47, e->rsrq_ant_port_db, 16 * sizeof(float));
  memcpy(out + 63, h->q.noise_estimate, 16 * sizeof(float));
  memcpy(out + 79, h->q.rsrp, 16 * sizeof(float));
  memcpy(out + 95, h->q.rssi, 16 * sizeof(float));
  out[111] = h->q.cfo;
  return rc;
}
'''


def build_reference(ref, d, scalar):
    """as make_pucch_golden.py builds its library; scalar: the second, plain build"""
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read().replace("\\\n", " ")
    var = lambda n: re.search(r"^%s\s*:?=\s*(.*)$" % n, mk, flags=re.M).group(1)  # noqa: E731
    ldpc = var("LDPCSRC").split()
    refsrc = var("REFSRC").replace("$(addprefix src/phy/fec/ldpc/,$(LDPCSRC))", " ".join("src/phy/fec/ldpc/" + f for f in ldpc))
    oflags = var("OFLAGS").split()
    refflags = var("REFFLAGS").replace("$(OFLAGS)", " ".join(oflags)).split()
    nofast = [f for f in refflags if f != "-Ofast"] + ["-fno-trapping-math", "-fno-math-errno"]
    if scalar:
        refflags = nofast = SCALAR_FLAGS
    os.makedirs(os.path.join(d, "srsran"))
    open(os.path.join(d, "srsran", "version.h"), "w").write("/* stand-in for the generated header */\n")
    open(os.path.join(d, "stubs.c"), "w").write(STUBS)
    open(os.path.join(d, "harness.c"), "w").write(HARNESS)
    inc = ["-I", d, "-I", os.path.join(ref, "include")]
    jobs = []
    for src in refsrc.split() + EXTRA:
        if scalar and re.search(r"avx|sse", os.path.basename(src)):
            continue  # SIMD-only translation units: empty without LV_HAVE_*, and not compilable without -mavx2
        jobs.append((os.path.join(ref, src), nofast if src.endswith("precoding.c") else refflags))
    jobs += [(os.path.join(d, "stubs.c"), refflags), (os.path.join(d, "harness.c"), refflags)]

    def cc(job):
        src, flags = job
        obj = os.path.join(d, os.path.basename(src)[:-2] + ".o")
        subprocess.run(["gcc"] + flags + inc + ["-c", src, "-o", obj], check=True)
        return obj

    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        objs = list(ex.map(cc, jobs))
    so = os.path.join(d, "libchestref.so")
    subprocess.run(["gcc", "-shared", "-Wl,-Bsymbolic", "-Wl,--unresolved-symbols=ignore-all", "-o", so] + objs + ["-lm"],
                   check=True)
    L = ctypes.CDLL(so, mode=os.RTLD_LAZY)
    L.cg_open.restype = ctypes.c_void_p
    L.cg_open.argtypes = [ctypes.c_uint32] * 4 + [ctypes.c_int] * 2
    L.cg_set_area.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    L.cg_close.argtypes = [ctypes.c_void_p]
    L.cg_tx.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    L.cg_run.argtypes = [ctypes.c_void_p] * 6
    return L


def sf_words(sc, i):
    tdd = sc["tdd"]
    return np.array([sc["ttis"][i], tdd[0] if tdd else 0, tdd[1] if tdd else 0, 1 if tdd else 0, sc["mbsfn"][i],
                     sc["areas"][i]], np.uint32)


def open_cell(L, sc, ports=None):
    h = L.cg_open(sc["nof_prb"], sc["cell_id"], ports or sc["ports"], sc["nrx"], sc["cp"], 1 if sc["tdd"] else 0)
    assert h, sc["name"]
    for a in sorted(set(sc["areas"])):
        if a:
            assert L.cg_set_area(h, a) == 0
    return h


def dims(sc):
    nsymb = 6 if sc["cp"] else 7
    nre = 12 * sc["nof_prb"]
    return nsymb, nre, 2 * nsymb * nre


def make_inputs(L, sc):
    """the scene's received grids, as stored: int16 (nsf, nrx, n, 2)"""
    rng = np.random.default_rng(1000 + sc["seed"])
    nprb, ports, nrx = sc["nof_prb"], sc["ports"], sc["nrx"]
    nsymb, nre, n = dims(sc)
    rows, N = 2 * nsymb, C.SYMBOL_SZ[nprb]
    assert L.cg_symbol_sz(nprb) == N
    h = open_cell(L, sc)
    k = np.arange(nre)
    H = np.zeros((ports, nrx, nre), np.complex128)
    for p in range(ports):
        for r in range(nrx):
            a = rng.standard_normal(3) + 1j * rng.standard_normal(3)
            e = sc["echo"]
            H[p, r] = a[0] + e * a[1] * np.exp(2j * np.pi * k * 0.8 / nre) + 0.3 * e * a[2] * np.exp(-2j * np.pi * k * 2.3 / nre)
    out = np.zeros((len(sc["ttis"]), nrx, n, 2), np.int16)
    for i, tti in enumerate(sc["ttis"]):
        s = sf_words(sc, i)
        tx = np.zeros((ports, rows, nre), np.complex64)
        for p in range(ports):
            g = np.zeros(n, np.complex64)
            assert L.cg_tx(h, s.ctypes.data, p, g.ctypes.data) == 0
            tx[p] = g.reshape(rows, nre)
        resv = (tx != 0).any(axis=0)  # reference signals of any port, the PSS
        if not sc["tdd"] and not sc["mbsfn"][i] and tti % 10 in (0, 5):  # the empty subcarriers beside PSS and SSS
            kp = nre // 2 - 31
            for row in (nsymb - 2, nsymb - 1):
                resv[row, kp - 5:kp] = True
                resv[row, kp + 62:kp + 67] = True
        sent = rows
        if sc["mbsfn"][i]:
            sent = 12  # extended-CP symbols; rows 12 / 13 of a normal-CP buffer hold noise
        elif sc["tdd"] and tti % 10 in (1, 6):
            sent = {0: 3, 1: 9, 4: 12}[sc["tdd"][1]]  # the DwPTS
        X = (rng.choice([-1, 1], (ports, rows, nre)) + 1j * rng.choice([-1, 1], (ports, rows, nre))) / np.sqrt(2)
        X[:, resv] = 0
        X = X + tx
        X[:, sent:] = 0
        Y = np.einsum("prk,psk->rsk", H, X)
        Y = Y * np.exp(2j * np.pi * C.ROT * np.arange(rows))[None, :, None]
        if sc["delay"]:
            Y = Y * np.exp(-2j * np.pi * sc["delay"] * k / N)[None, None, :]
        sig = 10 ** (-C.SNR_DB / 20)
        Y = Y + sig * (rng.standard_normal(Y.shape) + 1j * rng.standard_normal(Y.shape)) / np.sqrt(2)
        q = np.round(np.stack([Y.real, Y.imag], axis=-1).reshape(nrx, n, 2) * C.QSCALE)
        assert np.abs(q).max() < 32767
        out[i] = q.astype(np.int16)
    L.cg_close(h)
    return out


def run_case(L, sc, cs, Y):
    """the case's three calls on one reference object -> dict of arrays (per call, first axis)"""
    ports, nrx = sc["ports"], sc["nrx"]
    nsymb, nre, n = dims(sc)
    nsf = len(sc["ttis"])
    h = open_cell(L, sc)
    h2 = open_cell(L, sc, 2) if ports == 4 else None
    cfo_en = 0 if cs["zero"] else 1
    o = dict(ce=np.zeros((nsf, ports, nrx, n), np.complex64), out=np.zeros((nsf, NOUT), np.float32),
             grid=np.zeros((nsf, nrx, n), np.complex64), cfo_ports01=np.zeros(nsf, np.float32))
    for i in range(nsf):
        s = sf_words(sc, i)
        g = np.ascontiguousarray(Y[i]).copy()
        c = np.array([cs["est"], cs["noise"], cs["ftype"], cs["c0"], cs["c1"], cfo_en, cs["sync"], cs["zero"]], np.float32)
        assert L.cg_run(h, s.ctypes.data, c.ctypes.data, g.ctypes.data, o["ce"][i].ctypes.data, o["out"][i].ctypes.data) == 0
        o["grid"][i] = g
        if h2:  # ports 0 / 1 do not move with nof_ports: the CFO of a 2-port object on the (corrected) grids
            c[6] = 0
            ce2, out2 = np.zeros((2, nrx, n), np.complex64), np.zeros(NOUT, np.float32)
            assert L.cg_run(h2, s.ctypes.data, c.ctypes.data, g.copy().ctypes.data, ce2.ctypes.data, out2.ctypes.data) == 0
            o["cfo_ports01"][i] = out2[9]
    L.cg_close(h)
    if h2:
        L.cg_close(h2)
    return o


def fields(sc, cs, o):
    """the recorded quantities by name (tests/chest_cases.py: QUANTITIES); `res` is the record the fixture stores"""
    nsf = len(sc["ttis"])
    res = np.concatenate([o["out"], np.zeros((nsf, 1), np.float32), o["cfo_ports01"][:, None]], axis=1)
    assert res.shape == (nsf, C.RES_LEN)
    f = C.res_fields(res, sc["nrx"], sc["ports"])
    f["res"], f["ce"], f["grid"] = res, o["ce"], o["grid"]
    return f


def spread(sc, f1, f2):
    """per quantity, the largest distance between the two builds over the case's calls, in the tolerance's unit"""
    v = []
    for name in C.QUANTITIES:
        kind = C.KIND[name]
        v.append(max(C.err(kind, f2[name][i], f1[name][i]) for i in range(len(sc["ttis"]))))
    return np.array(v, np.float64)


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: a second run gives the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF")
    if not ref:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        ref = re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    if not os.path.exists(os.path.join(ref, "src/phy/ch_estimation/chest_dl.c")):
        sys.exit(f"reference tree not found at {ref}")
    scenes, cases = C.by_name(C.SCENES), C.by_name(C.CASES)
    assert len(cases) == len(C.CASES) and len(scenes) == len(C.SCENES)
    files = {k: {} for k in C.FILES}
    tables = {k: dict(cases=[], res=[], spread=[]) for k in C.FILES}
    rec, worst = {}, {name: 0.0 for name in C.QUANTITIES}
    with tempfile.TemporaryDirectory() as d:
        L1 = build_reference(ref, os.path.join(d, "b1"), False)
        L2 = build_reference(ref, os.path.join(d, "b2"), True)
        inputs = {}
        for sc in C.SCENES:
            q = make_inputs(L1, sc)
            assert np.array_equal(q, make_inputs(L2, sc)), sc["name"]
            inputs[sc["name"]] = q
            files[sc["file"]]["in." + sc["name"]] = q
        for cs in C.CASES:
            sc = scenes[cs["scene"]]
            Y = C.unpack_grids(inputs[sc["name"]])
            f1, f2 = fields(sc, cs, run_case(L1, sc, cs, Y)), fields(sc, cs, run_case(L2, sc, cs, Y))
            sp = spread(sc, f1, f2)
            rec[cs["name"]] = f1
            nsymb, nre, _ = dims(sc)
            nsf = len(sc["ttis"])
            # (a)
            for name, v in zip(C.QUANTITIES, sp):
                worst[name] = max(worst[name], v)
                assert v <= C.TOL[C.KIND[name]] / 4, (cs["name"], name, v)
            # the values the tests expect of res->cfo: ports 0 / 1 in a 4-port cell, kept where nothing is estimated
            base = f1["cfo_ports01"] if sc["ports"] == 4 else f1["cfo"]
            expect = np.zeros(nsf, np.float32)
            for i, tti in enumerate(sc["ttis"]):
                own = not cs["zero"] and not sc["mbsfn"][i] and C.crs_nsym(sc, tti)[0] == 4
                expect[i] = base[i] if own else (expect[i - 1] if i else 0.0)
                if sc["ports"] < 4 and (own or sc["mbsfn"][i] or cs["zero"]):
                    assert expect[i] == f1["cfo"][i] == f1["q_cfo"][i], (cs["name"], i)
                # (b)
                assert cs["zero"] or abs(expect[i]) >= C.CFO_FLOOR, (cs["name"], i, expect[i])
            rotated = np.array([[not np.array_equal(f1["grid"][i, r], Y[i, r]) for r in range(sc["nrx"])]
                                for i in range(nsf)])
            if cs["sync"] and sc["delay"] >= 0.1:
                assert (np.abs(f1["sync_error"]) >= C.SYNC_FLOOR).all() and rotated.all(), cs["name"]
            elif cs["sync"]:
                assert (np.abs(f1["sync_error"]) < C.SYNC_FLOOR).all() and not rotated.any(), cs["name"]
                assert (f1["sync_error"] != 0).all()
            else:
                assert not rotated.any() and (f1["sync_error"] == 0).all(), cs["name"]
            out = files[sc["file"]]
            pre = cs["name"] + "."
            ce = f1["ce"].reshape(nsf, sc["ports"], sc["nrx"], 2 * nsymb, nre)
            if cs["est"] == C.AVERAGE:  # one row per (port, rx): every row the reference writes is that row
                assert not any(sc["mbsfn"]) and np.array_equal(ce, np.broadcast_to(ce[:, :, :, :1], ce.shape)), cs["name"]
                ce = ce[:, :, :, 0]
            out[pre + "ce"] = np.ascontiguousarray(ce)
            f1["res"][:, 112] = expect
            res = np.zeros((3, C.RES_LEN), np.float32)
            res[:nsf] = f1["res"]
            table = tables[sc["file"]]
            table["cases"].append(cs["name"])
            table["res"].append(res)
            table["spread"].append(sp)
            if rotated.any():
                out[pre + "grid"] = f1["grid"]
            print("%-24s %s" % (cs["name"], " ".join("%s %.1e" % (nm, v) for nm, v in zip(C.QUANTITIES, sp) if v > 0)))
    # (c)
    for knob, a, b in C.KNOB_PAIRS:
        ca, cb = cases[a], cases[b]
        diff = {k for k in ca if k not in ("name",) and ca[k] != cb[k]}
        assert diff and diff <= set(C.KNOB_FIELDS[knob]) and ca["scene"] == cb["scene"], (knob, a, b, diff)
        sc = scenes[ca["scene"]]
        ratio = max(C.err(C.KIND[name], rec[b][name][i], rec[a][name][i]) / C.TOL[C.KIND[name]]
                    for name in C.QUANTITIES for i in range(len(sc["ttis"])))
        print("knob %-20s %-22s %-22s differ by %.3g x tolerance" % (knob, a, b, ratio))
        assert ratio >= 10, (knob, a, b, ratio)
    print("largest spread between the two builds per quantity (unit of its tolerance):")
    for name in C.QUANTITIES:
        print("  %-20s %-5s %.2e (tolerance %.0e)" % (name, C.KIND[name], worst[name], C.TOL[C.KIND[name]]))
    too_big = []
    for key, arrays in files.items():
        arrays["cases"] = np.array(tables[key]["cases"])
        arrays["res"] = np.stack(tables[key]["res"])
        arrays["spread"] = np.stack(tables[key]["spread"])
        tmp = os.path.join(HERE, C.FILES[key]) + ".tmp"
        write_npz(tmp, arrays)
        size = os.path.getsize(tmp)
        print(f"{C.FILES[key]}: {len(arrays)} arrays, {size} bytes")
        if size > MAX_BYTES:
            for k in sorted(arrays, key=lambda k: -np.asarray(arrays[k]).nbytes)[:25]:
                print("  %-32s %8d bytes deflated" % (k, len(zlib.compress(np.asarray(arrays[k]).tobytes(), 9))))
            too_big.append(f"{C.FILES[key]} would be {size} bytes, more than {MAX_BYTES}")
    for key in files:  # both files or neither
        tmp = os.path.join(HERE, C.FILES[key]) + ".tmp"
        if too_big:
            os.remove(tmp)
        else:
            os.replace(tmp, tmp[:-4])
    if too_big:
        sys.exit("; ".join(too_big))


if __name__ == "__main__":
    main()
