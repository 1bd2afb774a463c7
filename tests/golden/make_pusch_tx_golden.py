"""Generate tests/golden/pusch_tx_golden.npz from the reference's own PUSCH transmitter.

Run where the reference tree exists (REF as in oracle/Makefile):
    python tests/golden/make_pusch_tx_golden.py [REF]
The build is tests/golden/make_pusch_golden.py's (its source list, stubs, its O(M^2) double-accumulating
srsran_dft_plan_c / srsran_dft_run_c stand-in for FFTW, its temporary directory that is removed afterwards), with one
more harness function below (our own code: it only calls the reference's functions and reads fields of its structs).
Two builds: the flags of oracle/Makefile, and -O1 -ffp-contract=off with SSE only.

Per case of tests/pusch_tx_cases.py the harness calls srsran_ulsch_encode on zeroed buffers (its return, K_segm, the
packed g bits and the packed q bits before scrambling), then srsran_pusch_encode on a zeroed grid (the written-back
tb.mod / tb.nof_bits, the scrambled q bits with the placeholder rule applied, the modulation symbols d, the grid) and
srsran_refsignal_dmrs_pusch_gen / _put.  t11b runs on the object t11a ran on, without resetting the transmit soft
buffer: the reference reads rv 2 from what rv 0 left there.

Stored: payload, UCI value, those results of build 1 (d for cases of at most 6 PRB; the grid's columns between the
grant's lowest and highest subcarrier only), and MEASURED: per float quantity the largest distance of either build
from a float64 evaluation of the same formulas on the build's own scrambled bits (d: constellation in float64,
max |x - x64| / max |x64|; grid: numpy FFT / sqrt(M), max |x - x64| / rms(x64) over the grant's data REs).  The
table is printed; tests/pusch_tx_cases.py holds a copy and tests/test_pusch_tx_host.py holds the two equal.

No file is written unless
  (a) every return value, K_segm, write-back and every bit (g, q, scrambled q) is the same in both builds;
  (b) the two builds' d and grid lie within the measured distance of each other's float64 evaluation;
  (c) the REs outside the grant's data and DMRS REs are zero;
  (d) each build's DMRS lies within pusch_cases.dmrs_exact's bound of the exact one;
  (e) the reference's own receiver (srsran_chest_ul_estimate_pusch + srsran_pusch_decode, both builds) decodes the
      payload and every UCI field of t2, t4, t6 and t9 from the grid through a 3-tap channel with AWGN at 20 dB;
  (f) the file stays within chest_cases.MAX_FIXTURE_BYTES.
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
import pusch_cases as PC  # noqa: E402
import pusch_tx_cases as TC  # noqa: E402
import uci_cases as UC  # noqa: E402
from srsran_4g_amd import pusch as P  # noqa: E402
from srsran_4g_amd import sch as S  # noqa: E402
from synth.synth import modulate  # noqa: E402

LOOP_CASES = ("t2", "t4", "t6", "t9")
SNR_DB = 20.0

HARNESS_TX = r'''
/* srsran_ulsch_encode on zeroed buffers, then srsran_pusch_encode + the DMRS put on a zeroed grid.
 * out: ulsch_encode's return, K_segm, the written-back tb.mod and tb.nof_bits */
int ph_tx_rec(ph_t* q, uint32_t tti, int shortened, srsran_pusch_cfg_t* cfg, uint8_t* payload, srsran_uci_value_t* uci, int new_tb,
              cf_t* grid, cf_t* r, int32_t* out, uint8_t* g, uint8_t* qb, uint8_t* sb, cf_t* d)
{
  srsran_ul_sf_cfg_t  sf = sf_cfg(tti, shortened);
  srsran_pusch_cfg_t  c  = *cfg, c2;
  srsran_pusch_data_t dat;
  memset(&dat, 0, sizeof(dat));
  dat.ptr = payload, dat.uci = *uci;
  c.softbuffers.tx = &q->sbtx;
  if (new_tb) {
    srsran_softbuffer_tx_reset(&q->sbtx);
  }
  c2 = c; /* what srsran_pusch_encode hands to srsran_ulsch_encode: after the 64QAM limit (pusch.c:269-274) */
  if (!c2.enable_64qam && c2.grant.tb.mod >= SRSRAN_MOD_64QAM) {
    c2.grant.tb.mod = SRSRAN_MOD_16QAM, c2.grant.tb.nof_bits = c2.grant.nof_re * 4;
  }
  const uint32_t nbytes = c2.grant.tb.nof_bits / 8;
  memset(g, 0, nbytes), memset(qb, 0, nbytes);
  out[0] = srsran_ulsch_encode(&q->tx.ul_sch, &c2, payload, uci, g, qb);
  out[1] = (int32_t)c2.K_segm;
  if (out[0] < 0) {
    return -2;
  }
  memset(grid, 0, q->nre * sizeof(cf_t));
  if (srsran_pusch_encode(&q->tx, &sf, &c, &dat, grid) || ph_dmrs(q, tti, &c, r)) {
    return -1;
  }
  srsran_refsignal_dmrs_pusch_put(&q->sig, &c, r, grid);
  out[2] = (int32_t)c.grant.tb.mod, out[3] = (int32_t)c.grant.tb.nof_bits;
  memcpy(sb, q->tx.q, c.grant.tb.nof_bits / 8);
  memcpy(d, q->tx.d, c.grant.nof_re * sizeof(cf_t));
  return 0;
}
'''


def build(ref, d, scalar):
    MG.HARNESS = MG.HARNESS + HARNESS_TX if "ph_tx_rec" not in MG.HARNESS else MG.HARNESS
    L = MG.build_reference(ref, d, scalar)
    vp, u32, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.ph_tx_rec.argtypes = [vp, u32, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp]
    return L


def transmit(L, objs, c):
    """one build's results for case c -> dict"""
    key = c["payload_of"] or c["name"]
    if key not in objs:
        dm = np.array([int(v) for v in c["dmrs"]], np.uint32)
        objs[key] = ctypes.c_void_p(L.ph_new(c["nof_prb"], c["cell_id"], c["cp"], MG.ptr(dm)))
        assert objs[key], c["name"]
    cell, d, sf, cfg = TC.make(c)
    payload, u = TC.payload_uci(c, cfg)
    nre = 2 * PC.nsymb_slot(c["cp"]) * 12 * c["nof_prb"]
    nbytes = cfg.grant.nof_re * 6 // 8 + 16
    grid, r = np.zeros(nre, np.complex64), np.zeros(24 * c["L"], np.complex64)
    g, qb, sb = (np.zeros(nbytes, np.uint8) for _ in range(3))
    dsym, out = np.zeros(cfg.grant.nof_re, np.complex64), np.zeros(4, np.int32)
    pl = np.concatenate([payload, np.zeros(64, np.uint8)])
    rc = L.ph_tx_rec(objs[key], c["tti"], int(c["shortened"]), ctypes.byref(cfg), MG.ptr(pl), ctypes.byref(u),
                     0 if c["payload_of"] else 1, MG.ptr(grid), MG.ptr(r), MG.ptr(out), MG.ptr(g), MG.ptr(qb), MG.ptr(sb),
                     MG.ptr(dsym))
    assert rc == 0, (c["name"], rc)
    nb = int(out[3]) // 8
    return dict(payload=payload, uci=u, out=out, g=g[:nb].copy(), q=qb[:nb].copy(), s=sb[:nb].copy(), d=dsym, r=r,
                grid=grid.reshape(2 * PC.nsymb_slot(c["cp"]), -1), Qm={1: 2, 2: 4, 3: 6}[int(out[2])])


def f64_eval(c, o):
    """the constellation and the transform precoder in float64 on the build's own scrambled bits -> (d64, grid64)"""
    d64 = np.asarray(modulate(np.unpackbits(o["s"]), o["Qm"]), np.complex128)
    M, ns = 12 * c["L"], PC.nsymb_slot(c["cp"])
    grid = np.zeros(o["grid"].shape, np.complex128)
    for i, row in enumerate(TC.data_rows(c)):
        n0 = c["n_tilde"][row // ns] * 12
        grid[row, n0:n0 + M] = np.fft.fft(d64[i * M:(i + 1) * M]) / np.sqrt(M)
    return d64, grid


def loop_check(L, obj, c, o, rng):
    """the reference's own receiver on the grid through a 3-tap channel at SNR_DB: what was sent must come back"""
    cell, d, sf, cfg = TC.make(c)
    k = np.arange(12 * c["nof_prb"])
    taps = np.array([1.0, 0.3 * np.exp(1.1j), 0.12 * np.exp(-0.6j)])
    H = (taps[None, :] * np.exp(-2j * np.pi * np.outer(k, np.arange(3)) / 2048.0)).sum(axis=1) / np.sqrt((np.abs(taps) ** 2).sum())
    y = o["grid"].astype(np.complex128) * H[None, :]
    sigma = np.sqrt(10 ** (-SNR_DB / 10) / 2)
    y = (y + sigma * (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape))).astype(np.complex64).reshape(-1)
    ce, scal = np.zeros(y.size, np.complex64), np.zeros(10, np.float32)
    cfg.meas_ta_en = True
    assert L.ph_est(obj, c["tti"], int(c["shortened"]), ctypes.byref(cfg), 3, MG.ptr(y), MG.ptr(ce), MG.ptr(scal)) == 0
    tbs = cfg.grant.tb.tbs
    data, res = np.zeros(tbs // 8 + 64, np.uint8), P.srsran_pusch_res_t()
    res.data = data.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    sym, llr = np.zeros(cfg.grant.nof_re, np.complex64), np.zeros(cfg.grant.nof_re * 6, np.int16)
    assert L.ph_dec(obj, c["tti"], int(c["shortened"]), ctypes.byref(cfg), 1, MG.ptr(y), ctypes.byref(res), MG.ptr(sym),
                    MG.ptr(llr)) == 0
    u = o["uci"]
    ok = bool(res.crc) and np.array_equal(data[:tbs // 8], o["payload"])
    ok = ok and list(res.uci.ack.ack_value[:c["nack"]]) == list(u.ack.ack_value[:c["nack"]])
    ok = ok and (not c["ri"] or res.uci.ri == u.ri)
    if c["cqi"]:
        ok = ok and bool(res.uci.cqi.data_crc) and UC.cqi_fields(cfg, res.uci.cqi) == UC.cqi_fields(cfg, u.cqi)
    return ok


def main(write=True):
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF")
    if not ref:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        ref = re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    if not os.path.exists(os.path.join(ref, "src/phy/phch/pusch.c")):
        sys.exit(f"reference tree not found at {ref}")
    for c in TC.CASES:  # a valid TBS for each
        assert c["i_tbs"] < 0 or TC.tbs_of(c) > 0, c["name"]
    out, problems = {}, []
    measured = dict(d=0.0, grid=0.0)
    between = dict(d=0.0, grid=0.0)
    with tempfile.TemporaryDirectory() as tmp:
        Ls = [build(ref, os.path.join(tmp, "b1"), False), build(ref, os.path.join(tmp, "b2"), True)]
        objs = [{}, {}]
        for c in TC.CASES:
            name = c["name"]
            o = [transmit(L, ob, c) for L, ob in zip(Ls, objs)]
            for key in ("g", "q", "s"):
                if not np.array_equal(o[0][key], o[1][key]):
                    problems.append((name, key + " bits differ between the builds"))
            if not np.array_equal(o[0]["out"], o[1]["out"]):
                problems.append((name, "return values / write-back differ between the builds", o[0]["out"], o[1]["out"]))
            f = [f64_eval(c, x) for x in o]
            data, dm = TC.grant_mask(c, dict(nsym=PC.nsymb_slot(c["cp"]), M=12 * c["L"], rows=TC.data_rows(c)))
            for k in (0, 1):
                measured["d"] = max(measured["d"], float(np.abs(o[k]["d"] - f[k][0]).max() / np.abs(f[k][0]).max()))
                measured["grid"] = max(measured["grid"], PC.err("rms", o[k]["grid"][data], f[k][1][data]))
                if np.any(o[k]["grid"][~(data | dm)] != 0):
                    problems.append((name, "REs outside the grant are not zero", k))
                rex, bound = PC.dmrs_exact(dict(c, dmrs=[int(v) for v in c["dmrs"]]))
                if PC.err("abs", o[k]["r"], rex) > bound:
                    problems.append((name, "DMRS further from the exact one than the float formats explain", k))
            between["d"] = max(between["d"], float(np.abs(o[0]["d"] - f[1][0]).max() / np.abs(f[1][0]).max()))
            between["grid"] = max(between["grid"], PC.err("rms", o[0]["grid"][data], f[1][1][data]))
            if name in LOOP_CASES:
                for k in (0, 1):
                    key = c["payload_of"] or name
                    if not loop_check(Ls[k], objs[k][key], c, o[k], np.random.default_rng(4000 + c["seed"])):
                        problems.append((name, "the reference's receiver does not decode what was sent at %g dB" % SNR_DB, k))
            o1 = o[0]
            lo, hi = TC.columns(c)
            out["payload." + name] = o1["payload"]
            out["uci." + name] = np.frombuffer(bytes(o1["uci"]), np.uint8)
            out["out." + name] = o1["out"]
            out["g." + name], out["q." + name], out["s." + name] = o1["g"], o1["q"], o1["s"]
            out["dmrs." + name] = o1["r"]
            out["grid." + name] = np.ascontiguousarray(o1["grid"][:, lo:hi])
            if c["L"] <= 6:
                out["d." + name] = o1["d"]
        for L, ob in zip(Ls, objs):
            for q in ob.values():
                L.ph_free(q)
    for key in measured:
        if between[key] > measured[key] * 1.0000001 + 1e-12:
            problems.append((key, "the builds lie further apart than either lies from float64", between[key], measured[key]))
    for key, v in measured.items():  # four significant digits, rounded up: never below what was measured
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
        path = os.path.join(HERE, TC.FIXTURE)
        MG.write_npz(path, out)
        size = os.path.getsize(path)
        assert size <= MG.MAX_BYTES, size
        print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
