"""Generate tests/golden/phich_golden.npz from the reference's own PHICH transmitter and receiver.

Run where the reference tree exists (REF as in oracle/Makefile, the directory that holds include/ and src/):
    python tests/golden/make_phich_golden.py [REF]
With the flags of oracle/Makefile, that Makefile's REFSRC list plus phch/phich.c are compiled into a temporary
directory together with the small harness below (our own code: it only calls the reference's functions), an empty
stand-in srsran/version.h and a stub for srsran_phy_log_print.  The directory is removed afterwards; only arrays
and JSON of plain numbers are kept.

Per case of tests/phich_cases.py the file holds
  * re:      the PHICH RE table, 12 grid indices per mapping unit, read by walking srsran_regs_phich_get over a grid
             whose value at every RE is its index;
  * seq:     the 12 scrambling bits of the case's subframe (srsran_sequence_phich);
  * tx:      the reference's transmit grids after srsran_phich_encode of every item in put order on a cleared grid
             (ports x 3 symbols x 12 nof_prb: the PHICH lies in symbols 0..2, every other RE of the subframe is zero);
  * ce:      a 3-tap channel per (port, rx), evaluated exactly per subcarrier in float64, as the estimate;
  * rx0/rx1: the received grids, sum over ports of ce x tx, noise-free and with AWGN of variance `noise` (the value
             given to the decoder as the noise estimate; 0 for the noise-free one);
  * ref0/ref1: the reference's {ack_value, distance} for every queried resource (phich_cases.queries);
  * dev0/dev1: the largest |reference - float64| of `distance` over the case's queries, with the float64 evaluation
             of the same formulas on the recorded inputs (rx_f64 below);
  * invalid: srsran_phich_encode's and srsran_phich_decode's return values for the out-of-range resources;
  * calc:    srsran_phich_calc over n_prb_lowest 0 .. nof_prb - 1 x n_dmrs 0 .. 7 for the cases of phich_cases.CALC.
The generator fails unless the reference alone decodes every resource on which something was sent to the sent
value with |distance| >= 0.1, noise-free and with AWGN.  The AWGN starts at 10 dB SNR (relative to one unit-energy
symbol per RE) and the SNR is raised in 2 dB steps for a case that misses the margin; the SNR used is recorded.
"""
import concurrent.futures
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import phich_cases as C  # noqa: E402

EXTRA = ["src/phy/phch/phich.c"]
ROWS = 3
MARGIN = 0.1

STUBS = r'''
void srsran_phy_log_print(int level, const char* format, ...) {}
'''

HARNESS = r'''
#include <complex.h>
#include <stdlib.h>
#include <string.h>
#include "srsran/phy/phch/phich.h"
#include "srsran/phy/phch/regs.h"

static srsran_regs_t  regs;
static srsran_phich_t phich;
static srsran_cell_t  cell;
static int            is_open = 0;
static uint32_t       nrx     = 1;

void phich_ref_close(void)
{
  if (is_open) {
    srsran_phich_free(&phich);
    srsran_regs_free(&regs);
    is_open = 0;
  }
}

/* returns the reference's group count, or a negative value */
int phich_ref_open(uint32_t nof_prb, uint32_t ports, uint32_t id, int cp, int phich_len, int phich_res, int frame,
                   uint32_t mi, int sf1_6, uint32_t nof_rx)
{
  phich_ref_close();
  memset(&cell, 0, sizeof(cell));
  cell.nof_prb         = nof_prb;
  cell.nof_ports       = ports;
  cell.id              = id;
  cell.cp              = cp ? SRSRAN_CP_EXT : SRSRAN_CP_NORM;
  cell.phich_length    = phich_len ? SRSRAN_PHICH_EXT : SRSRAN_PHICH_NORM;
  cell.phich_resources = (srsran_phich_r_t)phich_res;
  cell.frame_type      = frame ? SRSRAN_TDD : SRSRAN_FDD;
  nrx                  = nof_rx;
  if (srsran_regs_init_opts(&regs, cell, mi, sf1_6 != 0)) {
    return -1;
  }
  if (srsran_phich_init(&phich, nof_rx) || srsran_phich_set_cell(&phich, &regs, cell)) {
    srsran_regs_free(&regs);
    return -2;
  }
  is_open = 1;
  return (int)srsran_phich_ngroups(&phich);
}

uint32_t phich_ref_ngroups_m1(void) { return srsran_regs_phich_ngroups_m1(&regs); }

/* 12 grid indices per mapping unit: srsran_regs_phich_get over a grid that holds its own indices */
int phich_ref_re_table(uint32_t* out, uint32_t sf_re)
{
  cf_t*    grid = malloc(sizeof(cf_t) * sf_re);
  cf_t     sym[SRSRAN_PHICH_MAX_NSYMB];
  uint32_t step = SRSRAN_CP_ISEXT(cell.cp) ? 2 : 1, n = 0;
  for (uint32_t i = 0; i < sf_re; i++) {
    grid[i] = (float)i;
  }
  for (uint32_t g = 0; g < srsran_phich_ngroups(&phich); g += step) {
    if (srsran_regs_phich_get(&regs, grid, sym, g) != SRSRAN_PHICH_MAX_NSYMB) {
      free(grid);
      return -1;
    }
    for (int e = 0; e < SRSRAN_PHICH_MAX_NSYMB; e++) {
      out[n++] = (uint32_t)crealf(sym[e]);
    }
  }
  free(grid);
  return (int)n;
}

void phich_ref_seq(uint32_t tti, float* out12)
{
  memcpy(out12, phich.seq[tti % 10].c_float, 12 * sizeof(float));
}

/* grids: ports x sf_re, contiguous */
int phich_ref_encode(uint32_t tti, uint32_t ngroup, uint32_t nseq, uint8_t ack, cf_t* grids, uint32_t sf_re)
{
  srsran_dl_sf_cfg_t      sf;
  srsran_phich_resource_t r = {ngroup, nseq};
  cf_t*                   p[SRSRAN_MAX_PORTS] = {NULL, NULL, NULL, NULL};
  memset(&sf, 0, sizeof(sf));
  sf.tti = tti;
  for (uint32_t i = 0; i < cell.nof_ports; i++) {
    p[i] = grids + (size_t)i * sf_re;
  }
  return srsran_phich_encode(&phich, &sf, r, ack, p);
}

/* grids: nrx x sf_re; ce: ports x nrx x sf_re */
int phich_ref_decode(uint32_t tti, uint32_t ngroup, uint32_t nseq, cf_t* grids, cf_t* ce, uint32_t sf_re, float noise,
                     float* distance, int* ack)
{
  srsran_dl_sf_cfg_t      sf;
  srsran_chest_dl_res_t   ch;
  srsran_phich_resource_t r = {ngroup, nseq};
  srsran_phich_res_t      res = {false, 0.0f};
  cf_t*                   y[SRSRAN_MAX_PORTS] = {NULL, NULL, NULL, NULL};
  memset(&sf, 0, sizeof(sf));
  memset(&ch, 0, sizeof(ch));
  sf.tti = tti;
  for (uint32_t j = 0; j < nrx; j++) {
    y[j] = grids + (size_t)j * sf_re;
    for (uint32_t i = 0; i < cell.nof_ports; i++) {
      ch.ce[i][j] = ce + ((size_t)i * nrx + j) * sf_re;
    }
  }
  ch.noise_estimate = noise;
  int ret = srsran_phich_decode(&phich, &sf, &ch, r, y, &res);
  *distance = res.distance;
  *ack      = res.ack_value ? 1 : 0;
  return ret;
}

void phich_ref_calc(uint32_t n_prb_lowest, uint32_t n_dmrs, uint32_t I_phich, uint32_t* ngroup, uint32_t* nseq)
{
  srsran_phich_grant_t    g = {n_prb_lowest, n_dmrs, I_phich};
  srsran_phich_resource_t r = {0, 0};
  srsran_phich_calc(&phich, &g, &r);
  *ngroup = r.ngroup;
  *nseq   = r.nseq;
}
'''


def build_reference(ref, d):
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read().replace("\\\n", " ")
    var = lambda n: re.search(r"^%s\s*:?=\s*(.*)$" % n, mk, flags=re.M).group(1)  # noqa: E731
    ldpc = var("LDPCSRC").split()
    refsrc = var("REFSRC").replace("$(addprefix src/phy/fec/ldpc/,$(LDPCSRC))",
                                   " ".join("src/phy/fec/ldpc/" + f for f in ldpc))
    oflags = var("OFLAGS").split()
    refflags = var("REFFLAGS").replace("$(OFLAGS)", " ".join(oflags)).split()
    nofast = [f for f in refflags if f != "-Ofast"] + ["-fno-trapping-math", "-fno-math-errno"]
    os.makedirs(os.path.join(d, "srsran"))
    open(os.path.join(d, "srsran", "version.h"), "w").write("/* stand-in for the generated header */\n")
    open(os.path.join(d, "stubs.c"), "w").write(STUBS)
    open(os.path.join(d, "harness.c"), "w").write(HARNESS)
    inc = ["-I", d, "-I", os.path.join(ref, "include")]
    jobs = []
    for src in refsrc.split() + EXTRA:
        jobs.append((os.path.join(ref, src), nofast if src.endswith("precoding.c") else refflags))
    jobs += [(os.path.join(d, "stubs.c"), refflags), (os.path.join(d, "harness.c"), refflags)]

    def cc(job):
        src, flags = job
        obj = os.path.join(d, os.path.basename(src)[:-2] + ".o")
        subprocess.run(["gcc"] + flags + inc + ["-c", src, "-o", obj], check=True)
        return obj

    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        objs = list(ex.map(cc, jobs))
    so = os.path.join(d, "libphichref.so")
    subprocess.run(["gcc", "-shared", "-Wl,-Bsymbolic", "-Wl,--unresolved-symbols=ignore-all", "-o", so] + objs +
                   ["-lm"], check=True)
    return ctypes.CDLL(so, mode=os.RTLD_LAZY)


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------ float64 evaluation of the receiver's formulas
W_NORM = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], np.complex128)
W_NORM = np.concatenate([W_NORM, 1j * W_NORM])
W_EXT = np.array([[1, 1], [1, -1], [1j, 1j], [1j, -1j]], np.complex128)


def rx_f64(c, re_tab, seq, rx, ce, noise, ngroup, nseq):
    """distance of srsran_phich_decode (phich.c:181-307) in float64 on the recorded float32 inputs.
    rx: (nrx, ROWS * nre), ce: (ports, nrx, ROWS * nre), seq: 12 values of +-1."""
    ext = c["cp"] == 1
    P, R = c["ports"], c["nrx"]
    idx = re_tab[ngroup // 2 if ext else ngroup]
    y = rx[:, idx].astype(np.complex128)
    h = ce[:, :, idx].astype(np.complex128)
    d0 = np.zeros(12, np.complex128)
    if P == 1:
        d0 = (y * np.conj(h[0])).sum(0) / ((np.abs(h[0]) ** 2).sum(0) + float(noise))
    elif P == 2:
        for i in range(6):
            hh = (np.abs(h[0, :, 2 * i]) ** 2 + np.abs(h[1, :, 2 * i + 1]) ** 2).sum()
            x0 = (np.conj(h[0, :, 2 * i]) * y[:, 2 * i] + h[1, :, 2 * i + 1] * np.conj(y[:, 2 * i + 1])).sum()
            x1 = (-h[1, :, 2 * i] * np.conj(y[:, 2 * i]) + np.conj(h[0, :, 2 * i + 1]) * y[:, 2 * i + 1]).sum()
            d0[2 * i], d0[2 * i + 1] = x0 / hh * np.sqrt(2.0), x1 / hh * np.sqrt(2.0)
    else:
        for i in range(3):
            h0, h1, h2, h3 = h[0, :, 4 * i], h[1, :, 4 * i + 2], h[2, :, 4 * i], h[3, :, 4 * i + 2]
            r0, r1, r2, r3 = (y[:, 4 * i + k] for k in range(4))
            hh02 = (np.abs(h0) ** 2 + np.abs(h2) ** 2).sum()
            hh13 = (np.abs(h1) ** 2 + np.abs(h3) ** 2).sum()
            d0[4 * i] = (np.conj(h0) * r0 + h2 * np.conj(r1)).sum() / hh02 * np.sqrt(2.0)
            d0[4 * i + 1] = (-h2 * np.conj(r0) + np.conj(h0) * r1).sum() / hh02 * np.sqrt(2.0)
            d0[4 * i + 2] = (np.conj(h1) * r2 + h3 * np.conj(r3)).sum() / hh13 * np.sqrt(2.0)
            d0[4 * i + 3] = (-h3 * np.conj(r2) + np.conj(h1) * r3).sum() / hh13 * np.sqrt(2.0)
    if ext:
        half = ngroup % 2
        d = np.array([d0[4 * (m // 2) + 2 * half + m % 2] for m in range(6)]) * seq[:6]
        z = (np.conj(W_EXT[nseq])[None, :] * d.reshape(3, 2)).sum(1) / 2
    else:
        d = d0 * seq
        z = (np.conj(W_NORM[nseq])[None, :] * d.reshape(3, 4)).sum(1) / 4
    llr = -(z.real + z.imag) / np.sqrt(2.0)
    return abs(llr.mean())


def channel(c, rng):
    """(ports, nrx, ROWS * nre) complex128: three taps per (port, rx), a dominant first one, constant in time"""
    nre = 12 * c["nof_prb"]
    k = np.arange(nre)
    H = np.zeros((c["ports"], c["nrx"], nre), np.complex128)
    for p in range(c["ports"]):
        for r in range(c["nrx"]):
            amp = np.array([1.0, 0.4, 0.2]) * np.exp(2j * np.pi * rng.random(3))
            delay = np.array([0.0, 1.0 + rng.random(), 3.0 + 2 * rng.random()])  # samples of a 128-point symbol
            H[p, r] = (amp[:, None] * np.exp(-2j * np.pi * delay[:, None] * k[None, :] / 128.0)).sum(0)
            H[p, r] /= np.sqrt((np.abs(amp) ** 2).sum())
    return np.tile(H, (1, 1, ROWS))


def open_case(L, c):
    n = L.phich_ref_open(c["nof_prb"], c["ports"], c["cell_id"], c["cp"], c["phich_len"], c["phich_res"], c["frame"],
                         c["mi"], int(c["sf1_6"]), c["nrx"])
    if n < 0:
        raise RuntimeError("reference refused case %s (%d)" % (c["name"], n))
    return n


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else None
    if ref is None:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        ref = re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        L = build_reference(ref, d)
        L.phich_ref_decode.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                                              ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
        L.phich_ref_encode.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint32]
        L.phich_ref_re_table.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.phich_ref_seq.argtypes = [ctypes.c_uint32, ctypes.c_void_p]
        L.phich_ref_calc.argtypes = [ctypes.c_uint32] * 3 + [ctypes.c_void_p, ctypes.c_void_p]
        L.phich_ref_ngroups_m1.restype = ctypes.c_uint32
        meta = []
        for ci, c in enumerate(C.CASES):
            name = c["name"]
            rng = np.random.default_rng(1000 + ci)
            ngroups = open_case(L, c)
            nre = 12 * c["nof_prb"]
            sf_re = 2 * (6 if c["cp"] else 7) * nre
            units = ngroups // 2 if c["cp"] else ngroups
            re_tab = np.zeros((max(units, 1), 12), np.uint32)
            assert L.phich_ref_re_table(ptr(re_tab), sf_re) == 12 * units
            re_tab = re_tab[:units]
            assert units == 0 or int(re_tab.max()) < ROWS * nre
            seq = np.zeros(12, np.float32)
            L.phich_ref_seq(c["tti"], ptr(seq))
            assert set(np.unique(seq)) <= {-1.0, 1.0}
            # transmit
            tx = np.zeros((c["ports"], sf_re), np.complex64)
            for g, s, a in c["items"]:
                assert L.phich_ref_encode(c["tti"], g, s, a, ptr(tx), sf_re) == 0
            assert not tx[:, ROWS * nre:].any()
            tx = tx[:, :ROWS * nre].copy()
            inv = []
            for g, s in c["invalid"]:
                t2 = np.zeros((c["ports"], sf_re), np.complex64)
                e = L.phich_ref_encode(c["tti"], g, s, 1, ptr(t2), sf_re)
                assert not t2.any()
                inv.append([g, s, e])
            # channel, received grids
            H = channel(c, rng)
            ce = H.astype(np.complex64)
            clean = (ce.astype(np.complex128) * tx.astype(np.complex128)[:, None, :]).sum(0)
            queries = C.queries(c)
            sent = {(g, s): a for g, s, a in c["items"]}
            assert len(sent) == len(c["items"])

            def decode(rx, noise):
                grid = np.zeros((c["nrx"], sf_re), np.complex64)
                grid[:, :ROWS * nre] = rx
                full = np.zeros((c["ports"], c["nrx"], sf_re), np.complex64)
                full[:, :, :ROWS * nre] = ce
                res, dev, ok = [], 0.0, True
                for g, s in queries:
                    dist, ack = ctypes.c_float(), ctypes.c_int()
                    assert L.phich_ref_decode(c["tti"], g, s, ptr(grid), ptr(full), sf_re, noise, ctypes.byref(dist),
                                              ctypes.byref(ack)) == 0
                    res.append([ack.value, dist.value])
                    dev = max(dev, abs(dist.value - rx_f64(c, re_tab, seq.astype(np.float64), rx, ce, noise, g, s)))
                    if (g, s) in sent and (ack.value != sent[(g, s)] or abs(dist.value) < MARGIN):
                        ok = False
                return np.array(res, np.float32).reshape(-1, 2), dev, ok

            rx0 = clean.astype(np.complex64)
            ref0, dev0, ok0 = decode(rx0, 0.0)
            if not ok0:
                raise SystemExit("%s: the reference misses the margin without noise" % name)
            w = (rng.standard_normal(clean.shape) + 1j * rng.standard_normal(clean.shape)) / np.sqrt(2.0)
            snr = 10.0
            while True:
                noise = float(np.float32(10.0 ** (-snr / 10.0)))
                rx1 = (clean + np.sqrt(noise) * w).astype(np.complex64)
                ref1, dev1, ok1 = decode(rx1, noise)
                if ok1:
                    break
                snr += 2.0
                if snr > 30.0:
                    raise SystemExit("%s: the reference misses the margin up to 30 dB SNR" % name)
            for i in inv:  # the receiver refuses them too
                grid = np.zeros((c["nrx"], sf_re), np.complex64)
                full = np.zeros((c["ports"], c["nrx"], sf_re), np.complex64)
                dist, ack = ctypes.c_float(), ctypes.c_int()
                i.append(L.phich_ref_decode(c["tti"], i[0], i[1], ptr(grid), ptr(full), sf_re, 0.0, ctypes.byref(dist),
                                            ctypes.byref(ack)))
            m = dict(c)
            m.update(ngroups=ngroups, ngroups_m1=int(L.phich_ref_ngroups_m1()), snr_db=snr, noise=noise,
                     dev0=float(dev0), dev1=float(dev1), queries=queries, invalid_ret=inv)
            meta.append(m)
            out[name + "/re"] = re_tab
            out[name + "/seq"] = (seq < 0).astype(np.uint8)
            out[name + "/tx"] = tx
            out[name + "/ce"] = ce
            out[name + "/rx0"] = rx0
            out[name + "/rx1"] = rx1
            out[name + "/ref0"] = ref0
            out[name + "/ref1"] = ref1
            print("%-18s groups %2d  snr %4.1f dB  dev %.2e / %.2e  min |distance| sent %.3f" % (
                name, ngroups, snr, dev0, dev1,
                min([abs(ref1[i, 1]) for i, q in enumerate(queries) if tuple(q) in sent] or [0.0])))
        calc = {}
        for name, iph in C.CALC:
            c = C.by_name(name)
            open_case(L, c)
            t = np.zeros((c["nof_prb"], 8, 2), np.uint32)
            for n in range(c["nof_prb"]):
                for dm in range(8):
                    g, s = ctypes.c_uint32(), ctypes.c_uint32()
                    L.phich_ref_calc(n, dm, iph, ctypes.byref(g), ctypes.byref(s))
                    t[n, dm] = g.value, s.value
            out[name + "/calc"] = t
            calc[name] = iph
        L.phich_ref_close()
    out["meta"] = np.frombuffer(json.dumps(dict(cases=meta, calc=calc, rows=ROWS)).encode(), np.uint8)
    path = os.path.join(HERE, "phich_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
