"""Generate tests/golden/pbch_golden.npz from the reference's own PBCH transmitter and receiver.

Run where the reference tree exists (REF as in oracle/Makefile, the directory that holds include/ and src/):
    python tests/golden/make_pbch_golden.py [REF]
oracle/Makefile's REFSRC list plus phch/pbch.c are compiled into a temporary directory together with the small harness
below (our own code: it only calls the reference's functions and reads its structs), an empty stand-in
srsran/version.h and a stub for srsran_phy_log_print; twice: with that Makefile's flags (build 1: AVX2, the 16-bit
Viterbi decoder) and with -O1 -ffp-contract=off and SSE only (build 2).  The directory is removed afterwards; only
arrays and JSON of plain numbers are kept.

A case of tests/pbch_cases.py is a sequence of calls on consecutive radio frames of one cell.  The transmit side is
srsran_pbch_encode of srsran_pbch_mib_pack(cell, sfn); every port goes through a 3-tap channel evaluated exactly in
float64, which is also the estimate (ports the cell does not have get small random estimates, as an estimator would
give: zero ones make the reference divide by zero), plus AWGN.  Per case the file holds
  * re:   the RE table read by walking srsran_pbch_get over a grid whose value at every RE is its index;
  * ce:   (decoder ports, 4, 72): slot 1's four symbols x 72 centre subcarriers of each port's estimate;
  * rx:   (calls, 4, 72): the same block of the received grid;
  * llr:  (calls, 2 nof_symbols): the frame each call stored in history slot frame_idx - 1 (the accepted port count's,
          or the last one tried).  The generator checks that the reference's whole history after every call is what
          pbch.c's bookkeeping makes of these frames (append, reset, shift after the fourth miss);
  * flags: (calls, 3, 30) int8: decode_frame's result for (port count 1 / 2 / 4, hypothesis in loop order of four
          stored frames), -1 where the hypothesis is not valid for the call, and `ran`: which of them the reference
          itself reached before it returned.  The hypotheses past its first success are run by the harness on the
          reference's own decode_frame; srsran_pbch_decode's results must be those of the first accepted one;
  * meta: per call ret, payload, nof_tx_ports, sfn_offset, frame_idx afterwards, noise estimate, sfn, seed.
Nothing is written unless
  (a) the two builds agree on every value above except the LLRs;
  (b) each build's LLRs lie within MEASURED (printed, stored) of the float64 evaluation of the same formulas (llr_f64);
  (c) every call returns what the case expects (noise-only calls: 0), for which a noise seed is searched;
  (d) no accept flag changes when build 1's LLRs are perturbed by random-sign errors of 10 x the LLR tolerance
      max(4 x MEASURED, 1e-6) x max |LLR| and decode_frame runs again;
  (e) the file stays within chest_cases.MAX_FIXTURE_BYTES.
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

import chest_cases  # noqa: E402
import pbch_cases as C  # noqa: E402

EXTRA = ["src/phy/phch/pbch.c"]
NSEED = 400
NANTS = (1, 2, 4)
FULL = [(nb, dst, src) for nb in range(4) for dst in range(4 - nb) for src in range(4 - nb)]

STUBS = r'''
void srsran_phy_log_print(int level, const char* format, ...) {}
'''

HARNESS = r'''
#include <complex.h>
#include <stdlib.h>
#include <string.h>
#include "srsran/phy/phch/pbch.h"
#include "srsran/phy/mimo/precoding.h"
#include "srsran/phy/mimo/layermap.h"
#include "srsran/phy/modem/demod_soft.h"

int decode_frame(srsran_pbch_t* q, uint32_t src, uint32_t dst, uint32_t n, uint32_t nof_bits, uint32_t nof_ports);

static srsran_pbch_t tx, rx, rx2; /* rx: srsran_pbch_decode itself; rx2: single steps on the reference's functions */
static srsran_cell_t cell;
static int           is_open = 0;

void pbch_ref_close(void)
{
  if (is_open) {
    srsran_pbch_free(&tx);
    srsran_pbch_free(&rx);
    srsran_pbch_free(&rx2);
    is_open = 0;
  }
}

int pbch_ref_open(uint32_t nof_prb, uint32_t ports, uint32_t id, int cp, int phich_len, int phich_res, int search)
{
  pbch_ref_close();
  memset(&cell, 0, sizeof(cell));
  cell.nof_prb         = nof_prb;
  cell.nof_ports       = ports;
  cell.id              = id;
  cell.cp              = cp ? SRSRAN_CP_EXT : SRSRAN_CP_NORM;
  cell.phich_length    = phich_len ? SRSRAN_PHICH_EXT : SRSRAN_PHICH_NORM;
  cell.phich_resources = (srsran_phich_r_t)phich_res;
  srsran_cell_t rc     = cell;
  if (search) {
    rc.nof_ports = 0;
  }
  if (srsran_pbch_init(&tx) || srsran_pbch_init(&rx) || srsran_pbch_init(&rx2) || srsran_pbch_set_cell(&tx, cell) ||
      srsran_pbch_set_cell(&rx, rc) || srsran_pbch_set_cell(&rx2, rc)) {
    return -1;
  }
  is_open = 1;
  return (int)rx.nof_symbols;
}

uint32_t pbch_ref_rx_ports(void) { return rx.cell.nof_ports; }

/* srsran_pbch_get over slot 1 of a grid that holds its own indices */
int pbch_ref_re_table(uint32_t* out, uint32_t sf_re)
{
  cf_t* grid = malloc(sizeof(cf_t) * sf_re);
  cf_t  sym[240];
  for (uint32_t i = 0; i < sf_re; i++) {
    grid[i] = (float)i;
  }
  int n = srsran_pbch_get(&grid[SRSRAN_SLOT_LEN_RE(cell.nof_prb, cell.cp)], sym, cell);
  for (int i = 0; i < n; i++) {
    out[i] = (uint32_t)crealf(sym[i]);
  }
  free(grid);
  return n;
}

/* grids: ports x sf_re, contiguous */
int pbch_ref_encode(uint32_t sfn, cf_t* grids, uint32_t sf_re, uint8_t* payload)
{
  cf_t* p[SRSRAN_MAX_PORTS] = {NULL, NULL, NULL, NULL};
  for (uint32_t i = 0; i < cell.nof_ports; i++) {
    p[i] = grids + (size_t)i * sf_re;
  }
  srsran_pbch_mib_pack(&cell, sfn, payload);
  return srsran_pbch_encode(&tx, payload, p, sfn);
}

static void channel(srsran_chest_dl_res_t* ch, cf_t* ce, uint32_t sf_re, float noise)
{
  memset(ch, 0, sizeof(*ch));
  for (uint32_t i = 0; i < SRSRAN_MAX_PORTS; i++) {
    ch->ce[i][0] = ce + (size_t)(i < rx.cell.nof_ports ? i : 0) * sf_re;
  }
  ch->noise_estimate = noise;
}

/* grid: sf_re; ce: decoder ports x sf_re; llr: 4 x nof_bits */
int pbch_ref_decode(cf_t* grid, cf_t* ce, uint32_t sf_re, float noise, uint8_t* payload, uint32_t* nports, int* off,
                    uint32_t* frame_idx, float* llr)
{
  srsran_chest_dl_res_t ch;
  cf_t*                 y[SRSRAN_MAX_PORTS] = {grid, NULL, NULL, NULL};
  channel(&ch, ce, sf_re, noise);
  int ret    = srsran_pbch_decode(&rx, &ch, y, payload, nports, off);
  *frame_idx = rx.frame_idx;
  memcpy(llr, rx.llr, sizeof(float) * 8 * rx.nof_symbols);
  return ret;
}

int pbch_ref_invalid(int which, cf_t* grid, cf_t* ce, uint32_t sf_re)
{
  srsran_chest_dl_res_t ch;
  cf_t*                 y[SRSRAN_MAX_PORTS] = {grid, NULL, NULL, NULL};
  uint8_t               pl[24];
  uint32_t              np;
  int                   off;
  channel(&ch, ce, sf_re, 0.0f);
  return which == 0 ? srsran_pbch_decode(NULL, &ch, y, pl, &np, &off) : srsran_pbch_decode(&rx, &ch, NULL, pl, &np, &off);
}

/* the equalised, demapped frame for one port-count hypothesis (pbch.c:456-511), on rx2 */
int pbch_ref_llr(cf_t* grid, cf_t* ce, uint32_t sf_re, float noise, uint32_t nant, float* out)
{
  srsran_pbch_t* q     = &rx2;
  uint32_t       slot  = SRSRAN_SLOT_LEN_RE(q->cell.nof_prb, q->cell.cp);
  cf_t*          x[SRSRAN_MAX_LAYERS];
  for (int i = 0; i < SRSRAN_MAX_PORTS; i++) {
    x[i] = q->x[i];
  }
  if (q->nof_symbols != srsran_pbch_get(&grid[slot], q->symbols[0], q->cell)) {
    return -1;
  }
  for (uint32_t i = 0; i < q->cell.nof_ports; i++) {
    if (q->nof_symbols != srsran_pbch_get(&ce[(size_t)i * sf_re + slot], q->ce[i], q->cell)) {
      return -1;
    }
  }
  if (nant == 1) {
    srsran_predecoding_single(q->symbols[0], q->ce[0], q->d, NULL, q->nof_symbols, 1.0f, noise);
  } else {
    srsran_predecoding_diversity(q->symbols[0], q->ce, x, nant, q->nof_symbols, 1.0f);
    srsran_layerdemap_diversity(x, q->d, nant, q->nof_symbols / nant);
  }
  srsran_demod_soft_demodulate(SRSRAN_MOD_QPSK, q->d, out, q->nof_symbols);
  return 0;
}

/* decode_frame on a given history (4 x nof_bits); bits: the 24 decoded payload bits */
int pbch_ref_hyp(const float* hist, uint32_t nant, uint32_t src, uint32_t dst, uint32_t n, uint8_t* bits)
{
  memcpy(rx2.llr, hist, sizeof(float) * 8 * rx2.nof_symbols);
  int ret = decode_frame(&rx2, src, dst, n, 2 * rx2.nof_symbols, nant);
  memcpy(bits, rx2.data, 24);
  return ret;
}
'''


def build_reference(ref, d, tag, second):
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read().replace("\\\n", " ")
    var = lambda n: re.search(r"^%s\s*:?=\s*(.*)$" % n, mk, flags=re.M).group(1)  # noqa: E731
    ldpc = var("LDPCSRC").split()
    refsrc = var("REFSRC").replace("$(addprefix src/phy/fec/ldpc/,$(LDPCSRC))",
                                   " ".join("src/phy/fec/ldpc/" + f for f in ldpc))
    oflags = var("OFLAGS").split()
    refflags = var("REFFLAGS").replace("$(OFLAGS)", " ".join(oflags)).split()
    nofast = [f for f in refflags if f != "-Ofast"] + ["-fno-trapping-math", "-fno-math-errno"]
    if second:
        refflags = nofast = ["-std=c99", "-D_GNU_SOURCE", "-O1", "-fPIC", "-fno-strict-aliasing", "-ffp-contract=off",
                             "-msse4.1", "-DLV_HAVE_SSE", "-w"]
    sub = os.path.join(d, tag)
    os.makedirs(os.path.join(sub, "srsran"))
    open(os.path.join(sub, "srsran", "version.h"), "w").write("/* stand-in for the generated header */\n")
    open(os.path.join(sub, "stubs.c"), "w").write(STUBS)
    open(os.path.join(sub, "harness.c"), "w").write(HARNESS)
    inc = ["-I", sub, "-I", os.path.join(ref, "include")]
    jobs = []
    for src in refsrc.split() + EXTRA:
        jobs.append((os.path.join(ref, src), nofast if src.endswith("precoding.c") else refflags))
    jobs += [(os.path.join(sub, "stubs.c"), refflags), (os.path.join(sub, "harness.c"), refflags)]

    def cc(job):
        src, flags = job
        obj = os.path.join(sub, os.path.basename(src)[:-2] + ".o")
        subprocess.run(["gcc"] + flags + inc + ["-c", src, "-o", obj], check=True)
        return obj

    with concurrent.futures.ThreadPoolExecutor(16) as ex:
        objs = list(ex.map(cc, jobs))
    so = os.path.join(sub, "libpbchref.so")
    subprocess.run(["gcc", "-shared", "-Wl,-Bsymbolic", "-Wl,--unresolved-symbols=ignore-all", "-o", so] + objs +
                   ["-lm"], check=True)
    L = ctypes.CDLL(so, mode=os.RTLD_LAZY)
    P, U = ctypes.c_void_p, ctypes.c_uint32
    L.pbch_ref_open.argtypes = [U, U, U] + [ctypes.c_int] * 4
    L.pbch_ref_rx_ports.restype = U
    L.pbch_ref_re_table.argtypes = [P, U]
    L.pbch_ref_encode.argtypes = [U, P, U, P]
    L.pbch_ref_decode.argtypes = [P, P, U, ctypes.c_float, P, P, P, P, P]
    L.pbch_ref_invalid.argtypes = [ctypes.c_int, P, P, U]
    L.pbch_ref_llr.argtypes = [P, P, U, ctypes.c_float, U, P]
    L.pbch_ref_hyp.argtypes = [P, U, U, U, U, P]
    return L


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def valid(fi, h):
    return h[0] < fi and h[2] < fi - h[0]


# ------------------------------------------------------------------ float64 evaluation of the receiver's formulas
def llr_f64(y, h, noise, nant):
    """pbch.c:497-511 in float64 on the recorded float32 inputs.  y: (nsym,), h: (ports, nsym) at the PBCH REs."""
    y = y.astype(np.complex128)
    h = h.astype(np.complex128)
    s2 = np.sqrt(2.0)
    if nant == 1:
        d = y * np.conj(h[0]) / (np.abs(h[0]) ** 2 + (float(noise) if noise > 0 else 0.0))
    elif nant == 2:
        r0, r1 = y[0::2], y[1::2]
        h00, h01, h10, h11 = h[0, 0::2], h[0, 1::2], h[1, 0::2], h[1, 1::2]
        hh = np.abs(h00) ** 2 + np.abs(h11) ** 2
        d = np.empty_like(y)
        d[0::2] = (np.conj(h00) * r0 + h11 * np.conj(r1)) / hh * s2
        d[1::2] = (-h10 * np.conj(r0) + np.conj(h01) * r1) / hh * s2
    else:
        r0, r1, r2, r3 = (y[k::4] for k in range(4))
        h0, h1, h2, h3 = h[0, 0::4], h[1, 2::4], h[2, 0::4], h[3, 2::4]
        hh02 = np.abs(h0) ** 2 + np.abs(h2) ** 2
        hh13 = np.abs(h1) ** 2 + np.abs(h3) ** 2
        d = np.empty_like(y)
        d[0::4] = (np.conj(h0) * r0 + h2 * np.conj(r1)) / hh02 * s2
        d[1::4] = (-h2 * np.conj(r0) + np.conj(h0) * r1) / hh02 * s2
        d[2::4] = (np.conj(h1) * r2 + h3 * np.conj(r3)) / hh13 * s2
        d[3::4] = (-h3 * np.conj(r2) + np.conj(h1) * r3) / hh13 * s2
    return np.stack([-s2 * d.real, -s2 * d.imag], 1).reshape(-1)


def channel(c, dec_ports, rng):
    """(dec_ports, 4, 72) complex128: three taps per real port, a dominant first one, constant in time; the ports
    the cell does not have: what an estimator would see there, small noise"""
    nre = 12 * c["nof_prb"]
    k = np.arange(nre // 2 - 36, nre // 2 + 36)
    H = np.zeros((dec_ports, 72), np.complex128)
    for p in range(dec_ports):
        if p < c["ports"]:
            amp = np.array([1.0, 0.4, 0.2]) * np.exp(2j * np.pi * rng.random(3))
            delay = np.array([0.0, 1.0 + rng.random(), 3.0 + 2 * rng.random()])  # samples of a 128-point symbol
            H[p] = (amp[:, None] * np.exp(-2j * np.pi * delay[:, None] * k[None, :] / 128.0)).sum(0)
            H[p] /= np.sqrt((np.abs(amp) ** 2).sum())
        else:
            H[p] = 0.05 * (rng.standard_normal(72) + 1j * rng.standard_normal(72))
    return np.tile(H[:, None, :], (1, 4, 1))


def block_index(c):
    """grid indices of slot 1's four symbols x 72 centre subcarriers"""
    nsymb, nre = (6 if c["cp"] else 7), 12 * c["nof_prb"]
    return ((nsymb + np.arange(4))[:, None] * nre + (nre // 2 - 36 + np.arange(72))[None, :]).reshape(-1)


def run_case(L, c, seed, ci):
    """all calls of case c with noise seed `seed` -> record, or None when a call does not return what the case
    expects"""
    nsym = L.pbch_ref_open(c["nof_prb"], c["ports"], c["cell_id"], c["cp"], c["phich_len"], c["phich_res"],
                           int(c["search"]))
    assert nsym == C.nof_symbols(c)
    nbits, dec_ports = 2 * nsym, int(L.pbch_ref_rx_ports())
    nsymb, nre = (6 if c["cp"] else 7), 12 * c["nof_prb"]
    sf_re = 2 * nsymb * nre
    re_tab = np.zeros(240, np.uint32)
    assert L.pbch_ref_re_table(ptr(re_tab), sf_re) == nsym
    re_tab = re_tab[:nsym]
    blk = block_index(c)
    pos = np.searchsorted(blk, re_tab)  # the PBCH REs within the block
    assert np.array_equal(blk[pos], re_tab)
    ce = channel(c, dec_ports, np.random.default_rng(5000 + ci)).astype(np.complex64).reshape(dec_ports, -1)
    ce_full = np.zeros((dec_ports, sf_re), np.complex64)
    ce_full[:, blk] = ce
    rng = np.random.default_rng(100000 * ci + seed)
    nants = NANTS if c["search"] else (c["ports"],)
    hist, fi = np.zeros((4, nbits), np.float32), 0
    rec = dict(re=re_tab, ce=ce.reshape(dec_ports, 4, 72), rx=[], llr=[], flags=[], ran=[], calls=[], hists=[], dev=0.0)
    for i, snr in enumerate(c["snr"]):
        sfn = (c["sfn0"] + i) % 1024
        w = (rng.standard_normal(4 * 72) + 1j * rng.standard_normal(4 * 72)) / np.sqrt(2.0)
        if snr is None:
            noise, clean = 1.0, np.zeros(4 * 72, np.complex128)
            sent = np.zeros(24, np.uint8)
        else:
            noise = float(np.float32(10.0 ** (-snr / 10.0)))
            tx = np.zeros((c["ports"], sf_re), np.complex64)
            sent = np.zeros(24, np.uint8)
            assert L.pbch_ref_encode(sfn, ptr(tx), sf_re, ptr(sent)) == 0
            clean = (ce[:c["ports"]].astype(np.complex128) * tx[:, blk].astype(np.complex128)).sum(0)
        rx = (clean + np.sqrt(noise) * w).astype(np.complex64)
        noise_est = 0.0 if c["zero_noise"] else noise
        grid = np.zeros(sf_re, np.complex64)
        grid[blk] = rx
        # the reference's own call
        pl, np_, off, fi_after = np.zeros(24, np.uint8), ctypes.c_uint32(0), ctypes.c_int(0), ctypes.c_uint32(0)
        ref_llr = np.zeros((4, nbits), np.float32)
        ret = L.pbch_ref_decode(ptr(grid), ptr(ce_full), sf_re, noise_est, ptr(pl), ctypes.byref(np_),
                                ctypes.byref(off), ctypes.byref(fi_after), ptr(ref_llr))
        if ret != c["expect"][i]:
            return None
        # every hypothesis, on the reference's own functions
        fi += 1
        flags = np.full((3, 30), -1, np.int8)
        ran = np.zeros((3, 30), np.uint8)
        first, hists, frames = None, {}, {}
        for nant in nants:
            a = NANTS.index(nant)
            f = np.zeros(nbits, np.float32)
            assert L.pbch_ref_llr(ptr(grid), ptr(ce_full), sf_re, noise_est, nant, ptr(f)) == 0
            want = llr_f64(rx[pos], ce[:, pos], noise_est, nant)
            if np.isfinite(f).all() and np.isfinite(want).all():
                rec["dev"] = max(rec["dev"], float(np.abs(f.astype(np.float64) - want).max() / np.abs(want).max()))
            else:
                return None
            h = hist.copy()
            h[fi - 1] = f
            hists[a], frames[a] = h, f
            for k, hyp in enumerate(FULL):
                if not valid(fi, hyp):
                    continue
                bits = np.zeros(24, np.uint8)
                r = L.pbch_ref_hyp(ptr(h), nant, hyp[2], hyp[1], hyp[0] + 1, ptr(bits))
                assert r in (0, 1)
                flags[a, k] = r
                if first is None:
                    ran[a, k] = 1
                    if r == 1:
                        first = (a, k, bits.copy())
        # srsran_pbch_decode must be the first accepted hypothesis, its history pbch.c's bookkeeping
        if first is None:
            assert ret == 0
            a_kept, exp_fi = NANTS.index(nants[-1]), (3 if fi == 4 else fi)
        else:
            a, k, bits = first
            nb, dst, src = FULL[k]
            assert ret == 1 and np.array_equal(pl, bits) and np_.value == NANTS[a] and off.value == dst - src + fi - 1
            if snr is not None and snr >= C.HI:
                assert np.array_equal(pl, sent) and NANTS[a] == c["ports"], "a clean frame decoded to something else"
            a_kept, exp_fi = a, 0
        hist[fi - 1] = frames[a_kept]
        stored, kept = frames[a_kept].copy(), fi
        if first is None and fi == 4:
            hist[:3] = hist[1:].copy()
            kept = 3
        assert np.array_equal(ref_llr[:kept], hist[:kept]), "history differs from the bookkeeping"
        assert fi_after.value == exp_fi
        fi = exp_fi
        rec["rx"].append(rx.reshape(4, 72))
        rec["llr"].append(stored)
        rec["flags"].append(flags)
        rec["ran"].append(ran)
        rec["hists"].append(hists)
        rec["calls"].append(dict(ret=int(ret), payload=[int(b) for b in pl] if ret == 1 else [0] * 24,
                                 nof_tx_ports=int(np_.value) if ret == 1 else 0,
                                 sfn_offset=int(off.value) if ret == 1 else 0, frame_idx=int(fi), noise=noise_est,
                                 sfn=sfn, sent=[int(b) for b in sent]))
    return rec


def same(a, b):
    return all(x == y for x, y in zip(a["calls"], b["calls"])) and \
        all(np.array_equal(x, y) for x, y in zip(a["flags"], b["flags"])) and \
        all(np.array_equal(x, y) for x, y in zip(a["ran"], b["ran"])) and np.array_equal(a["re"], b["re"])


def margin_ok(L, c, rec, tol, ci):
    """condition (d) on build 1"""
    L.pbch_ref_open(c["nof_prb"], c["ports"], c["cell_id"], c["cp"], c["phich_len"], c["phich_res"], int(c["search"]))
    rng = np.random.default_rng(777 + ci)
    for i in range(len(rec["calls"])):
        for a, h in rec["hists"][i].items():
            for trial in range(2):
                eps = 10.0 * tol * np.abs(h).max(1, keepdims=True)
                hp = (h + eps * rng.choice([-1.0, 1.0], h.shape)).astype(np.float32)
                for k, hyp in enumerate(FULL):
                    if rec["flags"][i][a, k] < 0:
                        continue
                    bits = np.zeros(24, np.uint8)
                    if L.pbch_ref_hyp(ptr(hp), NANTS[a], hyp[2], hyp[1], hyp[0] + 1, ptr(bits)) != rec["flags"][i][a, k]:
                        return False
    return True


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else None
    if ref is None:
        mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
        ref = re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    out, meta, recs = {}, [], []
    with tempfile.TemporaryDirectory() as d:
        L1 = build_reference(ref, d, "b1", False)
        L2 = build_reference(ref, d, "b2", True)
        # pass 1: a seed per case with which both builds do what the case expects and agree; MEASURED over them
        for ci, c in enumerate(C.CASES):
            for seed in range(NSEED):
                r1 = run_case(L1, c, seed, ci)
                if r1 is None:
                    continue
                r2 = run_case(L2, c, seed, ci)
                if r2 is not None and same(r1, r2):
                    break
            else:
                raise SystemExit("%s: no noise seed below %d gives the expected returns in both builds" % (c["name"], NSEED))
            recs.append([seed, r1, r2])
            print("%-20s seed %d" % (c["name"], seed), flush=True)
        # pass 2: the margin condition at the tolerance MEASURED implies; a case that misses it looks for another seed
        while True:
            measured = max(max(r1["dev"], r2["dev"]) for _, r1, r2 in recs)
            tol = max(4 * measured, 1e-6)
            redo = [ci for ci, (s, r1, r2) in enumerate(recs) if not margin_ok(L1, C.CASES[ci], r1, tol, ci)]
            if not redo:
                break
            for ci in redo:
                c = C.CASES[ci]
                for seed in range(recs[ci][0] + 1, NSEED):
                    r1 = run_case(L1, c, seed, ci)
                    if r1 is None:
                        continue
                    r2 = run_case(L2, c, seed, ci)
                    if r2 is not None and same(r1, r2):
                        break
                else:
                    raise SystemExit("%s: no noise seed below %d meets the margin condition" % (c["name"], NSEED))
                recs[ci] = [seed, r1, r2]
        # invalid inputs
        c = C.CASES[0]
        L1.pbch_ref_open(c["nof_prb"], c["ports"], c["cell_id"], c["cp"], c["phich_len"], c["phich_res"], 0)
        sf_re = 14 * 12 * c["nof_prb"]
        g, e = np.zeros(sf_re, np.complex64), np.zeros((4, sf_re), np.complex64)
        invalid = [int(L1.pbch_ref_invalid(w, ptr(g), ptr(e), sf_re)) for w in (0, 1)]
        L1.pbch_ref_close()
        L2.pbch_ref_close()
    for c, (seed, r1, r2) in zip(C.CASES, recs):
        name = c["name"]
        m = dict(c)
        m.update(seed=seed, calls=r1["calls"], dev1=r1["dev"], dev2=r2["dev"])
        meta.append(m)
        out[name + "/re"] = r1["re"]
        out[name + "/ce"] = r1["ce"]
        out[name + "/rx"] = np.stack(r1["rx"])
        out[name + "/llr"] = np.stack(r1["llr"])
        out[name + "/flags"] = np.stack(r1["flags"])
        out[name + "/ran"] = np.stack(r1["ran"])
        print("%-20s seed %3d  returns %s  frame_idx %s  dev %.2e / %.2e" % (
            name, seed, [k["ret"] for k in r1["calls"]], [k["frame_idx"] for k in r1["calls"]], r1["dev"], r2["dev"]))
    print("MEASURED = %r   (LLR tolerance %.3e)" % (measured, tol))
    out["meta"] = np.frombuffer(json.dumps(dict(cases=meta, measured=measured, invalid=invalid)).encode(), np.uint8)
    path = os.path.join(HERE, C.FIXTURE)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    if size > chest_cases.MAX_FIXTURE_BYTES:
        os.remove(path)
        raise SystemExit("fixture larger than %d bytes" % chest_cases.MAX_FIXTURE_BYTES)


if __name__ == "__main__":
    main()
