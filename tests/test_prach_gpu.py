"""PRACH on the GPU against tests/prach_np.py, the float64 numpy restatement of the reference's prach.c (its detector
needs FFTW and cannot be compiled here): sequences, generation for formats 0-3, the reference's own gen -> detect
loop over all 64 preambles, detection of one to three delayed preambles in noise (indices, offsets, peak / average
ratios, the full metrics table), frequency-domain offsets, indices above 63, the batch call and the refusals.

Ratio tolerance: the restatement is also evaluated in complex64 / float32 on the same inputs; the GPU may deviate
from the float64 ratios by 8 x the largest deviation of that evaluation, both relative to the root's largest ratio
(4 x is the project's convention; doubled because the 839-point inverse is a direct sum here).  Each case prints its
figures before it asserts."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import prach_np as R
from srsran_4g_amd import prach as P
from srsran_4g_amd import tdec
from srsran_4g_amd import ue_dl as U

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not tdec.gpu_available(), reason="needs a HIP device")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ZC = 839
SYMBOL_SZ = {6: 128, 25: 384, 100: 1536}  # the library default (the reference's 3/4 rates); standard: 100 -> 2048


class Cell:
    """a configured srsran_prach_t and the restatement's parameters for the same configuration"""

    def __init__(self, nof_prb, config_idx, rsi, zczc, standard=False, fdo=False, num_ra=0):
        self.nof_prb, self.standard = nof_prb, standard
        U.use_standard_symbol_size(standard)
        try:
            self.N = U.symbol_sz_for(nof_prb)
            self.p = P.Prach(2048).configure(P.cfg(config_idx, rsi, zczc, num_ra, freq_domain_offset=fdo), nof_prb)
        finally:
            U.use_standard_symbol_size(False)
        self.ref = R.Params(self.N, config_idx, rsi, zczc, num_ra, standard=standard)
        self.fdo = fdo

    def call(self, f, *a):
        """f(*a) under this cell's symbol-size convention (srsran_nof_prb is read at every gen / detect)"""
        U.use_standard_symbol_size(self.standard)
        try:
            return f(*a)
        finally:
            U.use_standard_symbol_size(False)

    def free(self):
        self.p.free()


@pytest.fixture(scope="module")
def cells():
    made = {}

    def get(*key, **kw):
        k = (key, tuple(sorted(kw.items())))
        if k not in made:
            made[k] = Cell(*key, **kw)
        return made[k]

    yield get
    for c in made.values():
        c.free()


# ---------------------------------------------------------------- sequences
@pytest.mark.parametrize("zczc", [0, 1, 5, 11, 15])
@pytest.mark.parametrize("rsi", [0, 22, 837])
def test_sequences(cells, zczc, rsi):
    c = cells(6, 0, rsi, zczc)
    q, ref = c.p.q, c.ref
    assert q.N_cs == ref.N_cs and q.N_roots == ref.N_roots and q.N_zc == N_ZC
    assert list(q.root_seqs_idx[:q.N_roots]) == ref.root_seqs_idx
    assert q.num_ra_preambles == ref.num_ra_preambles
    seqs = c.p.seqs
    assert np.abs(seqs - ref.seqs).max() < 1e-6  # float32 of an exact table
    assert np.abs(np.abs(seqs) - 1).max() < 1e-6
    for i in (0, 1, 63):  # ideal cyclic autocorrelation: a single peak of 839
        s = seqs[i].astype(np.complex128)
        ac = np.fft.ifft(np.fft.fft(s) * np.conj(np.fft.fft(s)))
        assert abs(ac[0] - N_ZC) < 1e-3 and np.abs(ac[1:]).max() < 1e-3


# ---------------------------------------------------------------- generation
@pytest.mark.parametrize("nof_prb,config_idx,standard", [(6, 0, False), (6, 16, False), (25, 32, False), (6, 63, False),
                                                         (100, 0, False), (100, 35, True)])
def test_gen_matches_restatement(cells, nof_prb, config_idx, standard):
    c = cells(nof_prb, config_idx, 22, 5, standard=standard)
    q, ref = c.p.q, c.ref
    assert (q.N_cp, q.N_seq, q.N_ifft_prach) == (ref.N_cp, ref.N_seq, ref.M)
    M = ref.M
    fo = 0 if nof_prb == 6 else nof_prb - 6
    for seq in (0, 37, 63):
        ret, x = c.call(c.p.gen, seq, fo)
        assert ret == 0
        want = R.gen(ref, seq, fo)
        err = np.abs(x - want).max() / np.abs(want).max()
        print(f"gen {nof_prb} PRB N={c.N} config {config_idx} seq {seq}: max err / max|x| = {err:.3g}")
        assert err < 1e-6
        assert np.array_equal(x[:q.N_cp], x[q.N_cp + M - q.N_cp:q.N_cp + M])  # the CP is the tail
        if config_idx // 16 >= 2:
            assert q.N_seq == 2 * M and np.array_equal(x[q.N_cp:q.N_cp + M], x[q.N_cp + M:])
    # device output = host output
    d = torch.zeros(2 * (q.N_cp + q.N_seq), dtype=torch.float32, device="cuda")
    assert c.call(c.p.gpu_gen, 63, fo, d.data_ptr()) == 0
    assert np.array_equal(d.cpu().numpy().view(np.complex64), x)
    assert c.call(c.p.gen, 64, fo)[0] == P.SRSRAN_ERROR  # seq_index out of range
    assert c.call(c.p.gen, 0, nof_prb - 5)[0] == P.SRSRAN_ERROR  # no space for 6 PRB


# ---------------------------------------------------------------- the reference's prach_test.c
@pytest.mark.parametrize("nof_prb,zczc", [(6, 15), (6, 1), (6, 0), (25, 11)])
def test_gen_detect_all_64(cells, nof_prb, zczc):
    c = cells(nof_prb, 0, 0, zczc)
    q = c.p.q
    c.p.set_detect_factor(18)
    for seq in range(64):
        ret, x = c.p.gen(seq, 0)
        assert ret == 0
        ret, idx = c.p.detect(0, x[q.N_cp:])
        assert ret == 0 and idx == [seq], (seq, idx)


# ---------------------------------------------------------------- detection against the restatement
FACTOR = 60.0  # srsENB's
# name: (nof_prb, config_idx, rsi, zczc, standard, freq_offset, [(seq, amplitude, delay in samples)], noise seed)
DETECT_CASES = {
    "6prb_z1_three": (6, 0, 0, 1, False, 0, [(3, 1.0, 0), (40, 0.6, 4), (63, 0.8, 9)], 1),
    "6prb_z15_two": (6, 0, 22, 15, False, 0, [(10, 1.0, 5), (11, 0.7, 0)], 2),
    "25prb_z5_two": (25, 16, 837, 5, False, 2, [(17, 1.0, 7), (50, 0.5, 0)], 3),
    "100prb_1536_z11_three": (100, 0, 22, 11, False, 4, [(12, 1.0, 15), (30, 0.6, 40), (63, 0.8, 0)], 4),
    "100prb_2048_z1_one": (100, 0, 0, 1, True, 10, [(5, 1.0, 30)], 5),
}


def check_against_restatement(c, fo, x, factor, name):
    """one detect on the GPU and in numpy (float64 and float32); returns the float64 result"""
    ref = c.ref
    want = R.detect(ref, fo, x, factor, c.fdo)
    single = R.detect(ref, fo, x, factor, c.fdo, single=True)
    c.p.set_detect_factor(factor)
    ret, idx, toff, p2a = c.call(c.p.detect_offset, fo, x)
    assert ret == 0
    ratio, offset = c.p.metrics()
    top = want["ratio"].max(axis=1, keepdims=True)
    dev32 = (np.abs(single["ratio"] - want["ratio"]) / top).max()
    bound = 8 * dev32
    dev = (np.abs(ratio - want["ratio"]) / top).max()
    det = want["ratio"] > factor
    print(f"{name}: indices {list(want['indices'])}; float32 restatement deviates {dev32:.3g}, bound {bound:.3g}, "
          f"GPU deviates {dev:.3g}; hits >= {want['ratio'][det].min() if det.any() else None}, "
          f"misses <= {want['ratio'][~det].max() if (~det).any() else None}, "
          f"second / peak <= {want['second'][det].max() if det.any() else None}")
    assert np.array_equal(idx, want["indices"])
    assert toff.tobytes() == want["t_offsets"].tobytes()
    assert ratio.shape == want["ratio"].shape
    assert dev <= bound
    top_det = np.repeat(top, ref.n_wins, axis=1)[det]
    assert (np.abs(p2a - want["peak_to_avg"]) / top_det <= bound).all()
    assert np.array_equal(offset[det], want["offset"][det])
    return want


@pytest.mark.parametrize("name", list(DETECT_CASES))
def test_detect_matches_restatement(cells, name):
    nof_prb, config_idx, rsi, zczc, standard, fo, pre, seed = DETECT_CASES[name]
    c = cells(nof_prb, config_idx, rsi, zczc, standard=standard)
    x = R.channel(c.ref, pre, fo, -10.0, seed)
    want = check_against_restatement(c, fo, x, FACTOR, name)
    # conditions on the restatement itself: nothing near the threshold, no near-tie inside a detected window
    r, det = want["ratio"], want["ratio"] > FACTOR
    assert not ((r >= FACTOR / 1.5) & (r <= FACTOR * 1.5)).any()
    assert (want["second"][det] <= 0.99).all()
    assert sorted(want["indices"]) == sorted(p[0] for p in pre)


# ---------------------------------------------------------------- frequency-domain offsets
# name: (nof_prb, rsi, standard, freq_offset, [(seq, amplitude, delay)], seed); zero_corr_zone 0: a root per preamble
FDO_CASES = {
    "6prb": (6, 0, False, 0, [(3, 1.0, 4)], 6),
    "25prb": (25, 22, False, 5, [(7, 1.0, 11)], 8),
    "100prb_2048": (100, 5, True, 10, [(33, 1.0, 50)], 7),
}


@pytest.mark.parametrize("name", list(FDO_CASES))
def test_freq_domain_offsets(cells, name):
    nof_prb, rsi, standard, fo, pre, seed = FDO_CASES[name]
    c = cells(nof_prb, 0, rsi, 0, standard=standard, fdo=True)
    assert c.p.q.freq_domain_offset_calc and c.p.q.N_roots == 64
    x = R.channel(c.ref, pre, fo, -10.0, seed)
    want = check_against_restatement(c, fo, x, FACTOR, "fdo " + name)
    assert list(want["indices"]) == sorted(p[0] for p in pre)
    srate = c.N * 15000
    for seq, _, delay in pre:
        est = want["est_samples"][seq]  # zero_corr_zone 0: root i is preamble i
        assert abs(est - np.round(est)) < 0.45  # more than 0.05 from a rounding boundary
        t = want["t_offsets"][list(want["indices"]).index(seq)]
        print(f"fdo {name}: preamble {seq} delayed {delay}, estimate {est:.3f} samples")
        assert abs(t * srate - delay) <= srate / 1048750  # prach_test_multi.c:248-249


# ---------------------------------------------------------------- indices above 63
def test_index_above_63(cells):
    """zero_corr_zone 11: 9 windows x 8 roots.  Preamble 63 (root 7, window 0) delayed by 15 samples leaks below the
    start of its window, i.e. into window 1 of root 7, index 64; with factor 18 the reference reports it."""
    c = cells(100, 0, 22, 11)
    assert c.p.q.N_roots == 8 and c.ref.n_wins == 9
    x = R.channel(c.ref, [(63, 1.0, 15)], 4, -10.0, 9)
    want = check_against_restatement(c, 4, x, 18.0, "index >= 64")
    assert 63 in want["indices"] and 64 in want["indices"]  # the input was chosen so


# ---------------------------------------------------------------- batch
def test_batch_equals_singles_in_any_order(cells):
    a, b = cells(6, 0, 0, 1), cells(25, 16, 837, 5)
    a2 = cells(6, 0, 22, 15)
    items = []
    for k in range(8):
        c = (a, b, a2, b)[k % 4]
        pre = [((7 * k + 3) % 64, 1.0, k % 5), ((11 * k + 30) % 64, 0.7, (2 * k) % 7)]
        fo = 2 + k % 3 if c is b else 0
        items.append((c, fo, R.channel(c.ref, pre, fo, -10.0, 20 + k)))
    for c in (a, b, a2):
        c.p.set_detect_factor(FACTOR)
    singles = []
    for c, fo, x in items:
        ret, idx, toff, p2a = c.p.detect_offset(fo, x)
        assert ret == 0 and len(idx) >= 1
        singles.append((idx, toff, p2a) + c.p.metrics())
    dev = [torch.from_numpy(x.view(np.float32)).cuda() for _, _, x in items]
    for order in (list(range(8)), list(range(7, -1, -1)), [3, 0, 6, 1, 7, 4, 2, 5]):
        ret, res, _ = P.detect_batch([(items[i][0].p, items[i][1], dev[i].data_ptr(), len(items[i][2])) for i in order])
        assert ret == 0
        for slot, i in enumerate(order):
            for got, want in zip(res[slot], singles[i][:3]):
                assert got.tobytes() == want.tobytes(), (order, i)
        # the metrics an object keeps are those of its last entry in the batch
        last = {}
        for i in order:
            last[id(items[i][0])] = i
        for i in last.values():
            r, o = items[i][0].p.metrics()
            assert r.tobytes() == singles[i][3].tobytes() and np.array_equal(o, singles[i][4])


def test_batch_workspace_regrowth_is_bit_identical():
    """One object as a batch's first: one occasion, twenty (above the 16-occasion floor, so the pinned and device
    workspace is reallocated), one again -- results equal a fresh object's bit for bit."""
    a = Cell(6, 0, 0, 1)
    x = [R.channel(a.ref, [((7 * k + 3) % 64, 1.0, k % 5)], 0, -10.0, 40 + k) for k in range(20)]
    dev = [torch.from_numpy(v.view(np.float32)).cuda() for v in x]
    a.p.set_detect_factor(FACTOR)
    try:
        for n in (1, 20, 1):
            fresh = Cell(6, 0, 0, 1)
            fresh.p.set_detect_factor(FACTOR)
            try:
                ret, want, _ = P.detect_batch([(fresh.p, 0, dev[i].data_ptr(), len(x[i])) for i in range(n)])
                assert ret == 0
            finally:
                fresh.free()
            ret, got, _ = P.detect_batch([(a.p, 0, dev[i].data_ptr(), len(x[i])) for i in range(n)])
            assert ret == 0 and len(got) == n
            for g, w in zip(got, want):
                assert len(g[0]) >= 1 and all(u.tobytes() == v.tobytes() for u, v in zip(g, w)), n
    finally:
        a.free()


def test_batch_refuses_a_short_entry_and_writes_nothing(cells):
    a, b = cells(6, 0, 0, 1), cells(25, 16, 837, 5)
    xa = torch.from_numpy(R.channel(a.ref, [(3, 1.0, 0)], 0, -10.0, 1).view(np.float32)).cuda()
    xb = torch.from_numpy(R.channel(b.ref, [(3, 1.0, 0)], 2, -10.0, 1).view(np.float32)).cuda()
    entries = [(a.p, 0, xa.data_ptr(), a.ref.M), (b.p, 2, xb.data_ptr(), b.ref.M - 1), (a.p, 0, xa.data_ptr(), a.ref.M)]
    n = len(entries)
    occ = (P.srsran_prach_gpu_occ_t * n)()
    res = (P.srsran_prach_gpu_res_t * n)()
    ctypes.memset(res, 0xA5, ctypes.sizeof(res))
    for i, (p, fo, dptr, sig_len) in enumerate(entries):
        occ[i].prach, occ[i].freq_offset, occ[i].d_signal, occ[i].sig_len = ctypes.pointer(p.q), fo, dptr, sig_len
    assert P.lib().srsran_prach_gpu_detect_batch(n, occ, res) == P.SRSRAN_ERROR_INVALID_INPUTS
    assert bytes(res) == b"\xa5" * ctypes.sizeof(res)
    # the host call returns the same code
    ret = b.p.detect(2, np.zeros(b.ref.M - 1, dtype=np.complex64))[0]
    assert ret == P.SRSRAN_ERROR_INVALID_INPUTS


# ---------------------------------------------------------------- refusals
def test_refusals():
    p = P.Prach(2048)
    try:
        assert p.set_cfg(P.cfg(48, 0, 1, tdd=True), 6) == P.SRSRAN_ERROR  # format 4 (36.211 Table 5.7.1-3)
        assert p.set_cfg(P.cfg(48, 0, 1), 6) == P.SRSRAN_SUCCESS and p.q.f == 3  # FDD: format 3
        assert p.set_cfg(P.cfg(0, 0, 1, hs_flag=True), 6) == P.SRSRAN_ERROR
        assert p.set_cfg(P.cfg(0, 0, 0, cancellation=True), 6) == P.SRSRAN_ERROR
        assert p.set_cfg(P.cfg(0, 0, 5, cancellation=True), 6) == P.SRSRAN_SUCCESS
        assert not p.q.successive_cancellation
        assert p.set_cfg(P.cfg(0, 838, 1), 6) == P.SRSRAN_ERROR  # root_seq_idx out of range
        assert p.set_cfg(P.cfg(0, 0, 16), 6) == P.SRSRAN_ERROR
        # num_ra_preambles: below 4 or above N_roots becomes N_roots; the search runs over that many roots
        assert p.set_cfg(P.cfg(0, 0, 0, num_ra_preambles=16), 6) == 0 and p.q.num_ra_preambles == 16
        assert p.set_cfg(P.cfg(0, 0, 11, num_ra_preambles=52), 6) == 0 and p.q.num_ra_preambles == p.q.N_roots == 8
        small = P.Prach(128)
        try:
            assert small.set_cfg(P.cfg(0, 0, 1), 25) == P.SRSRAN_ERROR  # above max_N_ifft_ul
        finally:
            small.free()
    finally:
        p.free()


def test_num_ra_preambles_limits_the_search(cells):
    c = cells(6, 0, 0, 0, num_ra=16)
    assert c.p.q.num_ra_preambles == 16
    c.p.set_detect_factor(18)
    x = R.channel(c.ref, [(5, 1.0, 0), (40, 1.0, 0)], 0, None, 0)
    ret, idx = c.p.detect(0, x)
    assert ret == 0 and idx == [5]  # root 40 is not searched
    assert c.p.metrics()[0].shape == (16, 1)


def test_detect_time_hook(cells):
    """the event pair on the object's stream: off by default, a positive time once enabled, results unchanged"""
    c = cells(6, 0, 0, 1)
    c.p.set_detect_factor(FACTOR)
    x = R.channel(c.ref, [(3, 1.0, 0)], 0, -10.0, 1)
    assert c.p.detect_time(False) == -1.0
    plain = c.p.detect_offset(0, x)
    assert c.p.detect_time(True) == -1.0  # the detect above was not timed
    timed = c.p.detect_offset(0, x)
    us = c.p.detect_time(False)
    print(f"detect_time: {us:.1f} us for one 6-PRB occasion, one root")
    assert 0 < us < 1e5
    assert all(np.array_equal(a, b) for a, b in zip(plain[1:], timed[1:]))


# ---------------------------------------------------------------- a C99 caller
C_CALLER = r'''
/* as the reference's prach_test.c: init, set_cfg, 64 x gen / detect, free */
#include "srsran_prach.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(void)
{
  srsran_prach_t     prach;
  srsran_prach_cfg_t cfg;
  uint32_t           nof_prb = 6, indices[SRSRAN_PRACH_GPU_MAX_DET], n_indices = 0;
  float              offsets[SRSRAN_PRACH_GPU_MAX_DET], p2avg[SRSRAN_PRACH_GPU_MAX_DET];
  cf_t*              preamble = malloc(sizeof(cf_t) * SRSRAN_PRACH_MAX_LEN);
  memset(&cfg, 0, sizeof(cfg));
  cfg.config_idx     = 0;
  cfg.root_seq_idx   = 0;
  cfg.zero_corr_zone = 11;
  if (srsran_prach_init(&prach, (uint32_t)srsran_symbol_sz(nof_prb))) {
    return 1;
  }
  if (srsran_prach_set_cfg(&prach, &cfg, nof_prb)) {
    return 2;
  }
  if (prach.N_zc != SRSRAN_PRACH_N_ZC_LONG || prach.N_ifft_prach != 1536 || prach.detect_factor != 18.0f) {
    return 3;
  }
  for (uint32_t seq = 0; seq < 64; seq++) {
    if (srsran_prach_gen(&prach, seq, 0, preamble)) {
      return 4;
    }
    if (srsran_prach_detect(&prach, 0, &preamble[prach.N_cp], prach.N_seq, indices, &n_indices)) {
      return 5;
    }
    if (n_indices != 1 || indices[0] != seq) {
      printf("seq %u: %u detected, first %u\n", seq, n_indices, indices[0]);
      return 6;
    }
    if (srsran_prach_detect_offset(&prach, 0, &preamble[prach.N_cp], prach.N_seq, indices, offsets, p2avg,
                                   &n_indices) || n_indices != 1 || offsets[0] != 0.0f || p2avg[0] < 800.0f) {
      return 7;
    }
  }
  if (srsran_prach_detect(&prach, 0, preamble, prach.N_ifft_prach - 1, indices, &n_indices) !=
      SRSRAN_ERROR_INVALID_INPUTS) {
    return 8;
  }
  srsran_prach_free(&prach);
  free(preamble);
  printf("%zu\n", sizeof(srsran_prach_t));
  return 0;
}
'''


def test_c99_caller_like_prach_test():
    libdir = os.path.dirname(tdec.LIB_PATH)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "prach.c"), os.path.join(d, "prach")
        open(src, "w").write(C_CALLER)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                            "-L", libdir, "-lsrsran_4g_amd", "-Wl,-rpath," + libdir, "-lm"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
        assert int(r.stdout.split()[-1]) == ctypes.sizeof(P.srsran_prach_t)
