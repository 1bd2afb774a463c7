"""PBCH / MIB decode on the GPU against fixtures recorded from the compiled reference (tests/golden/make_pbch_golden.py).

Everything discrete is compared for equality (return, payload, port count, sfn_offset, frame_idx, every hypothesis'
accept flag and so the index of the accepted one); the LLR history as max |got - want| / max |want| against
pbch_cases.LLR_TOL = max(4 x MEASURED, 1e-6), MEASURED being the reference builds' own distance from a float64
evaluation (2.9e-7).  The generator's margin condition keeps every recorded flag away from a decision that an LLR error
of ten times that tolerance could flip."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import pbch_cases as C
from srsran_4g_amd import enb_dl as E
from srsran_4g_amd import pbch as B
from srsran_4g_amd import tdec
from srsran_4g_amd import ue_dl as U

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NANTS = (1, 2, 4)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", C.FIXTURE))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, {m["name"]: m for m in meta["cases"]}, meta


def geometry(c):
    nsymb, nre = (6 if c["cp"] else 7), 12 * c["nof_prb"]
    blk = ((nsymb + np.arange(4))[:, None] * nre + (nre // 2 - 36 + np.arange(72))[None, :]).reshape(-1)
    return nsymb, nre, 2 * nsymb * nre, blk


def cell_of(c):
    return U.cell(c["nof_prb"], 0 if c["search"] else c["ports"], c["cell_id"], phich_res=c["phich_res"], cp=c["cp"],
                  phich_len=c["phich_len"])


def expand(c, z):
    """the stored blocks as full grids: (calls, sf_re) received, (decoder ports, sf_re) estimates"""
    _, _, sf_re, blk = geometry(c)
    rx, ce = z[c["name"] + "/rx"], z[c["name"] + "/ce"]
    grids = np.zeros((rx.shape[0], sf_re), np.complex64)
    grids[:, blk] = rx.reshape(rx.shape[0], -1)
    full = np.zeros((ce.shape[0], sf_re), np.complex64)
    full[:, blk] = ce.reshape(ce.shape[0], -1)
    return grids, full


class History:
    """pbch.c's bookkeeping on the recorded frames: what the object's history must hold after every call"""

    def __init__(self, nbits):
        self.h, self.fi = np.zeros((4, nbits), np.float32), 0

    def call(self, frame, ret):
        """-> number of leading frames of self.h to compare after this call"""
        self.fi += 1
        self.h[self.fi - 1] = frame
        kept = self.fi
        if ret == 1:
            self.fi = 0
        elif self.fi == 4:
            self.h[:3] = self.h[1:].copy()
            self.fi = kept = 3
        return kept


def rel(got, want):
    return float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max() / np.abs(want).max())


def check_flags(c, hyp, flags):
    """every recorded hypothesis' accept flag; the device's port-count index is 0 for a known port count"""
    for a in range(3):
        ks = np.nonzero(flags[a] >= 0)[0]
        if ks.size:
            dev_a = a if c["search"] else 0
            assert np.array_equal(hyp["ok"][dev_a, ks], flags[a, ks].astype(np.uint32)), (c["name"], NANTS[a])


@pytest.mark.parametrize("c", C.CASES, ids=lambda c: c["name"])
def test_decode_matches_reference(golden, c):
    z, metas, _ = golden
    m = metas[c["name"]]
    grids, ce = expand(c, z)
    pb = B.Pbch(cell_of(c))
    assert pb.q.nof_symbols == C.nof_symbols(c) and pb.q.search_all_ports == c["search"]
    assert pb.q.cell.nof_ports == (4 if c["search"] else c["ports"]) == ce.shape[0]
    hist = History(2 * C.nof_symbols(c))
    worst = 0.0
    for i, k in enumerate(m["calls"]):
        ret, pl, nports, off = pb.decode(grids[i], ce, k["noise"])
        assert ret == k["ret"], (i, ret)
        if ret == 1:
            assert list(pl) == k["payload"] and nports == k["nof_tx_ports"] and off == k["sfn_offset"], i
            assert off == (k["sfn"] % 4)  # one period: the position of the newest frame
        kept = hist.call(z[c["name"] + "/llr"][i], ret)
        got, fi = pb.last_llr()
        assert fi == k["frame_idx"] == hist.fi == pb.q.frame_idx, i
        d = rel(got[:kept], hist.h[:kept])
        worst = max(worst, d)
        print("%s call %d: LLR distance %.3e (bound %.3e)" % (c["name"], i, d, C.LLR_TOL))
        assert d <= C.LLR_TOL, (i, d)
        check_flags(c, pb.last_hyp(), z[c["name"] + "/flags"][i])
    pb.free()


def test_invalid_inputs(golden):
    _, _, meta = golden
    c = C.CASES[0]
    pb = B.Pbch(cell_of(c))
    L = B.lib()
    res = U.srsran_chest_dl_res_t()
    ptrs = (ctypes.c_void_p * 4)()
    assert L.srsran_pbch_decode(None, ctypes.byref(res), ptrs, None, None, None) == meta["invalid"][0]
    assert L.srsran_pbch_decode(ctypes.byref(pb.q), ctypes.byref(res), None, None, None, None) == meta["invalid"][1]
    assert pb.q.frame_idx == 0
    c3 = U.cell(6, 3, 0)
    assert pb.set_cell(c3) == B.ERROR_INVALID_INPUTS
    pb.free()


def test_set_cell_keeps_the_cell_of_an_unchanged_id():
    """pbch.c:247-252: the stored cell follows only a new cell id"""
    pb = B.Pbch(U.cell(25, 2, 7))
    assert pb.set_cell(U.cell(50, 1, 7)) == 0 and pb.q.cell.nof_prb == 25 and pb.q.cell.nof_ports == 2
    assert pb.set_cell(U.cell(50, 0, 8, cp=1)) == 0
    assert pb.q.cell.nof_prb == 50 and pb.q.cell.nof_ports == 4 and pb.q.search_all_ports and pb.q.nof_symbols == 216
    pb.free()


BATCH = ["p6_id0_1p", "p15_id1_4p_ext", "search_2p", "comb3_2p", "comb4_search", "shift6_search", "zero_mib",
         "p100_id2_4p", "comb_straddle"]


def run_batches(z, metas, names, delay, reverse):
    """every case's calls through srsran_pbch_gpu_decode_batch: case j starts at step delay[j]; the estimates of odd
    entries in the one-row form (the recorded channel is constant in time), those of every third entry with two rx
    antennas a port -> per case (results per call, history, frame_idx)"""
    objs, dev, keep = [], [], []
    for n in names:
        c = C.by_name(n)
        grids, ce = expand(c, z)
        _, nre, sf_re, _ = geometry(c)
        objs.append(B.Pbch(cell_of(c)))
        d_grid = torch.from_numpy(grids.view(np.float32).reshape(grids.shape[0], -1)).cuda()
        row = len(objs) % 2 == 0
        src = ce[:, sf_re // 2:sf_re // 2 + nre] if row else ce  # slot 1's first symbol
        nrx = 2 if len(objs) % 3 == 0 else 1  # a 2-rx UE's layout [port][rx][row]: rx 1 holds other values
        src = np.stack([src] + [src[::-1] * (0.5 + 0.25j)] * (nrx - 1), 1)
        d_ce = torch.from_numpy(np.ascontiguousarray(src).view(np.float32)).cuda()
        d_noise = torch.tensor([k["noise"] for k in metas[n]["calls"]], dtype=torch.float32, device="cuda")
        dev.append((d_grid, d_ce, nre if row else sf_re, d_noise, nrx))
    out = [[] for _ in names]
    steps = max(d + len(metas[n]["calls"]) for d, n in zip(delay, names))
    stream = torch.cuda.Stream()
    for t in range(steps):
        live = [j for j, n in enumerate(names) if 0 <= t - delay[j] < len(metas[n]["calls"])]
        if reverse:
            live = live[::-1]
        if not live:
            continue
        ents = []
        for j in live:
            i = t - delay[j]
            d_grid, d_ce, row_len, d_noise, nrx = dev[j]
            ents.append(objs[j].entry(d_grid[i].data_ptr(), d_ce.data_ptr(), row_len, nrx, d_noise[i:].data_ptr()))
        d_out = torch.zeros(len(live) * B.RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # the inputs and the cleared output are in place before the batch's own stream runs
        assert B.decode_batch(ents, d_out.data_ptr(), stream.cuda_stream) == 0
        keep.append((ents, d_out))
        stream.synchronize()
        res = d_out.cpu().numpy().view(B.RES_DTYPE)
        for r, j in zip(res, live):
            out[j].append(r.copy())
    final = []
    for j, o in enumerate(objs):
        h, fi = o.last_llr()
        assert o.q.frame_idx == fi
        final.append((out[j], h, fi))
        o.free()
    return final


def test_batch_is_bit_identical_to_single_calls(golden):
    z, metas, _ = golden
    single = []
    for n in BATCH:
        c = C.by_name(n)
        grids, ce = expand(c, z)
        pb = B.Pbch(cell_of(c))
        res = [pb.decode(grids[i], ce, k["noise"]) for i, k in enumerate(metas[n]["calls"])]
        single.append((res, *pb.last_llr()))
        pb.free()
    orders = [run_batches(z, metas, BATCH, [0] * len(BATCH), False),
              run_batches(z, metas, BATCH, [(3 * j) % 4 for j in range(len(BATCH))], True)]
    for got in orders:
        for n, (res, h, fi), (bres, bh, bfi) in zip(BATCH, single, got):
            assert fi == bfi and len(res) == len(bres), n
            assert np.array_equal(h.view(np.uint32), bh.view(np.uint32)), n  # the whole history, bit for bit
            for (ret, pl, nports, off), r in zip(res, bres):
                assert ret == int(r["found"]), n
                if ret == 1:
                    assert np.array_equal(pl, r["payload"]) and nports == r["nof_tx_ports"] and off == r["sfn_offset"], n
                else:
                    assert not r["payload"].any() and r["nof_tx_ports"] == 0 and r["sfn_offset"] == 0, n


def test_batch_descriptor_regrowth_is_bit_identical(golden):
    """One object as the first entry (the owner of the batch's descriptors) of a one-entry batch, a four-entry batch
    (its descriptor buffer is reallocated) and a one-entry batch again.  A second set of objects takes the same
    calls behind a new first entry every time, so none of them ever owns descriptors: results and histories of the
    two sets are the same bits."""
    z, metas, _ = golden
    names = ["comb3_2p", "p6_id0_1p", "p15_id1_4p_ext", "search_2p"]  # the owner has three recorded calls
    ncalls = [len(metas[n]["calls"]) for n in names]

    def make(n):
        c = C.by_name(n)
        grids, ce = expand(c, z)
        _, _, sf_re, _ = geometry(c)
        d_grid = torch.from_numpy(grids.view(np.float32).reshape(grids.shape[0], -1)).cuda()
        d_ce = torch.from_numpy(np.ascontiguousarray(ce[:, None]).view(np.float32)).cuda()
        d_noise = torch.tensor([k["noise"] for k in metas[n]["calls"]], dtype=torch.float32, device="cuda")
        return dict(o=B.Pbch(cell_of(c)), g=d_grid, ce=d_ce, row=sf_re, noise=d_noise, i=0, n=n)

    def entry(x):
        i = min(x["i"], x["g"].shape[0] - 1)
        x["i"] += 1
        return x["o"].entry(x["g"][i].data_ptr(), x["ce"].data_ptr(), x["row"], 1, x["noise"][i:].data_ptr())

    def batch(objs):
        ents = [entry(x) for x in objs]
        d_out = torch.zeros(len(ents) * B.RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert B.decode_batch(ents, d_out.data_ptr()) == 0
        torch.cuda.synchronize()
        return d_out.cpu().numpy().view(B.RES_DTYPE)

    live, ref, extra = [make(n) for n in names], [make(n) for n in names], []
    assert ncalls[0] >= 3
    found = 0
    for sel in ([0], [0, 1, 2, 3], [0]):
        got = batch([live[j] for j in sel])
        extra.append(make(names[1]))
        want = batch([extra[-1]] + [ref[j] for j in sel])[1:]
        assert got.tobytes() == want.tobytes(), sel
        found += int(got["found"].sum())
    assert found > 0
    for a, b in zip(live, ref):
        (h, fi), (bh, bfi) = a["o"].last_llr(), b["o"].last_llr()
        assert fi == bfi and np.array_equal(h.view(np.uint32), bh.view(np.uint32)), a["n"]
    for x in live + ref + extra:
        x["o"].free()


def test_batch_refuses_bad_entries():
    pb = B.Pbch(U.cell(6, 1, 0))
    d = torch.zeros(4096, dtype=torch.float32, device="cuda")
    e = pb.entry(d.data_ptr(), d.data_ptr(), 72, 1, d.data_ptr())
    assert B.decode_batch([e, e], d.data_ptr()) == B.ERROR_INVALID_INPUTS  # an object twice
    assert B.decode_batch([pb.entry(d.data_ptr(), d.data_ptr(), 0, 1, d.data_ptr())], d.data_ptr()) == \
        B.ERROR_INVALID_INPUTS
    assert B.decode_batch([pb.entry(None, d.data_ptr(), 72, 1, d.data_ptr())], d.data_ptr()) == B.ERROR_INVALID_INPUTS
    assert B.decode_batch([], d.data_ptr()) == 0
    pb.free()


# ---------------------------------------------------------------- srsran_ue_mib_* on samples
def enb_subframe0(cell, sfns):
    """subframe 0 of the given radio frames from the eNB object (put_base: CRS, PSS / SSS, PBCH, PCFICH) ->
    (frames, ports, sf_len) complex64 samples"""
    enb = E.EnbDl(cell)
    N = U.lib().srsran_symbol_sz(cell.nof_prb)
    d_tx = torch.zeros((len(sfns), cell.nof_ports, 15 * N, 2), dtype=torch.float32, device="cuda")
    assert enb.tx_batch([(10 * s, 1, None, [], (True, [])) for s in sfns], d_tx.data_ptr()) == 0
    torch.cuda.synchronize()
    tx = d_tx.cpu().numpy().view(np.complex64)[..., 0]
    enb.free()
    return tx


def through_channel(tx, snr_db, rng, taps=((0, 1.0), (2, 0.35j), (5, -0.2))):
    """every port through its own rotation of a short multipath channel (circular within the subframe), plus AWGN"""
    F, P, n = tx.shape
    y = np.zeros((F, n), np.complex128)
    for p in range(P):
        for d, a in taps:
            y += a * np.exp(0.7j * p * (d + 1)) * np.roll(tx[:, p].astype(np.complex128), d, axis=1)
    sig = np.mean(np.abs(y) ** 2)
    w = (rng.standard_normal(y.shape) + 1j * rng.standard_normal(y.shape)) / np.sqrt(2.0)
    return (y + np.sqrt(sig * 10.0 ** (-snr_db / 10.0)) * w).astype(np.complex64)


class Composition:
    """the test's own srsran_ue_mib_decode: srsran_ofdm_rx_sf, srsran_chest_dl_estimate with subframe 0 and
    srsran_pbch_decode through the library, with ue_mib.c:128-172's counter rules in Python"""

    def __init__(self, cell):
        dec = U.cell(cell.nof_prb, 4 if cell.nof_ports == 0 else cell.nof_ports, cell.id, cp=cell.cp)
        self.fft = U.OfdmRx(cell.nof_prb, cp=cell.cp)
        self.chest = U.ChestDl(dec, 1)
        self.pbch = B.Pbch(cell)
        self.frame_cnt = 0

    def decode(self, samples):
        grid = self.fft.rx(samples)
        ce, res = self.chest.estimate([grid], 0)
        if self.frame_cnt > 8:
            self.frame_cnt = 0
            self.pbch.reset()
        r = self.pbch.decode(grid, ce[:, 0], res.noise_estimate)
        if r[0] == 1:
            self.frame_cnt = 0
            self.pbch.reset()
        else:
            self.frame_cnt += 1
        return r

    def free(self):
        self.pbch.free()
        self.chest.free()
        self.fft.free()


def same_result(a, b):
    return a[0] == b[0] and (a[0] != 1 or (np.array_equal(a[1], b[1]) and a[2:] == b[2:]))


def test_ue_mib_decode_equals_composition_and_resets_after_nine_misses():
    cell = U.cell(15, 2, 11)
    search = U.cell(15, 0, 11)
    rng = np.random.default_rng(3)
    sfns = list(range(40, 46))
    rx = through_channel(enb_subframe0(cell, sfns), 20.0, rng)
    n = rx.shape[1]
    noise = ((rng.standard_normal((10, n)) + 1j * rng.standard_normal((10, n))) / np.sqrt(2.0)).astype(np.complex64)
    # ten frames of noise (nine misses reach frame_cnt = 9, the tenth call resets first), then the cell's frames
    seq = list(noise) + list(rx)
    mib, comp = B.UeMib(search), Composition(search)
    assert mib.q.fft.cfg.cp == 0 and mib.q.pbch.search_all_ports and mib.q.chest.cell.nof_ports == 4
    cnts = []
    for i, x in enumerate(seq):
        a, b = mib.decode(x), comp.decode(x)
        assert same_result(a, b), i
        assert mib.q.frame_cnt == comp.frame_cnt and mib.q.pbch.frame_idx == comp.pbch.q.frame_idx, i
        ha, hb = mib.last_llr(), comp.pbch.last_llr()
        assert ha[1] == hb[1] and np.array_equal(ha[0][:ha[1]].view(np.uint32), hb[0][:hb[1]].view(np.uint32)), i
        cnts.append((mib.q.frame_cnt, mib.q.pbch.frame_idx, a[0]))
    # misses: the history fills to 3 and stays; the tenth call starts from an empty history
    assert [c[0] for c in cnts[:10]] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 1]
    assert [c[1] for c in cnts[:10]] == [1, 2, 3, 3, 3, 3, 3, 3, 3, 1]
    assert not any(c[2] for c in cnts[:10])
    # the first clean frame decodes although a noise frame is still stored: found alone, sfn_offset from it
    assert cnts[10] == (0, 0, 1)
    for i, s in enumerate(sfns):
        r = mib.decode(rx[i])
        assert r[0] == 1 and r[2] == 2
        prb, plen, pres, sfn = B.mib_unpack(r[1])
        assert (prb, plen, pres) == (15, cell.phich_length, cell.phich_resources) and (sfn + r[3]) % 1024 == s
    mib.free()
    comp.free()


def test_ue_mib_extended_cp_switches_the_ofdm_object():
    mib = B.UeMib(U.cell(6, 0, 3, cp=1))
    assert mib.q.fft.cfg.cp == 1 and mib.q.pbch.nof_symbols == 216
    mib.free()


def test_ue_mib_batch_is_bit_identical_to_single_calls():
    """srsran_ue_mib_gpu_decode_batch against srsran_ue_mib_decode on the same samples: results, counters and the whole
    LLR history bit for bit, with all objects in one batch, and with the entries reversed while every object
    alternates between the batch and the synchronous call (so batches of changing composition, and histories filled
    by both calls in turn)"""
    cells = [U.cell(6, 1, 4), U.cell(25, 2, 150), U.cell(15, 4, 302, cp=1)]
    rng = np.random.default_rng(9)
    sfns = [6, 7, 8, 9, 10, 11]
    rxs = []
    for k, cl in enumerate(cells):
        rx = through_channel(enb_subframe0(cl, sfns), (15.0, -2.0, 4.0)[k], rng)
        for t in (k % 2, 3):  # noise frames: misses, then decodes with stored frames
            rx[t] = ((rng.standard_normal(rx.shape[1]) + 1j * rng.standard_normal(rx.shape[1])) / 2).astype(np.complex64)
        rxs.append(rx)
    search = [U.cell(c.nof_prb, 0, c.id, cp=c.cp) for c in cells]
    singles, batch, mixed = ([B.UeMib(c) for c in search] for _ in range(3))
    d_rx = [torch.from_numpy(r.view(np.float32)).cuda() for r in rxs]
    K = len(cells)

    def run(mibs, ks, t):
        d_out = torch.zeros(len(ks) * B.RES_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        assert B.ue_mib_decode_batch([mibs[k] for k in ks], [d_rx[k][t].data_ptr() for k in ks], d_out.data_ptr()) == 0
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().view(B.RES_DTYPE)
        return {k: (int(g["found"]), g["payload"].copy(), int(g["nof_tx_ports"]), int(g["sfn_offset"]))
                for k, g in zip(ks, got)}

    found = 0
    for t in range(len(sfns)):
        want = [m.decode(rxs[k][t]) for k, m in enumerate(singles)]
        got_b = run(batch, list(range(K)), t)
        in_batch = [k for k in reversed(range(K)) if (t + k) % 2 == 0]
        got_m = run(mixed, in_batch, t) if in_batch else {}
        for k in range(K):
            if k not in got_m:
                got_m[k] = mixed[k].decode(rxs[k][t])
        for k in range(K):
            hs = singles[k].last_llr()
            state = (singles[k].q.frame_cnt, singles[k].q.pbch.frame_idx)
            for name, mibs, got in (("batch", batch, got_b), ("mixed", mixed, got_m)):
                assert same_result(want[k], got[k]), (name, t, k)
                assert mibs[k].sync() == state, (name, t, k)
                h = mibs[k].last_llr()
                assert h[1] == hs[1] and np.array_equal(h[0].view(np.uint32), hs[0].view(np.uint32)), (name, t, k)
            found += want[k][0]
    assert 0 < found < K * len(sfns)  # the sequences hold decodes and misses
    for m in singles + batch + mixed:
        m.free()


def test_c99_caller_decodes_a_recorded_case(golden):
    z, metas, _ = golden
    c = C.by_name("p25_id1_1p")
    grids, ce = expand(c, z)
    k = metas[c["name"]]["calls"][0]
    src = r'''
#include "srsran_pbch.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(int argc, char** argv) {
  uint32_t n = (uint32_t)atoi(argv[2]), np = 0, sfn = 0;
  cf_t* grid = malloc(sizeof(cf_t) * n); cf_t* ce = malloc(sizeof(cf_t) * n);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(grid, sizeof(cf_t), n, f) != n || fread(ce, sizeof(cf_t), n, f) != n) return 10;
  fclose(f);
  srsran_cell_t cell = {25, 1, 301, SRSRAN_CP_NORM, SRSRAN_PHICH_NORM, SRSRAN_PHICH_R_1, SRSRAN_FDD}, got;
  srsran_pbch_t q;
  srsran_chest_dl_res_t ch;
  memset(&ch, 0, sizeof(ch));
  cf_t* y[SRSRAN_MAX_PORTS] = {grid, 0, 0, 0};
  uint8_t pl[SRSRAN_BCH_PAYLOAD_LEN];
  int off = -1;
  ch.ce[0][0] = ce;
  ch.noise_estimate = (float)atof(argv[3]);
  if (srsran_pbch_init(&q) || srsran_pbch_set_cell(&q, cell)) return 11;
  int ret = srsran_pbch_decode(&q, &ch, y, pl, &np, &off);
  srsran_pbch_mib_unpack(pl, &got, &sfn);
  printf("%d %u %d %u %u %u\n", ret, np, off, got.nof_prb, sfn, q.frame_idx);
  srsran_pbch_free(&q);
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "caller.c"), "w").write(src)
        with open(os.path.join(d, "in.bin"), "wb") as f:
            f.write(grids[0].tobytes())
            f.write(ce[0].tobytes())
        exe = os.path.join(d, "caller")
        libdir = os.path.dirname(tdec.LIB_PATH)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(d, "caller.c"), "-L", libdir, "-lsrsran_4g_amd", "-Wl,-rpath," + libdir, "-o", exe],
                       check=True)
        out = subprocess.run([exe, os.path.join(d, "in.bin"), str(grids.shape[1]), repr(k["noise"])], check=True,
                             capture_output=True, text=True).stdout
    assert [int(x) for x in out.split()] == [1, 1, k["sfn_offset"], 25, k["sfn"] & ~3, 0]
