"""PUSCH transmit on the GPU (srsran_ulsch_encode, srsran_pusch_encode, the DMRS put, srsran_ue_ul_gpu_tx_batch)
against tests/golden/pusch_tx_golden.npz, recorded from the compiled reference transmitter (sch.c, pusch.c, uci.c,
refsignal_ul.c; tests/golden/make_pusch_tx_golden.py), with the tolerances of tests/pusch_tx_cases.py.

  per case   srsran_ulsch_encode's return, K_segm, g and q bits EQUAL; srsran_pusch_encode's write-back EQUAL, its grid
             within max(4 x MEASURED, 1e-6 max|x|), every RE outside the grant still the sentinel; the UE path's
             scrambled bits EQUAL, symbols and grid within bound, DMRS REs equal to the library's own
             srsran_refsignal_dmrs_pusch_gen_cell, within pusch_cases.dmrs_exact's bound of the exact sequence and
             within twice that of the reference's
  sweep      40 random small grants (L <= 6, QPSK / 16QAM / 64QAM, random UCI, both CPs, shortened or not): q EQUAL
  batch      all cases in one srsran_ue_ul_gpu_tx_batch, two orders and two compositions: bit-identical to single calls
  refusals   each returns its code
  C99        a caller written like the PUSCH part of the reference's pusch_test.c links and encodes t2
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, HERE)

import pusch as OP  # noqa: E402  (oracle/pusch.py)
import pusch_cases as PC  # noqa: E402
import pusch_tx_cases as TC  # noqa: E402
import uci_cases as UC  # noqa: E402

pytestmark = pytest.mark.gpu
IDS = [c["name"] for c in TC.CASES]
SENTINEL = np.complex64(77.0 - 33.0j)


@pytest.fixture(scope="module")
def env():
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.fail("no HIP device on a GPU test run")
    if not OP.ref_available():  # on a HIP box the parity checker must be there: fail, never skip
        pytest.fail("oracle/_ref/libsrsref.so missing: the reference checker of this module was not built")
    return OP.PuschOracle()


def _limited(c, cfg):
    """the configuration after srsran_pusch_encode's 64QAM limit (what the model is computed for)"""
    from srsran_4g_amd import sch as S
    if not c["enable_64qam"] and cfg.grant.tb.mod >= S.MOD_FROM_QM[6]:
        cfg.grant.tb.mod = S.MOD_FROM_QM[4]
        cfg.grant.tb.nof_bits = cfg.grant.nof_re * 4


@pytest.fixture(scope="module")
def fx():
    return TC.Fixture()


@pytest.fixture(scope="module")
def models(env):
    """per case: the model, computed once and shared (never modified)"""
    out = {}
    for c in TC.CASES:
        cell, d, sf, cfg = TC.make(c)
        _limited(c, cfg)
        payload, u = TC.payload_uci(c, cfg)
        out[c["name"]] = (TC.tx_model(env, c, cfg, payload, u), payload, u)
    return out


@pytest.mark.parametrize("c", TC.CASES, ids=IDS)
def test_ulsch_encode(env, fx, c):
    from srsran_4g_amd import sch as S
    from srsran_4g_amd import ue_ul as UL
    cell, d, sf, cfg = TC.make(c)
    _limited(c, cfg)
    ret, K_segm, mod, nof_bits = (int(v) for v in fx.get(c, "out"))
    assert (cfg.grant.tb.mod, cfg.grant.tb.nof_bits) == (mod, nof_bits)
    sch = S.Sch()
    got, g, q = UL.ulsch_encode(sch, cfg, fx.get(c, "payload") if cfg.grant.tb.tbs else None, fx.uci(c))
    assert (got, cfg.K_segm) == (ret, K_segm)
    assert np.array_equal(q[:nof_bits // 8], fx.get(c, "q"))
    # the whole of g: the CQI bits, the TB's bits from their (unaligned) offset, zero bits after them
    assert np.array_equal(g[:nof_bits // 8], fx.get(c, "g"))
    assert not np.any(g[nof_bits // 8:]) and not np.any(q[nof_bits // 8:])


@pytest.mark.parametrize("c", TC.CASES, ids=IDS)
def test_pusch_encode(env, models, fx, c):
    from srsran_4g_amd import ue_ul as UL
    m, payload, u = models[c["name"]]
    cell, d, sf, cfg = TC.make(c)
    pu = UL.PuschUe(cell, max_prb=c["nof_prb"])
    try:
        grid = np.full((2 * m["nsym"], 12 * c["nof_prb"]), SENTINEL, np.complex64)
        assert pu.encode(sf, cfg, payload if cfg.grant.tb.tbs else None, u, grid) == 0
        want = TC.make(c)[3]
        _limited(c, want)
        assert (cfg.grant.tb.mod, cfg.grant.tb.nof_bits) == (want.grant.tb.mod, want.grant.tb.nof_bits)
        assert (cfg.grant.tb.mod, cfg.grant.tb.nof_bits) == tuple(int(v) for v in fx.get(c, "out")[2:])
        data, _ = TC.grant_mask(c, m)
        dist, bound = TC.grid_dist(grid[data], fx.grid(c)[data])
        print(c["name"], "pusch_encode grid: distance %.3e, bound %.3e" % (dist, bound))
        assert dist <= bound
        assert np.all(grid[~data] == SENTINEL)
    finally:
        pu.free()


@pytest.mark.parametrize("c", TC.CASES, ids=IDS)
def test_ue_path_bits_symbols_grid_dmrs(env, models, fx, c):
    from srsran_4g_amd import pusch as P
    from srsran_4g_amd import ue_ul as UL
    m, payload, u = models[c["name"]]
    cell, d, sf, cfg = TC.make(c)
    ue = UL.UeUl(cell)
    try:
        ucfg = TC.ue_cfg(c, cfg, d)
        ret, x = ue.encode(sf, ucfg, payload if cfg.grant.tb.tbs else None, u)
        assert ret == 1
        s, dsym, grid = ue.last()
        grid = grid.reshape(2 * m["nsym"], -1)
        assert np.array_equal(s, fx.get(c, "s"))
        if fx.has(c, "d"):
            derr = float(np.abs(dsym - fx.get(c, "d")).max() / np.abs(fx.get(c, "d")).max())
            print(c["name"], "symbols: distance %.3e, bound %.3e" % (derr, TC.D_TOL))
            assert derr <= TC.D_TOL
        data, dm = TC.grant_mask(c, m)
        dist, bound = TC.grid_dist(grid[data], fx.grid(c)[data])
        print(c["name"], "ue_ul grid: distance %.3e, bound %.3e" % (dist, bound))
        assert dist <= bound
        assert np.all(grid[~(data | dm)] == 0)
        ok, r = P.dmrs(cell, d, c["L"], c["tti"] % 10, c["n_dmrs"])
        assert ok == 0
        got = np.concatenate([grid[(sl + 1) * m["nsym"] - 4, c["n_tilde"][sl] * 12:c["n_tilde"][sl] * 12 + m["M"]]
                              for sl in (0, 1)])
        assert np.array_equal(got, r)
        exact, bnd = PC.dmrs_exact(dict(c, dmrs=[int(v) for v in c["dmrs"]]))
        assert PC.err("abs", got, exact) <= bnd and PC.err("abs", got, fx.get(c, "dmrs")) <= 2 * bnd
        # srsran_refsignal_dmrs_pusch_put_cell writes the same REs of a host grid and nothing else
        host = np.full(grid.shape, SENTINEL, np.complex64)
        assert UL.dmrs_put(cell, cfg, r, host) == 0
        assert np.array_equal(host[dm], grid[dm]) and np.all(host[~dm] == SENTINEL)
    finally:
        ue.free()


def test_random_small_grants(env):
    """q bits of srsran_ulsch_encode equal the reference encoder's over random small grants"""
    import pusch_tx as TX
    import uci as RU
    from srsran_4g_amd import pdcch
    from srsran_4g_amd import sch as S
    from srsran_4g_amd import ue_ul as UL
    rng = np.random.default_rng(2024)
    ref, sch, L = RU.RefUci(), S.Sch(), pdcch.lib()
    cqis = [None, (UC.WB, dict()), (UC.WB, dict(pmi_present=True)), (UC.SB_UE, dict(subband_label_2_bits=True)),
            (UC.HL, dict(N=5)), (UC.SB_DIFF, dict(L=3))]
    done = 0
    while done < 40:
        Lp, Qm = int(rng.choice([1, 2, 3, 4, 5, 6])), int(rng.choice([2, 4, 6]))
        cp, sh = int(rng.integers(0, 2)), bool(rng.integers(0, 2))
        nsymb = (12 if cp == 0 else 10) - (1 if sh else 0)
        i_tbs = int(rng.integers(0, 27))
        tbs = int(L.srsran_ra_tbs_from_idx(i_tbs, Lp))
        if tbs + 24 > 0.8 * Lp * 12 * nsymb * Qm:
            continue
        nack, ri = int(rng.integers(0, 5)), int(rng.integers(0, 3))
        cqi = cqis[int(rng.integers(0, len(cqis)))]
        mk = lambda: TX.make_cfg(25, Qm, Lp, 3, tbs, nack, ri, cqi, cp=cp, shortened=sh, rv=int(done % 4))  # noqa: E731
        cfg, cfg_ref = mk(), mk()
        u = UC.random_uci(cfg, rng)
        cfg_ref.uci_cfg.cqi.rank_is_not_one = cfg.uci_cfg.cqi.rank_is_not_one
        try:
            Qri, Qcqi, G = ref.tx_sizes(cfg_ref, u)
        except AssertionError:  # the reference's encoder refuses the mix: so does the library
            assert UL.ulsch_encode(sch, cfg, np.zeros(max(tbs // 8, 1), np.uint8), u)[0] < 0
            continue
        payload = rng.integers(0, 256, tbs // 8, dtype=np.uint8)
        e = env.ora.dlsch_encode(tbs, Qm, cfg.grant.tb.rv, G * Qm, payload)
        types, sizes = ref.tx(cfg_ref, u, e)
        ret, g, q = UL.ulsch_encode(sch, cfg, payload, u)
        assert ret == (sizes[3] + Qri) * Qm, (Lp, Qm, nack, ri, cqi)
        want = np.where(types <= 1, types, 0).astype(np.uint8)
        assert np.array_equal(np.unpackbits(q[:types.size // 8]), want), (Lp, Qm, cp, sh, tbs, nack, ri, cqi)
        done += 1


def test_scratch_regrowth_is_bit_identical(env, models):
    """One UL-SCH object and one ue_ul object: the smallest case, then a call that needs more of every growable
    buffer (the 25-PRB, 2-code-block grants; a batch of every 25-PRB case), then the smallest again -- bits,
    samples and grids equal a fresh object's."""
    import torch

    from srsran_4g_amd import sch as S
    from srsran_4g_amd import ue_ul as UL
    by = TC.BY_NAME

    def enc(sch, c):
        cell, d, sf, cfg = TC.make(c)
        _limited(c, cfg)
        _, payload, u = models[c["name"]]
        ret, g, q = UL.ulsch_encode(sch, cfg, payload if cfg.grant.tb.tbs else None, u)
        return [np.int64(ret), g.copy(), q.copy()]

    one = S.Sch()
    for name in ("t1", "t9", "t8", "t1"):
        fresh = S.Sch()
        want = enc(fresh, by[name])
        fresh.free()
        assert all(np.array_equal(g, w) for g, w in zip(enc(one, by[name]), want)), name
    one.free()

    cell25 = TC.make(by["t11a"])[0]
    names25 = [c["name"] for c in TC.CASES if (c["nof_prb"], c["cp"]) == (25, 0)]
    assert len(names25) > 3

    def tx(ue, names):
        keep, ents, outs = [], [], []
        for i, name in enumerate(names):
            c = by[name]
            m, payload, u = models[name]
            cell, d, sf, cfg = TC.make(c)
            ucfg = TC.ue_cfg(c, cfg, d, mode=i % 2, peak=0.7, cfo=1.3e-1 if c["L"] % 2 else None)
            d_pl = torch.from_numpy(np.concatenate([payload, np.zeros(16, np.uint8)])).cuda()
            d_out = torch.zeros(2 * ue.sf_len, dtype=torch.float32, device="cuda")
            d_grid = torch.zeros(2 * 2 * m["nsym"] * 12 * c["nof_prb"], dtype=torch.float32, device="cuda")
            keep.extend([d_pl, ucfg, sf, u, cfg, d])
            outs += [d_out, d_grid]
            ents.append((ue, sf, ucfg, u, d_pl.data_ptr() if cfg.grant.tb.tbs else None, d_out.data_ptr(),
                         d_grid.data_ptr()))
        assert UL.tx_batch(ents) == 0
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs]

    ue = UL.UeUl(cell25)
    try:
        for names in (["t11a"], names25, ["t11a"]):
            fresh = UL.UeUl(cell25)
            try:
                want = tx(fresh, names)
            finally:
                fresh.free()
            got = tx(ue, names)
            assert np.abs(got[0]).max() > 0
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), names
    finally:
        ue.free()


def test_batch_bit_identical_to_single_calls(env, models):
    """all cases in one batch, two orders, two compositions; samples and grids equal the single calls bit for bit"""
    import torch

    from srsran_4g_amd import ue_ul as UL
    ues, single, keep = {}, {}, []
    try:
        for nprb, cp in sorted({(c["nof_prb"], c["cp"]) for c in TC.CASES}):
            c0 = next(c for c in TC.CASES if (c["nof_prb"], c["cp"]) == (nprb, cp))
            ues[(nprb, cp)] = UL.UeUl(TC.make(c0)[0])

        def entry(c, mode):
            m, payload, u = models[c["name"]]
            cell, d, sf, cfg = TC.make(c)
            ue = ues[(c["nof_prb"], c["cp"])]
            ucfg = TC.ue_cfg(c, cfg, d, mode=mode, peak=0.7, cfo=1.3e-1 if c["L"] % 2 else None)
            d_pl = torch.from_numpy(np.concatenate([payload, np.zeros(16, np.uint8)])).cuda()
            d_out = torch.zeros(2 * ue.sf_len, dtype=torch.float32, device="cuda")
            d_grid = torch.zeros(2 * 2 * m["nsym"] * 12 * c["nof_prb"], dtype=torch.float32, device="cuda")
            keep.extend([d_pl, ucfg, sf, u, cfg, d])
            return (ue, sf, ucfg, u, d_pl.data_ptr() if cfg.grant.tb.tbs else None, d_out.data_ptr(),
                    d_grid.data_ptr()), d_out, d_grid

        for i, c in enumerate(TC.CASES):
            e, d_out, d_grid = entry(c, i % 2)
            assert UL.tx_batch([e]) == 0
            torch.cuda.synchronize()
            single[c["name"]] = (d_out.cpu().numpy().copy(), d_grid.cpu().numpy().copy())
            assert np.abs(single[c["name"]][0]).max() > 0
        order = list(range(len(TC.CASES)))
        for sel in (order, order[::-1], order[::2], order[1::2][::-1] + order[:3]):
            built = [entry(TC.CASES[i], i % 2) for i in sel]
            assert UL.tx_batch([b[0] for b in built]) == 0
            torch.cuda.synchronize()
            for i, (_, d_out, d_grid) in zip(sel, built):
                name = TC.CASES[i]["name"]
                assert np.array_equal(d_out.cpu().numpy(), single[name][0]), name
                assert np.array_equal(d_grid.cpu().numpy(), single[name][1]), name
    finally:
        for ue in ues.values():
            ue.free()


def test_refusals(env, models):
    from srsran_4g_amd import sch as S
    from srsran_4g_amd import ue_ul as UL
    c = TC.BY_NAME["t2"]
    m, payload, u = models["t2"]
    cell, d, sf, cfg = TC.make(c)
    L = UL.lib()
    sch = S.Sch()
    assert UL.ulsch_encode(sch, cfg, None, u)[0] == UL.ERROR  # data == NULL with tbs > 0
    bad = TC.make(c)[3]
    bad.grant.tb.tbs = 1040  # 1064 bits with the CRC is no interleaver size: 24 filler bits
    assert UL.ulsch_encode(sch, bad, np.zeros(130, np.uint8), u)[0] == UL.ERROR
    bad = TC.make(c)[3]
    bad.uci_cfg.cqi.ri_len = 3  # the reference encodes ri[2] = {ri, 0}
    assert UL.ulsch_encode(sch, bad, payload, u)[0] == UL.ERROR_INVALID_INPUTS
    pu, ue = UL.PuschUe(cell, max_prb=15), UL.UeUl(cell)
    try:
        grid = np.zeros((14, 180), np.complex64)
        bad = TC.make(c)[3]
        bad.grant.L_prb = 7  # not 2^a 3^b 5^c
        assert pu.encode(sf, bad, payload, u, grid) == UL.ERROR_INVALID_INPUTS
        bad = TC.make(c)[3]
        bad.grant.nof_re = pu.q.max_re + 12
        assert pu.encode(sf, bad, payload, u, grid) == UL.ERROR_INVALID_INPUTS
        bad = TC.make(c)[3]
        bad.grant.tb.rv = 5
        assert pu.encode(sf, bad, payload, u, grid) == -5  # SRSRAN_ERROR_OUT_OF_BOUNDS
        assert not np.any(grid)
        assert L.srsran_ue_ul_set_cfr(ctypes.byref(ue.q), None) == UL.ERROR
        ucfg = TC.ue_cfg(c, cfg, d)
        assert L.srsran_ue_ul_pregen_signals(ctypes.byref(ue.q), ctypes.byref(ucfg)) == UL.ERROR
        # SRS: refused where the subframe carries this UE's SRS (srs_tx_enabled: subframe_config 0 makes every subframe
        # a cell SRS subframe; I_srs 0 / 1 have period 2, offset 0 / 1; t2 is sent in tti 4), encoded elsewhere
        ucfg.ul_cfg.srs.configured, ucfg.ul_cfg.srs.I_srs = True, 0
        assert ue.encode(sf, ucfg, payload, u)[0] == UL.ERROR
        ucfg.ul_cfg.srs.I_srs = 1
        assert ue.encode(sf, ucfg, payload, u)[0] == 1
        ucfg.ul_cfg.srs.I_srs, ucfg.ul_cfg.srs.subframe_config = 0, 3  # cell SRS subframes 0 and 5 only
        assert ue.encode(sf, ucfg, payload, u)[0] == 1
        ucfg = TC.ue_cfg(c, cfg, d)
        ucfg.grant_available = False
        ucfg.ul_cfg.pucch.uci_cfg.ack[0].nof_acks = 1
        assert ue.encode(sf, ucfg, payload, u)[0] == UL.ERROR  # the PUCCH branch
        ucfg.ul_cfg.pucch.uci_cfg.ack[0].nof_acks = 0
        ucfg.ul_cfg.srs.configured = True
        assert ue.encode(sf, ucfg, payload, u)[0] == UL.ERROR  # the SRS-only branch (tti 4, I_srs 0)
        ucfg.ul_cfg.srs.I_srs = 1
        ret, x = ue.encode(sf, ucfg, payload, u)  # no SRS in this subframe: nothing to send
        assert ret == 0 and not np.any(x)
    finally:
        pu.free()
        ue.free()


C_CALLER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "srsran_ue_ul.h"

int main(int argc, char** argv)
{
  srsran_cell_t cell;
  memset(&cell, 0, sizeof(cell));
  cell.nof_prb = 15; cell.nof_ports = 1; cell.id = 150; cell.cp = SRSRAN_CP_NORM;
  srsran_pusch_t pusch;
  if (srsran_pusch_init_ue(&pusch, cell.nof_prb) || srsran_pusch_set_cell(&pusch, cell)) return 1;
  srsran_pusch_cfg_t cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.rnti = 0x46;
  cfg.grant.L_prb = 2; cfg.grant.n_prb[0] = cfg.grant.n_prb[1] = 6;
  cfg.grant.n_prb_tilde[0] = cfg.grant.n_prb_tilde[1] = 6;
  cfg.grant.nof_symb = 12; cfg.grant.nof_re = 2 * 12 * 12;
  cfg.grant.tb.mod = SRSRAN_MOD_16QAM; cfg.grant.tb.tbs = atoi(argv[2]); cfg.grant.tb.rv = 0;
  cfg.grant.tb.nof_bits = cfg.grant.nof_re * 4; cfg.grant.tb.enabled = true;
  cfg.grant.n_dmrs = 2;
  cfg.uci_offset.I_offset_cqi = 9; cfg.uci_offset.I_offset_ri = 6; cfg.uci_offset.I_offset_ack = 8;
  cfg.uci_cfg.ack[0].nof_acks = 1;
  cfg.enable_64qam = true;
  srsran_ul_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  sf.tti = 4;
  uint32_t nre = 14 * 12 * cell.nof_prb;
  cf_t* grid = calloc(nre, sizeof(cf_t));
  uint8_t* payload = malloc(cfg.grant.tb.tbs / 8);
  for (int i = 0; i < cfg.grant.tb.tbs / 8; i++) payload[i] = (uint8_t)(i * 37 + 11);
  srsran_pusch_data_t data;
  memset(&data, 0, sizeof(data));
  data.ptr = payload;
  data.uci.ack.ack_value[0] = 1;
  if (srsran_pusch_encode(&pusch, &sf, &cfg, &data, grid)) return 2;
  srsran_refsignal_dmrs_pusch_cfg_t dmrs = {1, 3, true, false};
  cf_t* r = calloc(2 * 12 * cfg.grant.L_prb, sizeof(cf_t));
  if (srsran_refsignal_dmrs_pusch_gen_cell(&cell, &dmrs, cfg.grant.L_prb, sf.tti % 10, cfg.grant.n_dmrs, r)) return 3;
  if (srsran_refsignal_dmrs_pusch_put_cell(&cell, &cfg, r, grid)) return 4;
  FILE* f = fopen(argv[1], "wb");
  fwrite(grid, sizeof(cf_t), nre, f);
  fclose(f);
  srsran_pusch_free(&pusch);
  free(grid); free(payload); free(r);
  return 0;
}
'''


def test_c99_caller_encodes_t2(env):
    from srsran_4g_amd import tdec
    c = TC.BY_NAME["t2"]
    cell, d, sf, cfg = TC.make(c)
    payload = ((np.arange(cfg.grant.tb.tbs // 8) * 37 + 11) & 0xff).astype(np.uint8)
    u = __import__("srsran_4g_amd.sch", fromlist=["x"]).srsran_uci_value_t()
    u.ack.ack_value[0] = 1
    m = TC.tx_model(env, c, cfg, payload, u)
    libdir = os.path.dirname(tdec.LIB_PATH)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, dat = os.path.join(tmp, "ue.c"), os.path.join(tmp, "ue"), os.path.join(tmp, "grid.bin")
        open(src, "w").write(C_CALLER)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                            "-L", libdir, "-lsrsran_4g_amd", "-Wl,-rpath," + libdir, "-lm"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe, dat, str(cfg.grant.tb.tbs)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        grid = np.fromfile(dat, np.complex64).reshape(14, -1)
    data, dm = TC.grant_mask(c, m)
    dist, bound = TC.grid_dist(grid[data], m["grid"][data])
    assert dist <= bound and np.all(grid[~(data | dm)] == 0)
    exact, bnd = PC.dmrs_exact(dict(c, dmrs=[int(v) for v in c["dmrs"]]))
    got = np.concatenate([grid[(sl + 1) * 7 - 4, 72:72 + 24] for sl in (0, 1)])
    assert PC.err("abs", got, exact) <= bnd
