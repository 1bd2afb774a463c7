"""The UE's sounding reference signal on the GPU (csrc/srs_kernel.hip) against what the reference's
srsran_refsignal_srs_gen / _put recorded (tests/golden/srs_golden.npz): the SRS-only branch of srsran_ue_ul_encode for
every case and subframe, the samples against the float64 model of the modulator and the normalisation, PUSCH + SRS
and PUCCH + SRS against the same subframe without the SRS, the batch bit-identical to single calls, the refusals, and
a C99 caller.

Bound of a row: srs_cases.srs_exact's, 1.5 ulp32 at the case's largest argument plus 2^-22 -- the bound the fixture's
generator holds both builds of the reference to.  The kernel forms the arguments as the recorded build does (alpha i
fused into the sum, one rounding), so it also lies within 2^-22 of a float64 evaluation at those arguments
(srs_cases.srs_rounded).  Samples: 2e-6 of the largest one, the bound of the modulator's own tests."""
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

import ofdm_np  # noqa: E402
import pucch_cases as C  # noqa: E402
import pucch_tx_cases as X  # noqa: E402
import pusch_tx_cases as TC  # noqa: E402
import srs_cases as SC  # noqa: E402
from srsran_4g_amd import tdec  # noqa: E402
from srsran_4g_amd import ue_ul as UL  # noqa: E402
from srsran_4g_amd.sch import srsran_uci_value_t  # noqa: E402
from test_ofdm_opts_gpu import TOL  # noqa: E402  (2e-6 of the largest sample: the same modulator)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    if not tdec.gpu_available():
        pytest.fail("no HIP device on a GPU test run")
    return SC.Fixture.get()


class Ues:
    """one srsran_ue_ul_t per cell"""

    def __init__(self):
        self.ues = {}

    def get(self, nof_prb, cell_id, cp, cell):
        key = (nof_prb, cell_id, cp)
        if key not in self.ues:
            self.ues[key] = UL.UeUl(cell)
        return self.ues[key]

    def of(self, c):
        return self.get(c["nof_prb"], c["cell_id"], c["cp"], SC.cell_of(c))

    def free(self):
        for ue in self.ues.values():
            ue.free()


@pytest.fixture(scope="module")
def ues():
    u = Ues()
    yield u
    u.free()


def sf_of(tti, shortened=False):
    sf = UL.srsran_ul_sf_cfg_t()
    sf.tti, sf.shortened = tti, shortened
    return sf


def comb_mask(c, k0, M):
    nsym, nre = 2 * SC.nsymb_slot(c["cp"]), 12 * c["nof_prb"]
    on = np.zeros((nsym, nre), bool)
    on[nsym - 1, k0:k0 + 2 * M:2] = True
    return on


def srs_only(ue, c, tti, **kw):
    """srsran_ue_ul_encode without a grant and without UCI -> (ret, samples, grid [2 nsym, 12 nof_prb])"""
    ucfg, sf = SC.ue_cfg(c, **kw), sf_of(tti)
    ret, x = ue.encode(sf, ucfg, None, srsran_uci_value_t())
    if ret != 1:
        return ret, None, None
    sbits, dsym, grid = ue.last()
    assert sbits.size == 0 and dsym.size == 0  # the grid alone, as after PUCCH
    return ret, x.copy(), grid.reshape(2 * SC.nsymb_slot(c["cp"]), -1).copy()


@pytest.mark.parametrize("c", SC.CASES, ids=[c["name"] for c in SC.CASES])
def test_srs_only_equals_the_recorded_rows(G, ues, c):
    ue, M = ues.of(c), G.m_sc(c)
    for i, tti in enumerate(c["ttis"]):
        ret, x, grid = srs_only(ue, c, tti)
        assert ret == 1, (c["name"], tti)
        on = comb_mask(c, G.k0(c)[i], M)
        assert np.all(grid[~on] == 0), (c["name"], tti)  # every other RE is zero
        want = G.rows(c)[i]
        _, bound, _ = SC.srs_exact(c, tti)
        dist = float(np.abs(grid[-1] - want).max())
        own = float(np.abs(grid[-1][on[-1]] - SC.srs_rounded(c, tti)).max())
        print("%s tti %d: row %.3e from the recording (bound %.3e), %.3e from the rounded-argument model" %
              (c["name"], tti, dist, bound, own))
        assert dist <= bound, (c["name"], tti, dist, bound)
        assert own <= 2.0 ** -22, (c["name"], tti, own)  # the arguments are the recorded build's, bit for bit
        assert np.abs(x).max() > 0


def srs_norm_factor(mode, peak_amp, nof_prb, M_sc, peak):
    """apply_norm / limit_norm_factor (ue_ul.c:246-299) from the SRS starting factor (float)nof_prb / 15 / sqrtf(M_sc)"""
    f32 = np.float32
    peak = f32(peak)
    if mode == 1:
        return f32((f32(peak_amp) if peak_amp > 0 else f32(1.0)) / peak)
    f = f32(f32(f32(nof_prb) / f32(15)) / np.sqrt(f32(M_sc)))
    if float(peak * f) > 0.95:
        f = f32(0.95 / float(peak))
    if float(peak * f) < 0.1:
        f = f32(0.1 / float(peak))
    return f


# (case, normalize mode, force_peak_amplitude, cfo_value or None)
RUNS = [("p6_phi24", 0, 0.0, None), ("p15_seqhop", 1, 0.6, 0.21), ("p25_m120", 0, 0.0, -0.4), ("p50_m288", 1, 0.0, None),
        ("p100_m576", 0, 0.0, 0.05), ("p15_extcp", 0, 0.0, 0.13)]


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_samples_match_the_float64_model(G, ues, run):
    name, mode, amp, cfo = run
    c = SC.BY_NAME[name]
    ue = ues.of(c)
    ret, x, grid = srs_only(ue, c, c["ttis"][0], mode=mode, peak=amp, cfo=cfo)
    assert ret == 1
    N, nre = ue.q.fft.cfg.symbol_sz, 12 * c["nof_prb"]
    assert x.size == 15 * N == ofdm_np.sf_len(N, c["cp"])
    y = ofdm_np.ofdm_tx_opts(grid.reshape(-1), N, nre, normalize=True, ext=c["cp"], freq_shift=0.5)
    if cfo is not None:
        f = float(np.float32(np.float32(cfo) / np.float32(N)))
        y = ofdm_np.ref_apply_cfo(np.asarray(y, np.complex64), f).astype(np.complex128)
    peak = max(np.abs(y.real).max(), np.abs(y.imag).max())
    fac = srs_norm_factor(mode, amp, c["nof_prb"], G.m_sc(c), peak)
    want = y * float(fac)
    err = float(np.abs(x - want).max() / np.abs(want).max())
    got_peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
    print(name, "samples: distance %.3e, bound %.3e; factor %.6g, peak %.6g" % (err, TOL, fac, got_peak))
    assert err <= TOL
    if mode == 1:
        assert got_peak == pytest.approx(amp if amp > 0 else 1.0, rel=1e-5)
    else:
        assert 0.1 * (1 - 1e-5) <= got_peak <= 0.95 * (1 + 1e-5)
    # only the last symbol carries energy
    n_last = N + (N // 4 if c["cp"] else (9 * N) // 128)
    assert not np.any(x[:x.size - n_last]) and np.abs(x[x.size - n_last:]).max() > 0


# ---- PUSCH + SRS in the 15-PRB cell of p15_seqhop (SRS region PRB 1 .. 12, the UE's SRS in tti 5)
def pusch_case(name, n_prb, L, shortened):
    c = SC.BY_NAME["p15_seqhop"]
    return TC.case(name, c["nof_prb"], c["cell_id"], L, n_prb, 2, 5, cp=c["cp"], tti=c["ttis"][0], shortened=shortened,
                   dmrs=tuple(c["dmrs"]), n_dmrs=2, seed=31)


def pusch_run(ue, pc, with_srs, keep):
    c = SC.BY_NAME["p15_seqhop"]
    cell, d, sf, cfg = TC.make(pc)
    payload, u = TC.payload_uci(pc, cfg)
    ucfg = TC.ue_cfg(pc, cfg, d)
    SC.ctypes_copy(ucfg.ul_cfg.srs, SC.srs_cfg(c, configured=with_srs))
    keep.extend([cfg, d, payload, u, ucfg, sf])
    ret, x = ue.encode(sf, ucfg, payload, u)
    assert ret == 1, pc["name"]
    sbits, dsym, grid = ue.last()
    assert dsym.size == cfg.grant.nof_re
    return x.copy(), grid.reshape(14, -1).copy(), ucfg, sf


@pytest.mark.parametrize("variant", ["shortened", "contiguous", "overwritten"])
def test_pusch_with_srs(G, ues, variant):
    """add_srs runs after the PUSCH and DMRS put whatever sf->shortened says: every RE off the comb equals the run with
    the SRS disabled, the comb holds the recorded row; where the caller leaves an overlapping PUSCH unshortened the
    comb REs of its last symbol are overwritten"""
    c = SC.BY_NAME["p15_seqhop"]
    tti, ue, keep = c["ttis"][0], ues.of(c), []
    pc = dict(shortened=pusch_case("ps", 6, 2, True), contiguous=pusch_case("pc", 13, 2, False),
              overwritten=pusch_case("po", 6, 2, False))[variant]
    # the helper gives the shortened flag a caller would pass (the overwritten variant ignores it on purpose)
    cell, d, sf, cfg = TC.make(pc)
    rule = UL.srs_pusch_shortened(cell, sf_of(tti), SC.srs_cfg(c), cfg)
    assert rule == (variant != "contiguous")
    x0, g0, _, _ = pusch_run(ue, pc, False, keep)
    x1, g1, _, sf1 = pusch_run(ue, pc, True, keep)
    assert bool(sf1.shortened) == pc["shortened"]  # the caller's, not rewritten
    on = comb_mask(c, G.k0(c)[0], G.m_sc(c))
    assert np.array_equal(g1[~on], g0[~on])
    _, bound, _ = SC.srs_exact(c, tti)
    assert np.abs(g1[-1] - G.rows(c)[0])[on[-1]].max() <= bound
    last_pusch = np.any(g0[-1] != 0)
    assert last_pusch == (not pc["shortened"])
    assert bool(np.any(g0[-1][on[-1]] != 0)) == (variant == "overwritten")
    assert not np.array_equal(x0, x1)
    # the same SRS as the SRS-only subframe of the same UE, bit for bit
    _, _, gs = srs_only(ue, c, tti)
    assert np.array_equal(gs[on], g1[on])


def pucch_run(ues, name, own_srs, keep):
    spec = next(sp for sp in C.Golden.get().cases if sp["name"] == name)
    s, cell, ucfg, v, sf = X.ue_setup(spec)
    if spec["fmt"] >= X.P.FORMAT_2:
        # the recorded format 2 resources lie in the outermost PRBs, where no valid SRS reaches: move this one to
        # m = 2 (PRB 1 in slot 0, PRB N_RB - 2 in slot 1), inside the SRS region
        ucfg.ul_cfg.pucch.n_rb_2, ucfg.ul_cfg.pucch.n_pucch_2 = 3, 24
    srs = ucfg.ul_cfg.srs
    srs.configured, srs.simul_ack, srs.subframe_config = True, True, 0
    srs.I_srs = (s["tti"] % 2) if own_srs else 1 - (s["tti"] % 2)
    srs.bw_cfg, srs.B, srs.b_hop, srs.k_tc, srs.n_srs, srs.n_rrc = 7, 0, 3, 1, 3, 0
    while srs.bw_cfg > 0 and SC.spec_row(s["nof_prb"], srs.bw_cfg - 1)[0][0] <= s["nof_prb"]:
        srs.bw_cfg -= 1  # the widest region that fits the cell
    ue = ues.get(s["nof_prb"], s["cell_id"], s["cp"], cell)
    keep.extend([ucfg, v, sf])
    ret, x = ue.encode(sf, ucfg, None, v)
    assert ret == 1, name
    return s, cell, ucfg, sf, x.copy(), ue.last()[2].reshape(2 * SC.nsymb_slot(s["cp"]), -1).copy()


@pytest.mark.parametrize("name", ["f1a_cp0_sh1", "f2_wb4_1"])
def test_pucch_with_srs(ues, name):
    """format 1a shortened by the rule with the SRS in the freed symbol; format 2 is never shortened and the SRS
    overwrites the comb REs of its last symbol where the two meet"""
    keep = []
    s, cell, u0, sf0, x0, g0 = pucch_run(ues, name, False, keep)
    s, cell, u1, sf1, x1, g1 = pucch_run(ues, name, True, keep)
    f1 = name.startswith("f1a")
    assert bool(sf0.shortened) == bool(sf1.shortened) == f1
    srs = u1.ul_cfg.srs
    k0, M = UL.srs_k0(cell, srs, s["tti"]), UL.srs_M_sc(cell, srs)
    on = comb_mask(s, k0, M)
    assert np.array_equal(g1[~on], g0[~on])
    over = int(np.count_nonzero(g0[on]))
    print(name, "comb REs that overwrite a PUCCH RE:", over)
    assert (over > 0) == (not f1)
    if f1:
        assert not np.any(g0[-1])  # the shortened format leaves the last symbol to the SRS
    ret, r = UL.srs_gen(cell, srs, u1.ul_cfg.dmrs, s["tti"] % 10)
    assert ret == 0 and np.abs(g1[on] - r[:M]).max() <= 2.0 ** -22  # the host sequence: the same arguments
    assert np.abs(np.abs(g1[on]) - 1).max() < 1e-6 and not np.array_equal(x0, x1)


def test_batch_bit_identical_to_single_calls(G, ues):
    """PUSCH, PUSCH + SRS, PUCCH, PUCCH + SRS, SRS-only entries of two cells and an entry with nothing to send in one
    batch, two orders: samples and grids equal the single calls bit for bit"""
    import torch
    keep = []

    def bufs(ue, nsym, nof_prb):
        d_out = torch.full((2 * ue.sf_len,), 5.0, dtype=torch.float32, device="cuda")
        d_grid = torch.full((2 * nsym * 12 * nof_prb,), 5.0, dtype=torch.float32, device="cuda")
        return d_out, d_grid

    def srs_entry(name, i, **kw):
        c = SC.BY_NAME[name]
        ue, ucfg, sf = ues.of(c), SC.ue_cfg(c, **kw), sf_of(c["ttis"][i])
        d_out, d_grid = bufs(ue, 2 * SC.nsymb_slot(c["cp"]), c["nof_prb"])
        keep.extend([ucfg, sf])
        return (ue, sf, ucfg, None, None, d_out.data_ptr(), d_grid.data_ptr()), d_out, d_grid

    def pusch_entry(pc, with_srs):
        c = SC.BY_NAME["p15_seqhop"]
        cell, d, sf, cfg = TC.make(pc)
        payload, u = TC.payload_uci(pc, cfg)
        ucfg = TC.ue_cfg(pc, cfg, d, mode=0, cfo=0.1)
        SC.ctypes_copy(ucfg.ul_cfg.srs, SC.srs_cfg(c, configured=with_srs))
        ue = ues.of(c)
        d_pl = torch.from_numpy(np.concatenate([payload, np.zeros(16, np.uint8)])).cuda()
        d_out, d_grid = bufs(ue, 14, c["nof_prb"])
        keep.extend([ucfg, u, sf, d_pl, cfg, d])
        return (ue, sf, ucfg, u, d_pl.data_ptr(), d_out.data_ptr(), d_grid.data_ptr()), d_out, d_grid

    def pucch_entry(name, own_srs):
        spec = next(sp for sp in C.Golden.get().cases if sp["name"] == name)
        s, cell, ucfg, v, sf = X.ue_setup(spec, mode=1, peak=0.7)
        srs = ucfg.ul_cfg.srs
        srs.configured, srs.simul_ack, srs.subframe_config = True, True, 0
        srs.I_srs = (s["tti"] % 2) if own_srs else 1 - (s["tti"] % 2)
        srs.bw_cfg, srs.B, srs.b_hop, srs.k_tc, srs.n_srs = 7, 0, 3, 0, 5
        ue = ues.get(s["nof_prb"], s["cell_id"], s["cp"], cell)
        d_out, d_grid = bufs(ue, 2 * SC.nsymb_slot(s["cp"]), s["nof_prb"])
        keep.extend([ucfg, v, sf])
        return (ue, sf, ucfg, v if any(bytes(v)) else None, None, d_out.data_ptr(), d_grid.data_ptr()), d_out, d_grid

    def empty_entry():
        c = SC.BY_NAME["p15_seqhop"]
        ue, ucfg, sf = ues.of(c), SC.ue_cfg(c), sf_of(c["ttis"][0] + 1)  # not an SRS subframe of the cell
        d_out, d_grid = bufs(ue, 14, c["nof_prb"])
        keep.extend([ucfg, sf])
        return (ue, sf, ucfg, None, None, d_out.data_ptr(), d_grid.data_ptr()), d_out, d_grid

    plan = {
        "srs15": lambda: srs_entry("p15_seqhop", 0, cfo=0.13),
        "pusch": lambda: pusch_entry(pusch_case("b0", 13, 2, False), False),
        "pusch+srs": lambda: pusch_entry(pusch_case("b1", 6, 2, True), True),
        "srs50a": lambda: srs_entry("p50_hop3", 1),
        "pucch": lambda: pucch_entry("f1a_cp0_sh1", False),
        "empty": empty_entry,
        "pucch+srs": lambda: pucch_entry("f2_wb4_1", True),
        "srs50b": lambda: srs_entry("p50_hop3", 4, mode=1, peak=0.5),
        "srs6": lambda: srs_entry("p6_phi24", 0),
    }
    single = {}
    for key, build in plan.items():
        e, d_out, d_grid = build()
        assert UL.tx_batch([e]) == 0, key
        torch.cuda.synchronize()
        single[key] = (d_out.cpu().numpy().copy(), d_grid.cpu().numpy().copy())
        assert (np.abs(single[key][0]).max() > 0) == (key != "empty"), key
        assert not np.any(single[key][0] == 5.0) and not np.any(single[key][1] == 5.0), key
    assert not np.array_equal(single["srs50a"][1], single["srs50b"][1])
    order = list(plan)
    for keys in (order, order[::-1]):
        built = [plan[k]() for k in keys]
        assert UL.tx_batch([b[0] for b in built]) == 0
        torch.cuda.synchronize()
        for k, (_, d_out, d_grid) in zip(keys, built):
            assert np.array_equal(d_out.cpu().numpy(), single[k][0]), k
            assert np.array_equal(d_grid.cpu().numpy(), single[k][1]), k
    # the single call of the host API gives the same samples
    c = SC.BY_NAME["p6_phi24"]
    _, x, _ = srs_only(ues.of(c), c, c["ttis"][0])
    assert np.array_equal(x.view(np.float32), single["srs6"][0])


def test_invalid_configurations_are_refused_with_nothing_written(ues):
    import torch
    c = SC.BY_NAME["p15_seqhop"]
    ue, tti = ues.of(c), c["ttis"][0]
    bad = [dict(bw_cfg=0), dict(bw_cfg=8), dict(B=4), dict(b_hop=4), dict(k_tc=2), dict(n_srs=8), dict(n_rrc=24)]
    ue.out[:] = 3.0
    for over in bad:
        ucfg, sf = SC.ue_cfg(c, **over), sf_of(tti)
        d = UL.make_data(None, srsran_uci_value_t())
        assert UL.lib().srsran_ue_ul_encode(ctypes.byref(ue.q), ctypes.byref(sf), ctypes.byref(ucfg), ctypes.byref(d)) == UL.ERROR
        assert np.all(ue.out == 3.0), over
    # a subframe that does not carry the SRS is not touched by the rule: nothing to send
    ucfg, sf = SC.ue_cfg(c, bw_cfg=0), sf_of(tti + 1)
    d = UL.make_data(None, srsran_uci_value_t())
    assert UL.lib().srsran_ue_ul_encode(ctypes.byref(ue.q), ctypes.byref(sf), ctypes.byref(ucfg), ctypes.byref(d)) == 0
    assert not np.any(ue.out)
    # the batch: an invalid entry refuses the whole call before anything is enqueued, in either position
    good, sfg = SC.ue_cfg(c), sf_of(tti)
    badc, sfb = SC.ue_cfg(c, bw_cfg=0), sf_of(tti)
    o1 = torch.full((2 * ue.sf_len,), 5.0, dtype=torch.float32, device="cuda")
    o2 = torch.full((2 * ue.sf_len,), 5.0, dtype=torch.float32, device="cuda")
    g1 = torch.full((2 * 14 * 12 * 15,), 5.0, dtype=torch.float32, device="cuda")
    for order in ((0, 1), (1, 0)):
        es = [(ue, sfg, good, None, None, o1.data_ptr(), g1.data_ptr()), (ue, sfb, badc, None, None, o2.data_ptr(), None)]
        assert UL.tx_batch([es[k] for k in order]) == UL.ERROR
        torch.cuda.synchronize()
        assert bool(torch.all(o1 == 5.0)) and bool(torch.all(o2 == 5.0)) and bool(torch.all(g1 == 5.0))
    # a grant in such a subframe is refused as well
    keep = []
    pc = pusch_case("r", 13, 2, False)
    cell, dm, sf, cfg = TC.make(pc)
    payload, u = TC.payload_uci(pc, cfg)
    ucfg = TC.ue_cfg(pc, cfg, dm)
    SC.ctypes_copy(ucfg.ul_cfg.srs, SC.srs_cfg(c, bw_cfg=0))
    keep.extend([cfg, dm, payload, u])
    assert ue.encode(sf, ucfg, payload, u)[0] == UL.ERROR
    # pregenerated signals and the CFR stay refused
    assert UL.lib().srsran_ue_ul_pregen_signals(ctypes.byref(ue.q), ctypes.byref(good)) == UL.ERROR
    assert UL.lib().srsran_ue_ul_set_cfr(ctypes.byref(ue.q), None) == UL.ERROR


C_CALLER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "srsran_ue_ul.h"

static uint32_t fnv(const void* p, size_t n)
{
  const uint8_t* b = (const uint8_t*)p;
  uint32_t       h = 2166136261u;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 16777619u;
  return h;
}

int main(void)
{
  srsran_cell_t cell;
  memset(&cell, 0, sizeof(cell));
  cell.nof_prb = 6; cell.nof_ports = 1; cell.id = 1; cell.cp = SRSRAN_CP_NORM;
  uint32_t len = SRSRAN_SF_LEN_PRB(cell.nof_prb);
  cf_t*    out = calloc(len, sizeof(cf_t));
  srsran_ue_ul_t q;
  if (srsran_ue_ul_init(&q, out, cell.nof_prb) || srsran_ue_ul_set_cell(&q, cell)) return 1;
  srsran_ue_ul_cfg_t cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.ul_cfg.srs.configured = true;
  cfg.ul_cfg.srs.bw_cfg = 7; /* the only one that fits 6 PRB */
  cfg.ul_cfg.srs.n_srs = 1;
  if (!srsran_refsignal_srs_cfg_isvalid(&cfg.ul_cfg.srs, cell.nof_prb)) return 2;
  srsran_ul_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  srsran_pusch_data_t data;
  memset(&data, 0, sizeof(data));
  sf.tti = 4; /* subframe_config 0, I_srs 0: every even subframe */
  if (srsran_ue_ul_encode(&q, &sf, &cfg, &data) != 1) return 3;
  printf("%u %u %u\n", (unsigned)srsran_refsignal_srs_k0_cell(&cell, &cfg.ul_cfg.srs, sf.tti),
         (unsigned)srsran_refsignal_srs_M_sc_cell(&cell, &cfg.ul_cfg.srs), fnv(out, len * sizeof(cf_t)));
  sf.tti = 5; /* not this UE's: nothing to send */
  if (srsran_ue_ul_encode(&q, &sf, &cfg, &data) != 0) return 4;
  printf("%u\n", fnv(out, len * sizeof(cf_t)));
  cfg.ul_cfg.srs.bw_cfg = 0; /* 36 PRB in a 6-PRB cell */
  sf.tti = 4;
  if (srsran_ue_ul_encode(&q, &sf, &cfg, &data) != SRSRAN_ERROR) return 5;
  srsran_ue_ul_free(&q);
  free(out);
  return 0;
}
'''


def test_c99_caller_sends_the_srs(G, ues):
    libdir = os.path.dirname(tdec.LIB_PATH)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "ue.c"), os.path.join(tmp, "ue")
        open(src, "w").write(C_CALLER)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
                            "-L", libdir, "-lsrsran_4g_amd", "-Wl,-rpath," + libdir, "-lm"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        got = [[int(x) for x in ln.split()] for ln in r.stdout.splitlines()]
    c = SC.BY_NAME["p6_phi24"]
    _, x, _ = srs_only(ues.of(c), c, 4)
    zero = np.zeros_like(x)
    assert got == [[G.k0(c)[0], G.m_sc(c), X.checksum(x)], [X.checksum(zero)]]
