"""PUCCH transmit on the GPU (csrc/pucch_tx_kernel.hip) against the grids the reference's own transmitter recorded
(tests/golden/pucch_golden.npz, clean_<i>): the encode level (srsran_pucch_encode + the DMRS calls on a host grid),
the UE level (srsran_ue_ul_encode without a grant, the grid read back through srsran_ue_ul_gpu_last), the samples
against the float64 model of tests/test_ue_ul_gpu.py, the batch bit-identical to single calls with PUSCH entries
interleaved, the refusals and branches, and a C99 caller.

Bound of the grids: 1e-6 max|clean_<i>|, the bound test_numpy_transmitter_equals_the_reference_grids applies to the
numpy transmitter on the same recordings.  Measured on an MI355X: encode level 2.07e-07 (f3_cp0_sh1), UE level
1.79e-07 (f1b_cp0_sh1); the samples lie 2.2e-07 .. 2.7e-07 from the model against the 2e-6 of the modulator's tests."""
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
import pucch_tx as T  # noqa: E402
import pucch_tx_cases as X  # noqa: E402
import pusch_tx_cases as TC  # noqa: E402
from srsran_4g_amd import pucch as P  # noqa: E402
from srsran_4g_amd import tdec  # noqa: E402
from srsran_4g_amd import ue_ul as UL  # noqa: E402
from srsran_4g_amd.sch import srsran_uci_value_t  # noqa: E402
from test_ofdm_opts_gpu import TOL  # noqa: E402  (2e-6 of the largest sample: the same modulator)

pytestmark = pytest.mark.gpu

F3_SHORTENED = ("f3_cp0_sh1", "f3_cp1_sh1")  # the rule clears shortened for format >= 2: encode level only


@pytest.fixture(scope="module")
def G():
    if not tdec.gpu_available():
        pytest.fail("no HIP device on a GPU test run")
    return C.Golden.get()


class Ues:
    """one srsran_ue_ul_t per cell of the fixture"""

    def __init__(self):
        self.ues = {}

    def get(self, s, cell):
        key = (s["nof_prb"], s["cell_id"], s["cp"])
        if key not in self.ues:
            self.ues[key] = UL.UeUl(cell)
        return self.ues[key]

    def free(self):
        for ue in self.ues.values():
            ue.free()


@pytest.fixture(scope="module")
def ues():
    u = Ues()
    yield u
    u.free()


def test_encode_level_equals_the_recorded_grids(G):
    """srsran_pucch_encode + srsran_refsignal_dmrs_pucch_gen_cell + _put_cell on a host grid full of a sentinel"""
    LP = P.lib()
    objs, n, worst = {}, 0, (0.0, "")
    try:
        for i, spec in X.tx_cases(G):
            s, cell, cfg, v2, sf = X.tx_setup(spec)
            assert (cfg.format, cfg.n_pucch) == (spec["fmt"], spec["n_pucch"]), spec["name"]
            key = (s["nof_prb"], s["cell_id"], s["cp"])
            if key not in objs:
                objs[key] = P.PucchUe(cell)
                assert objs[key].q.is_ue
            want = G.z[f"clean_{i}"].reshape(2 * T.nsym(s["cp"]), -1)
            grid = np.full(want.shape, X.SENTINEL, np.complex64)
            data, rs = X.masks(s, cfg.format, cfg.n_pucch, bool(s["shortened"]))
            assert objs[key].encode(sf, cfg, v2, grid) == 0, spec["name"]
            assert np.all(grid[~data] == X.SENTINEL), spec["name"]  # only the data REs are written
            if cfg.format in (P.FORMAT_2A, P.FORMAT_2B):
                nb = cfg.format - P.FORMAT_2
                assert list(cfg.pucch2_drs_bits)[:nb] == list(G.z[f"tx_ack_{i}"])[:nb], spec["name"]
            ret, _ = objs[key].put_dmrs(sf, cfg, grid)
            assert ret == 0, spec["name"]
            assert np.all(grid[~(data | rs)] == X.SENTINEL), spec["name"]
            d = float(np.abs(grid[data | rs] - want[data | rs]).max() / np.abs(want).max())
            worst = max(worst, (d, spec["name"]))
            assert d <= X.BOUND, (spec["name"], d)
            assert not np.any(want[~(data | rs)])  # the recording has nothing outside these REs either
            n += 1
        # an n_prb outside the cell and an unsupported format are errors; NULL is invalid input
        s, cell, cfg, v2, sf = X.tx_setup(G.cases[1])
        q = objs[(s["nof_prb"], s["cell_id"], s["cp"])]
        grid = np.full((14, 72), X.SENTINEL, np.complex64)
        cfg.format, cfg.n_pucch = P.FORMAT_2, 12 * 14
        assert q.encode(sf, cfg, v2, grid) == -1
        cfg.format, cfg.n_pucch = P.FORMAT_ERROR, 0
        assert q.encode(sf, cfg, v2, grid) == -1
        assert LP.srsran_pucch_encode(ctypes.byref(q.q), ctypes.byref(sf), ctypes.byref(cfg), None, X.ptr(grid)) == -2
        assert LP.srsran_pucch_encode(ctypes.byref(q.q), ctypes.byref(sf), ctypes.byref(cfg), ctypes.byref(v2), None) == -2
        assert np.all(grid == X.SENTINEL)
    finally:
        for q in objs.values():
            q.free()
    print("encode level: largest distance %.3e of max|clean| (%s), bound %.0e, %d cases" % (worst + (X.BOUND, n)))
    assert n >= 70 and len(objs) == 5


def test_ue_level_equals_the_recorded_grids(G, ues):
    """srsran_ue_ul_encode without a grant: format / resource written, the grid of srsran_ue_ul_gpu_last equal to the
    recording and zero elsewhere, the caller's UCI value unchanged, shortened written by the rule"""
    n, skipped, worst = 0, [], (0.0, "")
    for i, spec in X.tx_cases(G):
        if spec["name"] in F3_SHORTENED:
            skipped.append(spec["name"])
            continue
        s, cell, ucfg, v, sf = X.ue_setup(spec)
        ue = ues.get(s, cell)
        d = UL.make_data(None, v)
        before = bytes(d.uci)
        ret = UL.lib().srsran_ue_ul_encode(ctypes.byref(ue.q), ctypes.byref(sf), ctypes.byref(ucfg), ctypes.byref(d))
        assert ret == 1, spec["name"]
        pc = ucfg.ul_cfg.pucch
        assert (pc.format, pc.n_pucch) == (spec["fmt"], spec["n_pucch"]), spec["name"]
        assert bytes(d.uci) == before, spec["name"]
        assert bool(sf.shortened) == bool(s["shortened"]), spec["name"]
        sbits, dsym, grid = ue.last()
        assert sbits.size == 0 and dsym.size == 0
        want = G.z[f"clean_{i}"].reshape(2 * T.nsym(s["cp"]), -1)
        grid = grid.reshape(want.shape)
        on = np.logical_or(*X.masks(s, pc.format, pc.n_pucch, bool(s["shortened"])))
        dist = float(np.abs(grid - want).max() / np.abs(want).max())
        worst = max(worst, (dist, spec["name"]))
        assert dist <= X.BOUND, (spec["name"], dist)
        assert np.all(grid[~on] == 0), spec["name"]
        assert np.abs(ue.out[:ue.sf_len]).max() > 0
        n += 1
    print("UE level: largest distance %.3e of max|clean| (%s), bound %.0e, %d cases" % (worst + (X.BOUND, n)))
    assert sorted(skipped) == sorted(F3_SHORTENED) and n == len(X.tx_cases(G)) - 2 and n >= 68


def pucch_norm_factor(mode, peak_amp, nof_prb, peak):
    """apply_norm / limit_norm_factor (ue_ul.c:246-299) from the PUCCH starting factor (float)nof_prb / 15 / 10"""
    f32 = np.float32
    peak = f32(peak)
    if mode == 1:
        return f32((f32(peak_amp) if peak_amp > 0 else f32(1.0)) / peak)
    f = f32(f32(f32(nof_prb) / f32(15)) / f32(10))
    if float(peak * f) > 0.95:
        f = f32(0.95 / float(peak))
    if float(peak * f) < 0.1:
        f = f32(0.1 / float(peak))
    return f


# (case, normalize mode, force_peak_amplitude, cfo_value or None): the format families, both cyclic prefixes
RUNS = [("f1a_cp0_sh0", 0, 0.0, None), ("f1b_cp1_sh1", 1, 0.6, 0.21), ("f2_wb4_1", 0, 0.0, -0.4),
        ("f2b_01", 1, 0.0, None), ("f3_cp0_sh0", 0, 0.0, 0.05), ("f3_cp1_sh0", 1, 0.8, None), ("prb25_m3", 0, 0.0, 0.13)]


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_samples_match_the_float64_model(G, ues, run):
    name, mode, amp, cfo = run
    spec = next(sp for sp in G.cases if sp["name"] == name)
    s, cell, ucfg, v, sf = X.ue_setup(spec, mode=mode, peak=amp, cfo=cfo)
    ue = ues.get(s, cell)
    ret, x = ue.encode(sf, ucfg, None, v)
    assert ret == 1
    x = x.copy()
    grid = ue.last()[2]
    N, nre = ue.q.fft.cfg.symbol_sz, 12 * s["nof_prb"]
    assert x.size == 15 * N == ofdm_np.sf_len(N, s["cp"])
    y = ofdm_np.ofdm_tx_opts(grid, N, nre, normalize=True, ext=s["cp"], freq_shift=0.5)
    if cfo is not None:
        f = float(np.float32(np.float32(cfo) / np.float32(N)))
        y = ofdm_np.ref_apply_cfo(np.asarray(y, np.complex64), f).astype(np.complex128)
    peak = max(np.abs(y.real).max(), np.abs(y.imag).max())
    fac = pucch_norm_factor(mode, amp, s["nof_prb"], peak)
    want = y * float(fac)
    err = float(np.abs(x - want).max() / np.abs(want).max())
    got_peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
    print(name, "samples: distance %.3e, bound %.3e; factor %.6g, peak %.6g" % (err, TOL, fac, got_peak))
    assert err <= TOL
    if mode == 1:
        assert got_peak == pytest.approx(amp if amp > 0 else 1.0, rel=1e-5)
    else:
        assert 0.1 * (1 - 1e-5) <= got_peak <= 0.95 * (1 + 1e-5)


def test_batch_bit_identical_to_single_calls(G, ues):
    """every case as one entry of one batch, the five cells as five objects, three PUSCH entries and one entry with
    nothing to send interleaved, two orders; samples and grids equal the single calls bit for bit"""
    import torch
    keep, pusch_ues = [], {}
    try:
        def pucch_entry(k, spec):
            s, cell, ucfg, v, sf = X.ue_setup(spec, mode=k % 2, peak=0.7, cfo=0.13 if k % 3 == 0 else None)
            ue = ues.get(s, cell)
            d_out = torch.full((2 * ue.sf_len,), 5.0, dtype=torch.float32, device="cuda")
            d_grid = torch.full((2 * 2 * T.nsym(s["cp"]) * 12 * s["nof_prb"],), 5.0, dtype=torch.float32, device="cuda")
            keep.extend([ucfg, v, sf])
            uci = v if any(bytes(v)) else None  # uci == NULL stands for an all-zero value
            return (ue, sf, ucfg, uci, None, d_out.data_ptr(), d_grid.data_ptr()), d_out, d_grid

        def pusch_entry(name):
            c = TC.BY_NAME[name]
            cell, d, sf, cfg = TC.make(c)
            if name not in pusch_ues:
                pusch_ues[name] = UL.UeUl(cell)
            ue = pusch_ues[name]
            payload, u = TC.payload_uci(c, cfg)
            ucfg = TC.ue_cfg(c, cfg, d, mode=0, cfo=0.1)
            d_pl = torch.from_numpy(np.concatenate([payload, np.zeros(16, np.uint8)])).cuda()
            d_out = torch.full((2 * ue.sf_len,), 5.0, dtype=torch.float32, device="cuda")
            d_grid = torch.full((2 * 14 * 12 * c["nof_prb"],), 5.0, dtype=torch.float32, device="cuda")
            keep.extend([ucfg, u, sf, d_pl, cfg, d])
            return (ue, sf, ucfg, u, d_pl.data_ptr(), d_out.data_ptr(), d_grid.data_ptr()), d_out, d_grid

        def empty_entry():
            s, cell, ucfg, v, sf = X.ue_setup(G.cases[1])
            for a in ucfg.ul_cfg.pucch.uci_cfg.ack:
                a.nof_acks = 0
            ue = ues.get(s, cell)
            d_out = torch.full((2 * ue.sf_len,), 5.0, dtype=torch.float32, device="cuda")
            d_grid = torch.full((2 * 14 * 12 * s["nof_prb"],), 5.0, dtype=torch.float32, device="cuda")
            keep.extend([ucfg, sf])
            return (ue, sf, ucfg, None, None, d_out.data_ptr(), d_grid.data_ptr()), d_out, d_grid

        cases = [sp for _, sp in X.tx_cases(G) if sp["name"] not in F3_SHORTENED]
        assert len(cases) >= 68
        # the build list: ("pucch", k) / ("pusch", name) / ("empty",)
        plan = [("pucch", k) for k in range(len(cases))]
        plan.insert(3, ("pusch", "t1"))
        plan.insert(20, ("pusch", "t2"))
        plan.insert(41, ("pusch", "t7"))
        plan.insert(30, ("empty",))

        def build(item):
            if item[0] == "pucch":
                return pucch_entry(item[1], cases[item[1]])
            return pusch_entry(item[1]) if item[0] == "pusch" else empty_entry()

        single = {}
        for item in plan:
            e, d_out, d_grid = build(item)
            assert UL.tx_batch([e]) == 0, item
            torch.cuda.synchronize()
            single[item] = (d_out.cpu().numpy().copy(), d_grid.cpu().numpy().copy())
            assert (np.abs(single[item][0]).max() > 0) == (item[0] != "empty"), item
            assert not np.any(single[item][0] == 5.0) and not np.any(single[item][1] == 5.0), item
        for order in (plan, plan[::-1]):
            built = [build(item) for item in order]
            assert UL.tx_batch([b[0] for b in built]) == 0
            torch.cuda.synchronize()
            for item, (_, d_out, d_grid) in zip(order, built):
                assert np.array_equal(d_out.cpu().numpy(), single[item][0]), item
                assert np.array_equal(d_grid.cpu().numpy(), single[item][1]), item
        assert not np.any(single[("empty",)][0]) and not np.any(single[("empty",)][1])
    finally:
        for ue in pusch_ues.values():
            ue.free()


def test_refusals_and_branches(G, ues):
    L = UL.lib()
    spec = G.cases[1]  # f1a_cp0_sh0, tti 4

    def run(change, value=None):
        s, cell, ucfg, v, sf = X.ue_setup(spec)
        if value is not None:
            v = value
        change(ucfg)
        ue = ues.get(s, cell)
        d = UL.make_data(None, v)
        ret = L.srsran_ue_ul_encode(ctypes.byref(ue.q), ctypes.byref(sf), ctypes.byref(ucfg), ctypes.byref(d))
        return ret, ue, ucfg, d

    assert run(lambda u: None)[0] == 1
    assert run(lambda u: setattr(u.ul_cfg.pucch, "rnti", 0))[0] == UL.ERROR
    assert run(lambda u: setattr(u.ul_cfg.pucch, "delta_pucch_shift", 0))[0] == UL.ERROR
    ret, ue, _, _ = run(lambda u: setattr(u, "cc_idx", 1))  # not the PCell: not the PUCCH branch
    assert ret == 0 and not np.any(ue.out)

    def own_srs(u):  # subframe_config 0: every subframe; I_srs 0: period 2, offset 0; tti 4 is this UE's
        u.ul_cfg.srs.configured, u.ul_cfg.srs.subframe_config, u.ul_cfg.srs.I_srs = True, 0, 0
    assert run(own_srs)[0] == UL.ERROR
    # a format selection that yields SRSRAN_PUCCH_FORMAT_ERROR: five HARQ-ACK bits without channel selection
    assert run(lambda u: setattr(u.ul_cfg.pucch.uci_cfg.ack[0], "nof_acks", 5))[0] == UL.ERROR

    # DTX (2) becomes NACK in a feedback mode other than NORMAL; all DTX clears nof_acks of the PUSCH configuration
    cs = next(sp for sp in G.cases if sp["name"] == "cs2_0")

    def run_cs(acks):
        s, cell, ucfg, v, sf = X.ue_setup(cs)
        assert ucfg.ul_cfg.pucch.ack_nack_feedback_mode != 0
        ucfg.ul_cfg.pusch.uci_cfg.ack[0].nof_acks = 2
        for k, a in enumerate(acks):
            v.ack.ack_value[k] = a
        ue = ues.get(s, cell)
        d = UL.make_data(None, v)
        ret = L.srsran_ue_ul_encode(ctypes.byref(ue.q), ctypes.byref(sf), ctypes.byref(ucfg), ctypes.byref(d))
        return ret, ue.last()[2].copy(), ucfg, d

    ret, g_dtx, ucfg, d = run_cs([2, 1])
    assert ret == 1 and list(d.uci.ack.ack_value)[:2] == [0, 1] and ucfg.ul_cfg.pusch.uci_cfg.ack[0].nof_acks == 2
    ret, g_nack, _, _ = run_cs([0, 1])
    assert ret == 1 and np.array_equal(g_dtx, g_nack)
    ret, _, ucfg, d = run_cs([2, 2])
    assert ret == 1 and list(d.uci.ack.ack_value)[:2] == [0, 0]
    assert all(a.nof_acks == 0 for a in ucfg.ul_cfg.pusch.uci_cfg.ack)
    # the batch: an invalid PUCCH entry refuses the whole call before anything is written
    import torch
    s, cell, ucfg, v, sf = X.ue_setup(spec)
    ucfg.ul_cfg.pucch.rnti = 0
    ue = ues.get(s, cell)
    d_out = torch.full((2 * ue.sf_len,), 5.0, dtype=torch.float32, device="cuda")
    assert UL.tx_batch([(ue, sf, ucfg, v, None, d_out.data_ptr(), None)]) == UL.ERROR
    torch.cuda.synchronize()
    assert bool(torch.all(d_out == 5.0))


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
  cfg.ul_cfg.pucch.rnti = 0x46;
  cfg.ul_cfg.pucch.delta_pucch_shift = 1;
  cfg.ul_cfg.pucch.simul_cqi_ack = true;
  cfg.ul_cfg.pucch.n_pucch_2 = 3;
  srsran_ul_sf_cfg_t sf;
  memset(&sf, 0, sizeof(sf));
  srsran_pusch_data_t data;
  memset(&data, 0, sizeof(data));
  /* format 1a: one HARQ-ACK bit, n_cce 5 */
  sf.tti = 4;
  cfg.ul_cfg.pucch.uci_cfg.ack[0].nof_acks = 1;
  cfg.ul_cfg.pucch.uci_cfg.ack[0].ncce[0] = 5;
  data.uci.ack.ack_value[0] = 1;
  if (srsran_ue_ul_encode(&q, &sf, &cfg, &data) != 1 || cfg.ul_cfg.pucch.format != SRSRAN_PUCCH_FORMAT_1A) return 2;
  printf("%u %u\n", (unsigned)cfg.ul_cfg.pucch.n_pucch, fnv(out, len * sizeof(cf_t)));
  /* format 2: a wideband CQI report */
  sf.tti = 9;
  cfg.ul_cfg.pucch.uci_cfg.ack[0].nof_acks = 0;
  cfg.ul_cfg.pucch.uci_cfg.cqi.data_enable = true;
  cfg.ul_cfg.pucch.uci_cfg.cqi.type = SRSRAN_CQI_TYPE_WIDEBAND;
  data.uci.ack.ack_value[0] = 0;
  data.uci.cqi.wideband.wideband_cqi = 11;
  if (srsran_ue_ul_encode(&q, &sf, &cfg, &data) != 1 || cfg.ul_cfg.pucch.format != SRSRAN_PUCCH_FORMAT_2) return 3;
  printf("%u %u\n", (unsigned)cfg.ul_cfg.pucch.n_pucch, fnv(out, len * sizeof(cf_t)));
  srsran_ue_ul_free(&q);
  free(out);
  return 0;
}
'''


def test_c99_caller_sends_format_1a_and_format_2(G):
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
    from srsran_4g_amd.ue_dl import cell as make_cell
    ue = UL.UeUl(make_cell(6, 1, 1))
    try:
        want = []
        for tti, acks, cqi in ((4, [[1, 5, 0, 0]], None), (9, [], (0, 0, 0))):
            cfg = C.build_cfg(dict(acks=acks, cqi=cqi, n_pucch_2=3))
            ucfg = UL.srsran_ue_ul_cfg_t()
            for k in ("rnti", "delta_pucch_shift", "simul_cqi_ack", "n_pucch_2"):
                setattr(ucfg.ul_cfg.pucch, k, getattr(cfg, k))
            ctypes.memmove(ctypes.byref(ucfg.ul_cfg.pucch.uci_cfg), ctypes.byref(cfg.uci_cfg), ctypes.sizeof(cfg.uci_cfg))
            v = srsran_uci_value_t()
            if acks:
                v.ack.ack_value[0] = 1
            else:
                v.cqi.wideband.wideband_cqi = 11
            sf = C.build_sf(dict(tti=tti))
            ret, x = ue.encode(sf, ucfg, None, v)
            assert ret == 1
            want.append([ucfg.ul_cfg.pucch.n_pucch, X.checksum(x)])
    finally:
        ue.free()
    assert got == want
