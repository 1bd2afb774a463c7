"""The host side of the sounding reference signal (no GPU): the C helpers of include/srsran_ue_ul.h against the
reference's recorded k0 / M_sc / rows (tests/golden/srs_golden.npz) and against 36.211 5.5.3.2 / 5.5.3.3 and 36.213
Table 8.2-1 written out independently (tests/srs_cases.py), the shortened-PUSCH rule, the validity rule, the float64
estimator model tests/srs_np.py against every field the reference's estimator recorded, and the layout of the
configuration struct."""
import ctypes
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import srs_cases as SC  # noqa: E402
import srs_np  # noqa: E402
from srsran_4g_amd import sch as S  # noqa: E402
from srsran_4g_amd import ue_ul as UL  # noqa: E402


@pytest.fixture(scope="module")
def G():
    return SC.Fixture.get()


def all_ttis():
    return [(c, i, tti) for c in SC.CASES for i, tti in enumerate(c["ttis"])]


def test_measured_table_equals_the_fixture(G):
    assert G.measured == SC.MEASURED
    assert set(SC.MEASURED) == {"seq"} | {e["name"] for e in SC.EST_CASES}


def test_every_case_subframe_carries_the_srs_and_is_valid():
    L = UL.lib()
    for c, _, tti in all_ttis():
        assert SC.spec_valid(c) and UL.srs_cfg_isvalid(SC.srs_cfg(c), c["nof_prb"]), c["name"]
        assert L.srsran_refsignal_srs_send_cs(c["sfc"], tti % 10) == 1, (c["name"], tti)
        assert L.srsran_refsignal_srs_send_ue(c["I_srs"], tti) == 1, (c["name"], tti)
    assert len({(c["k_tc"], c["n_srs"]) for c in SC.CASES}) >= 8 and {c["k_tc"] for c in SC.CASES} == {0, 1}


def test_k0_and_m_sc_equal_the_reference(G):
    n = 0
    for c, i, tti in all_ttis():
        cell, srs = SC.cell_of(c), SC.srs_cfg(c)
        assert UL.srs_M_sc(cell, srs) == G.m_sc(c) == SC.spec_k0_msc(c, tti)[1], c["name"]
        assert UL.srs_k0(cell, srs, tti) == G.k0(c)[i] == SC.spec_k0_msc(c, tti)[0], (c["name"], tti)
        n += 1
    assert n == 31
    for name, period in (("p15_hop_n3", 3), ("p25_hop_n6", 6), ("p50_hop3", 12)):  # the hopping visits every position
        k0 = G.k0(SC.BY_NAME[name])
        assert len(set(k0[:period])) == period and k0[period] == k0[0], name


def test_k0_equals_the_specification_over_the_whole_configuration_space():
    """every bandwidth table, C_SRS, B, b_hop, both combs, n_RRC and a run of n_SRS; inside the cell in every case"""
    n = 0
    for nof_prb in (6, 15, 25, 40, 41, 50, 60, 61, 75, 80, 81, 100):
        cell = SC.cell_of(dict(nof_prb=nof_prb, cell_id=1, cp=0))
        for bw_cfg, B, b_hop, n_rrc in itertools.product(range(8), range(4), range(4), (0, 1, 5, 23)):
            c = dict(nof_prb=nof_prb, bw_cfg=bw_cfg, B=B, b_hop=b_hop, k_tc=(bw_cfg + B) % 2, n_srs=0, n_rrc=n_rrc, sfc=0,
                     I_srs=(0, 3, 9)[n_rrc % 3])
            srs = SC.srs_cfg(c)
            ok = SC.spec_valid(c)
            assert UL.srs_cfg_isvalid(srs, nof_prb) == ok, c
            if not ok:
                assert UL.srs_M_sc(cell, srs) == 0 and UL.srs_k0(cell, srs, 0) == 0
                continue
            for tti in (0, 2, 7, 10, 33, 64, 1000, 10239):
                k0, M = SC.spec_k0_msc(c, tti)
                assert (UL.srs_k0(cell, srs, tti), UL.srs_M_sc(cell, srs)) == (k0, M), (c, tti)
                assert k0 + 2 * (M - 1) < 12 * nof_prb and M >= 24
                n += 1
    assert n > 20000


def test_subframe_tables_equal_the_specification():
    L = UL.lib()
    for sfc, sf_idx in itertools.product(range(15), range(10)):
        assert L.srsran_refsignal_srs_send_cs(sfc, sf_idx) == int(SC.spec_send_cs(sfc, sf_idx)), (sfc, sf_idx)
    assert L.srsran_refsignal_srs_send_cs(15, 0) == UL.ERROR_INVALID_INPUTS
    assert L.srsran_refsignal_srs_send_cs(0, 10) == UL.ERROR_INVALID_INPUTS
    edges = sorted({i + d for i, _ in SC.SPEC_ISRS for d in (-1, 0, 1) if i + d >= 0} | {636, 637, 1023})
    for I_srs in edges:
        for tti in list(range(0, 700)) + [10239]:
            assert L.srsran_refsignal_srs_send_ue(I_srs, tti) == int(SC.spec_send_ue(I_srs, tti)), (I_srs, tti)
    # one SRS per period, at the offset, for every I_srs
    for I_srs in range(637):
        T, off = SC.spec_T(I_srs)
        hits = [t for t in range(off, off + 2 * T) if L.srsran_refsignal_srs_send_ue(I_srs, t) == 1]
        assert hits == [off, off + T], I_srs
    assert L.srsran_refsignal_srs_send_ue(1024, 0) == UL.ERROR_INVALID_INPUTS
    assert L.srsran_refsignal_srs_send_ue(0, 10240) == UL.ERROR_INVALID_INPUTS


def test_cell_region_helpers():
    L = UL.lib()
    for nof_prb, bw_cfg in itertools.product((6, 15, 25, 50, 75, 100), range(8)):
        m0 = SC.spec_row(nof_prb, bw_cfg)[0][0]
        assert L.srsran_refsignal_srs_rb_L_cs(bw_cfg, nof_prb) == m0
        assert L.srsran_refsignal_srs_rb_start_cs(bw_cfg, nof_prb) == (nof_prb // 2 - m0 // 2) % 2 ** 32
    assert L.srsran_refsignal_srs_rb_L_cs(8, 50) == 0 and L.srsran_refsignal_srs_rb_start_cs(8, 50) == 0


def test_validity_rule():
    base = SC.BY_NAME["p15_seqhop"]
    assert UL.srs_cfg_isvalid(SC.srs_cfg(base), 15)
    for key, bad in (("bw_cfg", 8), ("B", 4), ("b_hop", 4), ("k_tc", 2), ("n_srs", 8), ("n_rrc", 24), ("subframe_config", 15),
                     ("I_srs", 637)):
        assert not UL.srs_cfg_isvalid(SC.srs_cfg(base, **{key: bad}), 15), key
        assert UL.srs_cfg_isvalid(SC.srs_cfg(base, **{key: bad - 1}), 15), key
    # m_SRS,0 > N_RB: the reference's nof_prb / 2 - m_SRS,0 / 2 wraps there
    for nof_prb, bw_cfg, ok in ((6, 0, False), (6, 6, False), (6, 7, True), (15, 0, False), (15, 4, False), (15, 5, True),
                                (25, 1, False), (25, 2, True), (36, 0, True), (35, 0, False), (47, 0, False), (48, 0, True),
                                (71, 0, False), (72, 0, True), (95, 0, False), (96, 0, True), (100, 0, True)):
        assert UL.srs_cfg_isvalid(SC.srs_cfg(base, bw_cfg=bw_cfg), nof_prb) == ok, (nof_prb, bw_cfg)
    cell = SC.cell_of(dict(base, nof_prb=6))
    bad = SC.srs_cfg(base, bw_cfg=0)
    grid = np.full(14 * 72, 3 + 3j, np.complex64)
    assert UL.srs_put(cell, bad, 5, np.ones(600, np.complex64), grid) == UL.ERROR_INVALID_INPUTS
    assert UL.srs_get(cell, bad, 5, grid)[0] == UL.ERROR_INVALID_INPUTS
    assert UL.srs_gen(cell, bad, SC.dmrs_cfg(base), 5)[0] == UL.ERROR_INVALID_INPUTS
    assert np.all(grid == 3 + 3j)


def test_gen_put_get_equal_the_reference_rows(G):
    """the host sequence (both slots), its mapping and its extraction; the row is the sequence of slot 2 sf_idx"""
    worst = 0.0
    for c, i, tti in all_ttis():
        cell, srs, d = SC.cell_of(c), SC.srs_cfg(c), SC.dmrs_cfg(c)
        ret, r = UL.srs_gen(cell, srs, d, tti % 10)
        M, k0 = G.m_sc(c), G.k0(c)[i]
        assert ret == 0 and r.size == 2 * M
        rex, bound, _ = SC.srs_exact(c, tti)
        assert np.abs(r[:M] - rex).max() <= bound, c["name"]
        nsym, nre = 2 * SC.nsymb_slot(c["cp"]), 12 * c["nof_prb"]
        grid = np.full((nsym, nre), 3 + 3j, np.complex64)
        assert UL.srs_put(cell, srs, tti, r, grid) == 0
        on = np.zeros((nsym, nre), bool)
        on[nsym - 1, k0:k0 + 2 * M:2] = True
        assert np.all(grid[~on] == 3 + 3j) and np.array_equal(grid[on], r[:M])
        want = G.rows(c)[i]
        dist = float(np.abs(grid[nsym - 1][on[nsym - 1]] - want[on[nsym - 1]]).max())
        worst = max(worst, dist)
        assert dist <= bound, (c["name"], dist, bound)
        assert not np.any(want[~on[nsym - 1]])
        ret, back = UL.srs_get(cell, srs, tti, grid)
        assert ret == 0 and np.array_equal(back, r[:M])
    print("host rows: largest distance from the recorded ones %.3e" % worst)
    # the quirk is visible: with group hopping the two slot sequences differ, and the row holds the first
    c = SC.BY_NAME["p15_grouphop"]
    _, r = UL.srs_gen(SC.cell_of(c), SC.srs_cfg(c), SC.dmrs_cfg(c), c["ttis"][0] % 10)
    M = G.m_sc(c)
    assert np.abs(r[:M] - r[M:]).max() > 0.5


def test_pusch_shortened_rule(G):
    import make_srs_golden as MK
    assert len(MK.SHORT_CASES) == G.z["short"].size
    seen = set()
    for (name, tti, nt, L_prb, rar), want in zip(MK.SHORT_CASES, G.z["short"]):
        c = SC.BY_NAME[name]
        for before in (False, True):
            pc = S.srsran_pusch_cfg_t()
            pc.grant.n_prb_tilde[0], pc.grant.n_prb_tilde[1], pc.grant.L_prb, pc.grant.is_rar = nt[0], nt[1], L_prb, bool(rar)
            sf = UL.srsran_ul_sf_cfg_t()
            sf.tti, sf.shortened = tti, before
            assert UL.srs_pusch_shortened(SC.cell_of(c), sf, SC.srs_cfg(c), pc) == bool(want), (name, tti, nt, L_prb, rar)
        seen.add(int(want))
    assert seen == {0, 1}
    # what the list must contain: overlapping, contiguous left and right, disjoint, a RAR grant
    want = dict(zip([x[1:] for x in MK.SHORT_CASES], G.z["short"]))
    assert want[(5, (3, 3), 4, 0)] == 1 and want[(5, (13, 13), 2, 0)] == 0 and want[(5, (0, 0), 1, 0)] == 0
    assert want[(5, (14, 14), 1, 0)] == 1 and want[(5, (3, 3), 4, 1)] == 0 and want[(10, (14, 14), 1, 0)] == 0
    # not configured: never
    c = SC.BY_NAME["p15_seqhop"]
    pc = S.srsran_pusch_cfg_t()
    pc.grant.n_prb_tilde[0], pc.grant.n_prb_tilde[1], pc.grant.L_prb = 3, 3, 4
    sf = UL.srsran_ul_sf_cfg_t()
    sf.tti, sf.shortened = 5, True
    assert UL.srs_pusch_shortened(SC.cell_of(c), sf, SC.srs_cfg(c, configured=False), pc) is False


def test_float64_estimator_model_equals_the_reference(G):
    """tests/srs_np.py on the recorded inputs against every field the reference's estimator returned: within the
    measured distance of the two builds (x 1.0001 for the table's own rounding), ta_us and the special values exactly"""
    for e in SC.EST_CASES:
        c = SC.BY_NAME[e["of"]]
        tti = c["ttis"][0]
        k0, M = G.k0(c)[0], G.m_sc(c)
        y = G.z["rx." + e["name"]]
        r = G.rows(c)[0][k0:k0 + 2 * M:2]  # the sequence build 1 sent is the one its estimator generates
        m = srs_np.estimate(srs_np.comb(y, k0, M), r, e["smooth"])
        sc = dict(zip(SC.SCALARS, G.z["scal." + e["name"]]))
        tol = SC.MEASURED[e["name"]] * 1.0001
        assert np.isnan(sc["cfo_hz"]) and np.isnan(m["cfo_hz"])
        assert sc["ta_us"] == np.float32(m["ta_us"]), e["name"]
        assert abs(abs(m["ta_raw"]) * 10 % 1 - 0.5) >= 0.2
        # chest_ul.c:644: a pilot spacing of 1 on a comb of 2 -- twice the applied delay (plus the channel's own)
        assert abs(m["ta_raw"] - 2 * e["ta_us"]) < 0.08, (e["name"], m["ta_raw"])
        for key in SC.SCALARS[:8]:
            if np.isnan(m[key]) or np.isinf(m[key]) or m[key] == 0:
                assert (np.isnan(sc[key]) and np.isnan(m[key])) or sc[key] == m[key], (e["name"], key)
            else:
                assert abs(float(sc[key]) - m[key]) <= tol * abs(m[key]), (e["name"], key, sc[key], m[key])
        ce = G.z["ce." + e["name"]]
        assert ce.size == M and np.abs(ce - m["ce"]).max() <= tol * np.abs(m["ce"]).max(), e["name"]
        if e["smooth"] == 0:
            assert sc["noise_estimate"] == 0 and np.isnan(sc["snr"])
    assert {e["smooth"] for e in SC.EST_CASES} == {0, 3} and any(e["snr_db"] is None for e in SC.EST_CASES)


LAYOUT_C = r'''
#include <stddef.h>
#include <stdio.h>
#include "srsran_ue_ul.h"
int main(void)
{
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(srsran_refsignal_srs_cfg_t), offsetof(srsran_refsignal_srs_cfg_t, simul_ack),
         offsetof(srsran_refsignal_srs_cfg_t, B), offsetof(srsran_refsignal_srs_cfg_t, n_rrc),
         offsetof(srsran_refsignal_srs_cfg_t, dedicated_enabled), offsetof(srsran_refsignal_srs_cfg_t, configured),
         offsetof(srsran_ue_ul_cfg_t, ul_cfg.srs));
  return 0;
}
'''


def test_struct_layout_of_the_srs_configuration():
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "l.c"), os.path.join(tmp, "l")
        open(src, "w").write(LAYOUT_C)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    T = UL.srsran_refsignal_srs_cfg_t
    assert got == [ctypes.sizeof(T), T.simul_ack.offset, T.B.offset, T.n_rrc.offset, T.dedicated_enabled.offset,
                   T.configured.offset, UL.srsran_ue_ul_cfg_t.ul_cfg.offset + UL.srsran_ul_cfg_t.srs.offset]
