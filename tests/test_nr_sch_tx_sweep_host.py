"""CPU checks of the NR SCH transmit sweep's case lists (nr_sch_tx_sweep_cases.py) against the compiled
reference: the counts the lists must have, that the row edges straddle their boundaries, and that the slice-edge
payload lengths and the C > 1 pairs are what the reference's segmentation gives."""
import numpy as np
import pytest

import nr_sch_tx_sweep_cases as K
from nr_sch import RefNr, ref_available

pytestmark = pytest.mark.skipif(not ref_available(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def ref():
    return RefNr()


@pytest.fixture(scope="module")
def shapes(ref):
    return K.reachable_shapes(ref.tb_info)


def test_reachable_shapes(ref, shapes):
    assert len(shapes) == 84
    bg1 = sorted(Z for bg, Z in shapes if bg == 0)
    bg2 = sorted(Z for bg, Z in shapes if bg == 1)
    assert len(bg1) == 38 and bg1[0] == 15
    all_Z = sorted(a << j for a in (2, 3, 5, 7, 9, 11, 13, 15) for j in range(8) if a << j <= 384)
    assert len(all_Z) == 51 and len(bg2) == 46 and bg2 == [Z for Z in all_Z if Z not in (2, 3, 5, 9, 13)]
    assert bg1 == [Z for Z in all_Z if Z >= 15]
    assert sum(len(v) for v in shapes.values()) == 156
    for (bg, Z), v in shapes.items():
        for s in v:
            t = ref.tb_info(s.tbs, s.R, 1, 8 * s.tbs, 1)
            assert (t["bg"], t["Z"], t["C"], t["F"], t["Kp"], t["Kr"]) == (bg, Z, 1, s.F, s.Kp, s.Kr)
            assert s.Kr == Z * K.BG_K[bg] and s.tbs % 8 == 0
        assert len(v) == 1 or v[0].F < v[1].F
    # the four high-rate solutions: BG1 set index 6 and other, BG2 set indices 3 / 7 and other
    assert {K.hr_case(bg, Z) for bg, Z in shapes} == {1, 2, 3, 4}
    assert {K.set_index(Z) for bg, Z in shapes if bg == 1 and K.hr_case(bg, Z) == 3} == {3, 7}
    assert {K.set_index(Z) for bg, Z in shapes if bg == 0 and K.hr_case(bg, Z) == 2} == {6}
    # fillers over more than two whole chunks
    for bg in (0, 1):
        assert any(s.F > 2 * Z for (b, Z), v in shapes.items() if b == bg for s in v), bg
    assert sorted(Z for (b, Z), v in shapes.items() if b == 0 and v[-1].F > 2 * Z) == [36, 72, 80, 144, 160, 288, 320]


def test_lifting_items_meet_every_modulation(shapes):
    items = K.lifting_items(shapes)
    assert len(items) == 2 * 156
    assert {(K.hr_case(i["bg"], i["Z"]), i["Qm"]) for i in items} == {(c, q) for c in (1, 2, 3, 4) for q in K.QMS}
    for i in items:
        N = i["Z"] * K.BG_N[i["bg"]]
        assert i["G"] % i["Qm"] == 0 and (i["G"] >= 1.3 * N if i["kind"] == "long" else i["G"] < N)
    assert {(i["bg"], i["Z"]) for i in items} == set(shapes)
    # both launch widths have work
    assert len({(i["bg"], i["Z"]) for i in items if i["Z"] <= 32}) == 28  # 10 of BG1, 18 of BG2
    assert len({(i["bg"], i["Z"]) for i in items if i["Z"] > 32}) == 56


def test_lbrm_items(ref, shapes):
    t = ref.tb_info(8424, 0.5, 2, 30000, 1, lbrm=True, nof_prb=25)
    assert t["Nref"] == 11854
    items = K.lbrm_items(shapes, t["Nref"])
    pairs = sorted({(i["bg"], i["Z"]) for i in items})
    assert len(pairs) == 15
    assert pairs == [(0, Z) for Z in (192, 208, 224, 240, 256, 288, 320, 352, 384)] + \
        [(1, Z) for Z in (240, 256, 288, 320, 352, 384)]
    assert all(t["Nref"] % Z for _, Z in pairs)


def test_walk_against_reference_dematcher(ref, shapes):
    """The position the walk gives the last of E selected bits is where the reference's rate de-matcher
    (srsran_ldpc_rm_rx_c) puts the last of E soft bits."""
    for (bg, Z), Nref in (((0, 15), K.MAX_NREF), ((1, 7), K.MAX_NREF), ((1, 36), K.MAX_NREF), ((0, 26), 1000),
                          ((1, 64), 2999)):
        s = K.pick(shapes, bg, Z)
        for rv in range(4):
            order = K.selection_order(bg, Z, s.Kp, s.Kr, rv, Nref)
            _, Ncb = K.k0_ncb(bg, Z, rv, Nref)
            assert len(order) == Ncb - max(0, min(s.Kr - 2 * Z, Ncb) - min(s.Kp - 2 * Z, Ncb))
            for E in (1, 2, s.Kp - 2 * Z, len(order) - 1, len(order), len(order) + 1, len(order) + Z):
                e = np.zeros(E, np.int8)
                e[-1] = 1
                out = np.zeros(Z * K.BG_N[bg] + 8, np.int8)
                ref.rm_rx(e, out, s.F, bg, Z, rv, 1, Nref)
                assert list(np.flatnonzero(out == 1)) == [K.last_position(order, E)], (bg, Z, rv, E)


@pytest.mark.parametrize("pairs", [K.EXHAUSTIVE, K.EDGE_SHAPES])
def test_row_edges_straddle_their_boundaries(shapes, pairs):
    n = 0
    for bg, Z in pairs:
        s = K.pick(shapes, bg, Z)
        assert s.F > 0
        for rv in range(4):
            order = K.selection_order(bg, Z, s.Kp, s.Kr, rv)
            edges = K.row_edges(s, rv)
            k0, Ncb = K.k0_ncb(bg, Z, rv)
            # every row above the one k0 lies in has an edge
            first = max(4, k0 // Z + 2 - K.BG_K[bg] + 1)
            assert [r for r, _ in edges] == list(range(first, K.BG_M[bg])), (bg, Z, rv)
            for r, E_r in edges:
                b = K.row_boundary(bg, Z, r)
                assert E_r >= 2 and K.last_position(order, E_r - 1) < b <= K.last_position(order, E_r), (bg, Z, rv, r)
                assert max(order[:E_r - 1]) < b
                n += 1
            w = K.wrap_edge(s, rv)
            assert K.last_position(order, w) < K.last_position(order, w - 1) == Ncb - 1
    assert n > 300


def test_edge_values():
    assert K.edge_E_values(589) == [(1, 588), (1, 589), (1, 590), (2, 588), (2, 590)]
    assert K.edge_E_values(590) == [(1, 589), (1, 590), (1, 591), (2, 588), (2, 590)]
    assert K.edge_E_values(2) == [(1, 1), (1, 2), (1, 3), (2, 2)]


def test_tb_crc_lengths(ref):
    # the reference's segmentation gives these payload byte counts next to the slice edges 4096 k: the nearest
    # the product accepts, and the nearest whose code blocks carry the whole TB
    assert K.slice_edge_counts(ref.tb_info, 0.9) == [4093, 4097, 8189, 8197, 12286, 12297]
    assert K.slice_edge_counts(ref.tb_info, 0.2) == [4093, 4101, 8189, 8205, 12272, 12295]
    assert K.slice_edge_counts(ref.tb_info, 0.9, K.tiles) == [4093, 4097, 8189, 8197, 12285, 12297]
    assert K.slice_edge_counts(ref.tb_info, 0.2, K.tiles) == [4092, 4101, 8187, 8205, 12269, 12295]
    for R in (0.9, 0.2):
        for k in (1, 2, 3):
            t = ref.tb_info(8 * K.TB_SLICE * k, R, 1, 64 * K.TB_SLICE * k, 1)
            assert t["C"] > 1 and not K.accepted(t) and not K.tiles(t)  # no admitted size is an edge itself
            assert (K.TB_SLICE * k + 3) % t["C"]
    assert ref.tb_info(8 * 478, 0.5, 1, 9000, 1)["L_tb"] == 16 and ref.tb_info(8 * 479, 0.9, 1, 9000, 1)["L_tb"] == 24
    assert {K.TB_CHUNK * k + d for k in (1, 2) for d in (-1, 0, 1)} <= set(K.SMALL_BYTE_COUNTS)  # chunk edges
    items = K.tb_crc_items(ref.tb_info)
    assert sorted({i["tbs"] // 8 for i in items}) == sorted(set(K.SMALL_BYTE_COUNTS) | {
        4092, 4093, 4097, 4101, 8187, 8189, 8197, 8205, 12269, 12272, 12285, 12286, 12295, 12297})
    for i in items:
        t = ref.tb_info(i["tbs"], i["R"], i["Qm"], i["G"], i["Nl"])
        assert K.accepted(t) and i["G"] % (i["Qm"] * i["Nl"]) == 0
        assert t["C"] == 1 or (i["G"] // (i["Qm"] * i["Nl"])) % t["C"]
        assert i["tiles"] == (i["delivered"] == i["tbs"] // 8) and i["delivered"] <= i["tbs"] // 8
    assert {i["rv"] for i in items} == {0, 1, 2, 3}
    # accepted sizes whose blocks leave out the TB's last bytes: four lengths, at rv 0 and one other rv each
    assert sorted({(i["tbs"] // 8, i["R"]) for i in items if not i["tiles"]}) == [
        (4093, 0.2), (8189, 0.2), (12272, 0.2), (12286, 0.9)]


def test_multi_cb_pairs(ref):
    pairs = K.multi_cb_pairs(ref.tb_info)
    assert len(pairs) == 16
    assert sorted(pairs) == [(bg, Z) for bg in (0, 1) for Z in (208, 224, 240, 256, 288, 320, 352, 384)]
    assert max(hi[0] for _, hi in pairs.values()) == K.MAX_NOF_CB
    items = K.multi_cb_items(ref.tb_info)
    assert len(items) == 64 and {i["Nl"] for i in items} == {1, 2, 3, 4}
    for (bg, Z), (lo, hi) in pairs.items():
        assert {i["C"] for i in items if (i["bg"], i["Z"]) == (bg, Z)} == {lo[0], hi[0]}
    for i in items:
        t = ref.tb_info(i["tbs"], i["R"], i["Qm"], i["G"], i["Nl"])
        assert K.tiles(t) and i["tiles"] and t["C"] == i["C"] > 1 and (t["bg"], t["Z"]) == (i["bg"], i["Z"])
        n = i["G"] // (i["Qm"] * i["Nl"])
        assert n * i["Qm"] * i["Nl"] == i["G"] and n % t["C"]  # two E values
