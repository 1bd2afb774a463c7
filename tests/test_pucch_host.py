"""PUCCH receive, host side (CPU only): the ctypes layouts against what the C compiler lays out, every resource
helper of include/srsran_pucch.h against the values recorded from the reference (tests/golden/pucch_golden.npz,
made by tests/golden/make_pucch_golden.py), the numpy test transmitter against the reference transmitter's grids,
and the loud failure of the receive calls without a device."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pucch_cases as C
import pucch_tx as T
from srsran_4g_amd import pucch as P
from srsran_4g_amd import tdec
from srsran_4g_amd.sch import srsran_uci_value_t
from srsran_4g_amd.ue_dl import cell as make_cell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
STRUCTS = [P.srsran_pucch_cfg_t, P.srsran_pucch_t, P.srsran_pucch_res_t, P.srsran_pucch_gpu_ue_t]


@pytest.fixture(scope="module")
def G():
    return C.Golden.get()


def test_ctypes_layouts_match_the_c_compiler(G):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "srsran_pucch.h"', 'int main(void) {']
    for s in STRUCTS:
        lines.append(f'  printf("{s.__name__} %zu\\n", sizeof({s.__name__}));')
        for f in s._fields_:
            lines.append(f'  printf("{s.__name__}.{f[0]} %zu\\n", offsetof({s.__name__}, {f[0]}));')
    lines += ['  return 0;', '}']
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, src, "-o", exe], check=True)
        got = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for s in STRUCTS:
        assert int(got[s.__name__]) == ctypes.sizeof(s), s.__name__
        for f in s._fields_:
            assert int(got[f"{s.__name__}.{f[0]}"]) == getattr(s, f[0]).offset, (s.__name__, f[0])
    # and the reference's own layout, recorded by the generator
    mine = [ctypes.sizeof(P.srsran_pucch_cfg_t), ctypes.sizeof(P.srsran_pucch_res_t), ctypes.sizeof(srsran_uci_value_t),
            ctypes.sizeof(P.srsran_uci_cfg_t), P.srsran_pucch_cfg_t.format.offset, ctypes.sizeof(C.srsran_ul_sf_cfg_t),
            P.srsran_pucch_cfg_t.threshold_format1.offset, P.srsran_pucch_res_t.correlation.offset]
    assert mine == list(G.z["layout"])


def test_n_cs_cell_two_cells(G):
    for cid in (1, 150):
        for cp in (0, 1):
            t = np.array(P.n_cs_cell(make_cell(6, 1, cid, cp=cp))).reshape(20, 7)[:, :T.nsym(cp)]
            assert np.array_equal(t, G.z[f"h_ncs_{cid}_{cp}"]), (cid, cp)
            assert np.array_equal(T.cell_tables(cid, cp)[0], G.z[f"h_ncs_{cid}_{cp}"])


def test_m_n_prb_alpha_over_the_recorded_configurations(G):
    L = P.lib()
    for i, spec in enumerate(G.cases):
        s = C.full(spec)
        cell = make_cell(s["nof_prb"], 1, s["cell_id"], cp=s["cp"])
        cfg = C.build_cfg(s)
        m = [L.srsran_pucch_m(ctypes.byref(cfg), s["cp"]), L.srsran_pucch_n_prb(ctypes.byref(cell), ctypes.byref(cfg), 0),
             L.srsran_pucch_n_prb(ctypes.byref(cell), ctypes.byref(cfg), 1)]
        assert m == list(G.z[f"h_m_{i}"]), spec["name"]
        ncs = P.n_cs_cell(cell)
        nL = T.nsym(s["cp"])
        al, noc, npr = [], [], []
        for dm in range(2):
            for ns in range(20):
                for l in range(nL):
                    o, p = ctypes.c_uint32(0), ctypes.c_uint32(0)
                    if s["fmt"] < P.FORMAT_2:
                        al.append(L.srsran_pucch_alpha_format1(ctypes.byref(ncs), ctypes.byref(cfg), s["cp"], bool(dm), ns, l,
                                                               ctypes.byref(o), ctypes.byref(p)))
                    else:
                        al.append(L.srsran_pucch_alpha_format2(ctypes.byref(ncs), ctypes.byref(cfg), ns, l))
                    noc.append(o.value)
                    npr.append(p.value)
        assert np.array_equal(np.array(al, np.float32), G.z[f"h_alpha_{i}"]), spec["name"]  # value-exact
        assert noc == list(G.z[f"h_noc_{i}"]) and npr == list(G.z[f"h_npr_{i}"]), spec["name"]


def test_select_format_and_get_resources(G):
    L = P.lib()
    for i, spec in enumerate(G.cases):
        s = C.full({k: v for k, v in spec.items() if k not in ("fmt", "n_pucch")})
        cell = make_cell(s["nof_prb"], 1, s["cell_id"], cp=s["cp"])
        cfg = C.build_cfg(s)
        if not cfg.simul_cqi_ack and s["acks"] and cfg.uci_cfg.cqi.data_enable:
            cfg.uci_cfg.cqi.data_enable = False
        cfg.format = L.srsran_pucch_proc_select_format(ctypes.byref(cell), ctypes.byref(cfg), ctypes.byref(cfg.uci_cfg), None)
        npi = (ctypes.c_uint32 * 4)()
        n = L.srsran_pucch_proc_get_resources(ctypes.byref(cell), ctypes.byref(cfg), ctypes.byref(cfg.uci_cfg), None, npi)
        assert [cfg.format, n] + list(npi)[:n] == list(G.z[f"h_sel_{i}"]), spec["name"]


def test_get_npucch_is_the_reference_ue_choice(G):
    """format, resource and b(0) b(1) of every recorded transmission: srsran_pucch_proc_select_format with the UCI
    value + srsran_pucch_proc_get_npucch, as ue_ul.c calls them"""
    L = P.lib()
    n = 0
    for i, spec in enumerate(G.cases):
        if spec["tx"] is None:
            continue
        s = C.full({k: v for k, v in spec.items() if k not in ("fmt", "n_pucch")})
        cell = make_cell(s["nof_prb"], 1, s["cell_id"], cp=s["cp"])
        cfg = C.build_cfg(s)
        if not cfg.simul_cqi_ack and s["acks"] and cfg.uci_cfg.cqi.data_enable:
            cfg.uci_cfg.cqi.data_enable = False
        v = C.build_uci_value(spec["tx"], srsran_uci_value_t)
        cfg.format = L.srsran_pucch_proc_select_format(ctypes.byref(cell), ctypes.byref(cfg), ctypes.byref(cfg.uci_cfg),
                                                       ctypes.byref(v))
        b = (ctypes.c_uint8 * 10)()
        npucch = L.srsran_pucch_proc_get_npucch(ctypes.byref(cell), ctypes.byref(cfg), ctypes.byref(cfg.uci_cfg),
                                                ctypes.byref(v), b)
        assert (cfg.format, npucch) == (spec["fmt"], spec["n_pucch"]), spec["name"]
        if cfg.format in (P.FORMAT_1A, P.FORMAT_1B):
            assert list(b)[:cfg.format] == list(G.z[f"tx_bits_{i}"]), spec["name"]
        n += 1
    assert n >= 70
    tdd = make_cell(6, 1, 1, tdd=True)  # the reference's TDD resource list comes back as an error: 0
    cfg = C.build_cfg(dict(acks=[[2, 0, 0, 0]], mode=1))
    cfg.format = P.FORMAT_1B
    cfg.uci_cfg.ack[0].tdd_ack_M = 2
    assert L.srsran_pucch_proc_get_npucch(ctypes.byref(tdd), ctypes.byref(cfg), ctypes.byref(cfg.uci_cfg),
                                          ctypes.byref(srsran_uci_value_t()), (ctypes.c_uint8 * 10)()) == 0


def test_cs_get_ack_whole_table(G):
    L = P.lib()
    want = G.z["h_cs_ack"]
    for a in range(3):
        for j in range(4):
            for b0 in range(2):
                for b1 in range(2):
                    cfg = P.srsran_pucch_cfg_t()
                    cfg.uci_cfg.ack[0].nof_acks = a + 2
                    v = srsran_uci_value_t()
                    v.ack.ack_value[5] = 1  # cleared by the call
                    ret = L.srsran_pucch_cs_get_ack(ctypes.byref(cfg), ctypes.byref(cfg.uci_cfg), j,
                                                    (ctypes.c_uint8 * 2)(b0, b1), ctypes.byref(v))
                    assert [ret] + list(v.ack.ack_value)[:4] == list(want[a, j, b0, b1]), (a, j, b0, b1)
                    assert v.ack.ack_value[5] == 0


def test_cfg_isvalid_collision_and_small_tables(G):
    L = P.lib()
    for ds, ncs, nrb2, want in G.z["h_isvalid"]:
        cfg = C.build_cfg(dict(ds=int(ds), N_cs=int(ncs), n_rb_2=int(nrb2)))
        assert int(L.srsran_pucch_cfg_isvalid(ctypes.byref(cfg), 6)) == want, (ds, ncs, nrb2)
    cell = make_cell(6, 1, 1)
    for fmt, a, b, want in G.z["h_collision"]:
        ca = C.build_cfg(dict(ds=2, N_cs=4, n_rb_2=1, fmt=int(fmt), n_pucch=int(a)))
        cb = C.build_cfg(dict(ds=2, N_cs=4, n_rb_2=1, fmt=int(fmt), n_pucch=int(b)))
        assert L.srsran_pucch_collision(ctypes.byref(cell), ctypes.byref(ca), ctypes.byref(cb)) == want, (fmt, a, b)
    assert L.srsran_pucch_collision(None, None, None) == -2
    got = []
    for f in range(7):
        got.append(L.srsran_pucch_nof_ack_format(f))
        for cp in range(2):
            if cp == 1 and f in (P.FORMAT_2A, P.FORMAT_2B):
                got += [0, 0, 0, 0]
                continue
            n = L.srsran_refsignal_dmrs_N_rs(f, cp)
            got += [n] + [L.srsran_refsignal_dmrs_pucch_symbol(m, f, cp) if m < n else 0 for m in range(3)]
    assert got == list(G.z["h_misc"])
    assert L.srsran_pucch_format_text(P.FORMAT_2B) == b"Format 2B" and L.srsran_pucch_format_text_short(P.FORMAT_1A) == b"1a"
    assert L.srsran_pucch_format_text(P.FORMAT_ERROR) == b"Format Error" and L.srsran_pucch_format_text_short(9) == b"Err"
    d = (ctypes.c_float * 2)()
    for bits, want in (((0, 0), (1, 0)), ((0, 1), (0, -1)), ((1, 0), (0, 1)), ((1, 1), (-1, 0))):
        assert L.srsran_pucch_format2ab_mod_bits(P.FORMAT_2B, (ctypes.c_uint8 * 2)(*bits), d) == 0 and tuple(d) == want
    assert L.srsran_pucch_format2ab_mod_bits(P.FORMAT_2A, (ctypes.c_uint8 * 2)(1, 0), d) == 0 and tuple(d) == (-1, 0)
    assert L.srsran_pucch_format2ab_mod_bits(P.FORMAT_2, (ctypes.c_uint8 * 2)(1, 0), d) == -1
    good = C.build_cfg(dict(ds=2, N_pucch_1=0, n_pucch_sr=9))
    assert L.srsran_pucch_cfg_assert(ctypes.byref(cell), ctypes.byref(good)) == 0
    good.n_pucch_sr = 0  # the SR resource on top of N_pucch_1
    assert L.srsran_pucch_cfg_assert(ctypes.byref(cell), ctypes.byref(good)) == -1


def test_numpy_transmitter_equals_the_reference_grids(G):
    """tests/pucch_tx.py against the reference's srsran_pucch_encode + DMRS, every case with a transmission"""
    n = 0
    for i, spec in enumerate(G.cases):
        if spec["tx"] is None:
            continue
        s = C.full(spec)
        r = T.Res(s["fmt"], s["n_pucch"], s["ds"], s["N_cs"], s["n_rb_2"], bool(s["gh"]), s["rnti"])
        g = T.encode(r, s["nof_prb"], s["cell_id"], s["cp"], s["tti"], bool(s["shortened"]),
                     list(G.z[f"tx_bits_{i}"]), list(G.z[f"tx_ack_{i}"]))
        want = G.z[f"clean_{i}"].reshape(g.shape)
        assert np.abs(g - want).max() <= 1e-6 * np.abs(want).max(), spec["name"]
        n += 1
    assert n >= 70


@pytest.mark.skipif(tdec.gpu_available(), reason="a HIP device is present")
def test_pucch_fails_loudly_without_gpu():
    with pytest.raises(RuntimeError):
        P.Pucch(make_cell(6, 1, 1))
    q = P.srsran_pucch_t()
    assert P.lib().srsran_pucch_init_enb(ctypes.byref(q)) == -1 and not q.gpu
    # the receive calls refuse objects that hold no device state
    res = P.srsran_pucch_res_t()
    assert P.lib().srsran_pucch_gpu_get_batch(ctypes.byref(q), 0, None, ctypes.byref(res)) == -2
    assert P.lib().srsran_pucch_decode(ctypes.byref(q), None, None, None, None, ctypes.byref(res)) == -2
    assert P.lib().srsran_chest_ul_estimate_pucch(None, None, None, None, None) == -2
