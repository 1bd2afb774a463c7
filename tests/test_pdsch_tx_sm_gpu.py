"""Closed-loop spatial multiplexing (TM4) in the GPU transmitter against the reference's own precoder: the
composition of oracle/ref_pdsch_tx_harness.c (srsran_sequence_pdsch_apply_pack, srsran_mod_modulate_bytes,
srsran_layermap_type, srsran_precoding_type -> srsran_precoding_multiplex, precoding.c:2087-2211), marshalled as
tests/test_pdsch_tx_ref_gpu.py does, with the codebook index the harness derives (pmi with one codeword, pmi + 1 with
two) and the tolerance that module applies to CDD: 1e-6 absolute on unit-power symbols.

Cells of 6 and 15 PRB on 2 ports, normal CP and one extended-CP cell; every batch carries the nine scheme cases
(1 layer / 1 TB with pmi 0..3, 2 layers / 2 TBs with pmi 0 and 1, 2 layers / 1 TB with pmi 0..2) as nine subframes,
at QPSK and 64QAM, with the precoder scaling 1 and sqrt 2.

2 layers / 1 TB: the DCI's precoding information gives one codeword pmi 0..3 (ra_dl.c:513-519, dci_api.cpp
config_mimo) and the codebook of one codeword is its pmi, of which the two-layer precoder takes 0..2
(precoding.c:2196-2202): those three are the cases.  The codeword carries 2 nre modulation symbols, even ones on
layer 0 and odd ones on layer 1 (srsran_layermap_multiplex -> srsran_layermap_diversity, layermap.c:38-61); the
harness gets them as a 2 nre codeword, whose nre precoded symbols a port are the expected REs.

RE counts: the allocations are chosen so that several are no multiple of the kernel's 16 symbols a thread (asserted
below).  An odd count cannot be made with 2 ports: an OFDM symbol of a PRB has 12 PDSCH REs, or 8 where the CRS of
both ports sit, and PSS / SSS / PBCH take whole 72-RE rows (48 where the CRS sit), so every count is even; the
allocation of 5 PRB (660 = 41 x 16 + 4 REs) ends a thread in the middle of its 16 instead."""
import ctypes
import os
import sys

import numpy as np
import pytest

from synth import synth as SY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOD_OF_QM = {2: 1, 4: 2, 6: 3}  # srsran_mod_t
SPATIALMUX = 2  # srsran_tx_scheme_t
ATOL = 1e-6  # test_pdsch_tx_ref_gpu.py's, float precoding of unit-power symbols

SM_CASES = [(1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 1, 3), (2, 2, 0), (2, 2, 1), (2, 1, 0), (2, 1, 1), (2, 1, 2)]  # nl, ntb, pmi
CELLS = [  # (nof_prb, cp, cfi, tti of the nine subframes, PRBs left out of subframe i's allocation)
    (6, 0, 1, [1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 1, 0, 2, 0, 1, 0, 0, 1]),
    (15, 0, 2, [1, 2, 3, 4, 16, 6, 7, 8, 9], [0, 4, 1, 0, 2, 0, 6, 3, 0]),
    (6, 1, 1, [1, 2, 3, 4, 5, 6, 7, 8, 9], [1, 0, 0, 1, 0, 2, 0, 1, 0]),
]
TBS = {(6, 2): 328, (6, 6): 1544, (15, 2): 1064, (15, 6): 4264}  # (nof_prb, Qm): a table TBS that fits every allocation


@pytest.fixture(scope="module")
def env():
    from srsran_4g_amd import tdec
    if not tdec.gpu_available():
        pytest.fail("no HIP device on a GPU test run")
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    if not O.ref_available():  # on a HIP box the parity checker must be there: fail, never skip
        pytest.fail("oracle/_ref/libsrsref.so missing: the reference checker of this module was not built")
    L = ctypes.CDLL(O.REF_SO, mode=os.RTLD_LAZY)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    L.ref_pdsch_tx_symbols_sc.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint32, u32p, u32p,
                                          u32p, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                          ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_float, ctypes.POINTER(ctypes.c_float)]
    L.ref_pdsch_tx_symbols_sc.restype = ctypes.c_int
    import torch
    return torch, L, O.Oracle()


def ref_symbols(L, es, Qm, nl, pmi, rnti, sf_idx, cell_id, nre, scaling):
    """the reference composition of the codewords' coded bits es on 2 ports -> (2, nre) complex64"""
    ncw = len(es)
    lpc = nl // ncw  # layers a codeword: its nre * lpc symbols are the harness's codeword length
    stride = max(len(e) for e in es)
    buf = np.zeros((ncw, stride), np.uint8)
    for c, e in enumerate(es):
        assert len(e) == nre * lpc * Qm
        buf[c, :len(e)] = e
    u = lambda v: (ctypes.c_uint32 * len(v))(*v)  # noqa: E731
    out = np.zeros((2, nre * lpc, 2), np.float32)
    r = L.ref_pdsch_tx_symbols_sc(ncw, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), stride,
                                  u([len(e) for e in es]), u([MOD_OF_QM[Qm]] * ncw), u(list(range(ncw))), rnti, sf_idx,
                                  cell_id, SPATIALMUX, 2, nl, pmi, nre * lpc, scaling,
                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    assert r == 0
    return out.view(np.complex64)[:, :nre, 0]


def rho_a(p_a, P):
    """apply_power_allocation's rho_a (pdsch.c:492): 10^(p_a / 20) x sqrt 2 with more than one port, in float"""
    return float(np.float32(float(np.float32(10.0) ** np.float32(p_a / 20.0)) * (1.0 if P == 1 else np.sqrt(2.0))))


def sm_cfg(U, nprb, prb, nre, tbs, Qm, nl, ntb, pmi, rnti, cp=0):
    cfg = U.pdsch_cfg(nprb, nre, [tbs] * ntb, [Qm] * ntb, scheme="sm", pmi=pmi, rnti=rnti, cp=cp, layers=nl)
    for s in range(2):
        for n in range(nprb):
            cfg.grant.prb_idx[s][n] = bool(prb[n])
    cfg.grant.nof_prb = int(np.sum(prb))
    return cfg


def coded_bits(ora, tbs, Qm, nl, ntb, nre, pls):
    lpc = nl // ntb
    return [ora.dlsch_encode(tbs, Qm * lpc, 0, nre * Qm * lpc, pl) for pl in pls]  # rate matching on Qm * Nl


def device_grids(torch, enb, nsf, P, sf_re):
    from srsran_4g_amd.sch import _memcpy_d2h
    ptr = enb.sf_symbols()
    assert ptr
    host = torch.empty(nsf * P * sf_re * 2, dtype=torch.float32)
    _memcpy_d2h(host, ptr, host.numel() * 4)
    return host.numpy().view(np.complex64).reshape(nsf, P, sf_re).copy()


def test_re_counts_cover_partial_threads():
    """the allocations below: several RE counts are no multiple of the 16 symbols a thread, every one is even"""
    counts = []
    for nprb, cp, cfi, ttis, drop in CELLS:
        for tti, k in zip(ttis, drop):
            prb = np.arange(nprb) < nprb - k
            counts.append(int(SY.pdsch_mask(nprb, 2, 29, cfi, tti % 10, prb=prb, cp=cp).sum()))
    assert sum(1 for c in counts if c % 16) >= 8 and 660 in counts
    assert all(c % 2 == 0 for c in counts)


@pytest.mark.parametrize("scaling", [1.0, float(np.float32(np.sqrt(2.0)))], ids=["sc1", "sc_sqrt2"])
@pytest.mark.parametrize("Qm", [2, 6], ids=["qpsk", "64qam"])
@pytest.mark.parametrize("cellcase", CELLS, ids=["6prb", "15prb", "6prb_extcp"])
def test_enb_tx_batch_sm_matches_reference_precoder(env, cellcase, Qm, scaling):
    """srsran_enb_dl_gpu_tx_batch: nine subframes, one per (layers, TBs, pmi); the PDSCH REs of both port grids
    (srsran_enb_dl_gpu_sf_symbols) equal the reference composition, every other RE is what the same batch
    without the PDSCH holds"""
    torch, L, ora = env
    from srsran_4g_amd import enb_dl as E
    from srsran_4g_amd import ue_dl as U
    nprb, cp, cfi, ttis, drop = cellcase
    cell_id, rnti, P = 29, 0x2B17, 2
    tbs = TBS[(nprb, Qm)]
    U.use_standard_symbol_size(True)
    N = SY.symbol_sz(nprb)
    cell = U.cell(nprb, P, cell_id, cp=cp)
    enb = E.EnbDl(cell)
    sfs, empty, wants, masks, keep = [], [], [], [], []
    rng = np.random.default_rng(1000 * nprb + 10 * Qm + cp)
    for (nl, ntb, pmi), tti, k in zip(SM_CASES, ttis, drop):
        prb = np.arange(nprb) < nprb - k
        mask = SY.pdsch_mask(nprb, P, cell_id, cfi, tti % 10, prb=prb, cp=cp)
        nre = int(mask.sum())
        pls = [rng.integers(0, 256, tbs // 8, dtype=np.uint8) for _ in range(ntb)]
        d_pl = [torch.from_numpy(p).cuda() for p in pls]
        cfg = sm_cfg(U, nprb, prb, nre, tbs, Qm, nl, ntb, pmi, rnti, cp)
        keep += [d_pl, cfg]
        sfs.append((tti, cfi, cfg, [p.data_ptr() for p in d_pl]))
        empty.append((tti, cfi, None, []))
        wants.append(ref_symbols(L, coded_bits(ora, tbs, Qm, nl, ntb, nre, pls), Qm, nl, pmi, rnti, tti % 10, cell_id,
                                 nre, scaling))
        masks.append(mask)
    nsf, sf_re = len(sfs), masks[0].size
    d_out = torch.zeros((nsf, P, 15 * N, 2), dtype=torch.float32, device="cuda")
    try:
        assert enb.tx_batch(sfs, d_out.data_ptr(), 1.0 / N, pdsch_scaling=scaling) == 0
        torch.cuda.synchronize()
        grid = device_grids(torch, enb, nsf, P, sf_re)
        assert enb.tx_batch(empty, d_out.data_ptr(), 1.0 / N) == 0
        torch.cuda.synchronize()
        bare = device_grids(torch, enb, nsf, P, sf_re)
    finally:
        enb.free()
    for b in range(nsf):
        m = masks[b].reshape(-1)
        for p in range(P):
            np.testing.assert_allclose(grid[b, p][m], wants[b][p], rtol=0, atol=ATOL, err_msg=f"{SM_CASES[b]} port {p}")
            assert np.array_equal(grid[b, p][~m], bare[b, p][~m]), f"{SM_CASES[b]} port {p}: RE outside the PDSCH"
            assert not np.any(bare[b, p][m])


def test_pdsch_encode_sm_matches_reference_precoder(env):
    """srsran_pdsch_encode on host grids, 2 layers / 2 TBs pmi 1 at 15 PRB 64QAM with p_a = -3 dB: its rho_a is
    the precoder's scaling (pdsch.c:1057-1071)"""
    torch, L, ora = env
    from srsran_4g_amd import ue_dl as U
    nprb, P, Qm, tti, cfi, cell_id, rnti, p_a = 15, 2, 6, 3, 2, 29, 0x2B17, -3.0
    tbs = TBS[(nprb, Qm)]
    mask = SY.pdsch_mask(nprb, P, cell_id, cfi, tti % 10)
    nre = int(mask.sum())
    rng = np.random.default_rng(5)
    pls = [rng.integers(0, 256, tbs // 8, dtype=np.uint8) for _ in range(2)]
    want = ref_symbols(L, coded_bits(ora, tbs, Qm, 2, 2, nre, pls), Qm, 2, 1, rnti, tti % 10, cell_id, nre,
                       rho_a(p_a, P))
    pd = U.Pdsch(U.cell(nprb, P, cell_id), 1, enb=True)
    cfg = sm_cfg(U, nprb, np.ones(nprb, bool), nre, tbs, Qm, 2, 2, 1, rnti)
    cfg.p_a = p_a
    keepval = np.complex64(0.25 - 0.5j)  # what the caller's grids hold outside the PDSCH stays
    ret, got = pd.encode(cfg, tti, cfi, pls, [np.full(mask.size, keepval, np.complex64) for _ in range(P)])
    pd.free()
    assert ret == 0
    for p in range(P):
        g = np.asarray(got[p]).reshape(mask.shape)
        np.testing.assert_allclose(g[mask], want[p], rtol=0, atol=ATOL)
        assert np.all(g[~mask] == keepval), "REs outside the PDSCH written"


def test_enb_dl_put_pdsch_sm_matches_reference_precoder(env):
    """srsran_enb_dl_put_pdsch + srsran_enb_dl_gen_signal, 1 layer pmi 2 at 6 PRB QPSK: sf_symbols hold the
    reference composition with rho_a = sqrt 2 (p_a = 0, 2 ports) on the PDSCH REs"""
    torch, L, ora = env
    from srsran_4g_amd import enb_dl as E
    from srsran_4g_amd import ue_dl as U
    nprb, P, Qm, tti, cfi, cell_id, rnti = 6, 2, 2, 7, 1, 29, 0x2B17
    tbs = TBS[(nprb, Qm)]
    mask = SY.pdsch_mask(nprb, P, cell_id, cfi, tti % 10)
    nre = int(mask.sum())
    pl = np.random.default_rng(6).integers(0, 256, tbs // 8, dtype=np.uint8)
    want = ref_symbols(L, coded_bits(ora, tbs, Qm, 1, 1, nre, [pl]), Qm, 1, 2, rnti, tti % 10, cell_id, nre,
                       rho_a(0.0, P))
    U.use_standard_symbol_size(True)
    N = U.lib().srsran_symbol_sz(nprb)
    out = [np.zeros(15 * N, np.complex64) for _ in range(P)]
    enb = E.EnbDlRef(U.cell(nprb, P, cell_id), out)
    try:
        cfg = sm_cfg(U, nprb, np.ones(nprb, bool), nre, tbs, Qm, 1, 1, 2, rnti)
        cfg.p_a = 0.0
        enb.put_base(U.sf_cfg(tti, cfi))
        assert enb.put_pdsch(cfg, [pl]) == 0
        enb.gen_signal()
        grid = [enb.sf_symbols(p, mask.size) for p in range(P)]
    finally:
        enb.free()
    for p in range(P):
        np.testing.assert_allclose(grid[p][mask.reshape(-1)], want[p], rtol=0, atol=ATOL)
    assert any(np.abs(o).max() > 0 for o in out)


@pytest.mark.parametrize("P,nl,ntb,pmi", [(4, 1, 1, 0), (4, 2, 2, 0), (2, 2, 2, 2), (2, 2, 1, 3)],
                         ids=["4port_1l", "4port_2l", "2l_2tb_pmi2", "2l_1tb_pmi3"])
def test_sm_refusals(env, P, nl, ntb, pmi):
    """what the reference's precoder refuses stays refused by both entry points: 4 ports (precoding.c:2207-2209) and
    two-layer codebook 3 (:2196-2202), which is pmi 2 with two codewords and pmi 3 with one"""
    torch, L, ora = env
    from srsran_4g_amd import enb_dl as E
    from srsran_4g_amd import ue_dl as U
    nprb, Qm, tti, cfi, cell_id, rnti = 6, 2, 7, 1, 29, 0x2B17
    tbs = TBS[(nprb, Qm)]
    mask = SY.pdsch_mask(nprb, P, cell_id, cfi, tti % 10)
    nre = int(mask.sum())
    pls = [np.zeros(tbs // 8, np.uint8) for _ in range(ntb)]
    cfg = sm_cfg(U, nprb, np.ones(nprb, bool), nre, tbs, Qm, nl, ntb, pmi, rnti)
    cell = U.cell(nprb, P, cell_id)
    U.use_standard_symbol_size(True)
    N = SY.symbol_sz(nprb)
    enb = E.EnbDl(cell)
    d_pl = [torch.from_numpy(p).cuda() for p in pls]
    d_out = torch.zeros((1, P, 15 * N, 2), dtype=torch.float32, device="cuda")
    try:
        assert enb.tx_batch([(tti, cfi, cfg, [p.data_ptr() for p in d_pl])], d_out.data_ptr(), 1.0 / N) == -1
    finally:
        enb.free()
    pd = U.Pdsch(cell, 1, enb=True)
    try:
        ret, _ = pd.encode(cfg, tti, cfi, pls, [np.zeros(mask.size, np.complex64) for _ in range(P)])
    finally:
        pd.free()
    assert ret == -1
