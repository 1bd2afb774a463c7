"""TDD cells on the downlink receive path (srsran_pdsch_decode on TDD, ra_dl.c:55-56, 433-435,
pdsch.c:90-107, 154-159; refsignal_dl.c:169-226).

* the CRS estimator in special subframes, whose DwPTS holds 1-4 CRS symbols a port (the 1- / 2-symbol noise path,
  the time average over the symbols present, the one-symbol interpolation), host-synchronous and batched, against
  the oracle restatement (oracle_chest_dl_tdd / _ext_tdd; itself pinned to recorded results of the compiled
  chest_dl.c in special subframes with 1 / 3 / 4 CRS symbols, test_chest_golden.py) at 2e-5 of the largest estimate;
* the whole UE DL chain on TDD cells from time samples (synth/ TDD transmitter: SSS in the last symbol of
  subframes 0 / 5, PSS in symbol 2 of subframes 1 / 6, special subframes sending their DwPTS only): every
  downlink and special subframe of a frame decoded host-synchronously and in one batch, equal to the oracle chain
  (decode_tb return, payload bytes) and to what was sent."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import Oracle, crs_nsym
import pdsch_chain as PC
import pdsch_np
from synth import synth as S

from test_phy_oracle import make_subframe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ora():
    return Oracle()


@pytest.fixture(scope="module")
def U():
    from srsran_4g_amd import ue_dl
    ue_dl.use_standard_symbol_size(True)
    yield ue_dl
    ue_dl.use_standard_symbol_size(False)


@pytest.fixture(scope="module")
def SCH():
    from srsran_4g_amd import sch
    return sch


# (special-subframe configuration, DwPTS symbols): 1 / 2 / 3 / 4 CRS symbols of ports 0-1
SS_CASES = [(0, 3), (9, 6), (1, 9), (4, 12)]


@pytest.mark.parametrize("ss", [c[0] for c in SS_CASES])
@pytest.mark.parametrize("nports,nof_prb,est", [(2, 100, 0), (1, 50, 0), (4, 25, 0), (2, 100, 1), (1, 25, 1)])
def test_chest_special_subframe_matches_oracle(U, ora, ss, nports, nof_prb, est):
    """srsran_chest_dl_estimate_cfg on subframe 1 (special) of TDD configuration 1: the CRS symbols of the DwPTS only,
    against oracle_chest_dl_ext_tdd; INTERPOLATE where the reference's own interpolation reads only rows it
    estimated (1 or 3+ CRS symbols; with 2 the host refuses, see test_chest_interpolate_refused)"""
    dw = pdsch_np.TDD_SS_SYMBOLS[ss][0]
    nsym = crs_nsym(dw)
    if est == 1 and nsym[0] == 2:
        pytest.skip("INTERPOLATE with 2 CRS symbols: refused (test_chest_interpolate_refused)")
    rng = np.random.default_rng(ss * 10 + nports + est)
    cell_id = 17
    tdd = (1, ss)
    Y, _, _ = make_subframe(ora, rng, nof_prb=nof_prb, cell_id=cell_id, nports=nports, nrx=2, sf_idx=1, snr_db=25)
    N = U.lib().srsran_symbol_sz(nof_prb)
    ch = U.ChestDl(U.cell(nof_prb, nports, cell_id, tdd=True), 2)
    cfg = U.chest_cfg(est, 0, 4, 1.0)
    ce, res = ch.estimate(Y, 11, cfg, tdd=tdd)
    ceo, st, _, _ = ora.chest_dl_ext(Y, nof_prb, cell_id, nports, 1, N, 0, est, 0, 4, 1.0, nsym=nsym)
    assert np.abs(ce - ceo).max() <= 2e-5 * np.abs(ceo).max()
    assert res.noise_estimate == pytest.approx(st["noise"], rel=1e-4)
    assert res.rsrp == pytest.approx(st["rsrp"], rel=1e-4)
    # a downlink subframe of the same cell keeps 4 / 2 CRS symbols
    ce4, res4 = ch.estimate(Y, 14, cfg, tdd=tdd)
    ce4o, st4, _, _ = ora.chest_dl_ext(Y, nof_prb, cell_id, nports, 4, N, 0, est, 0, 4, 1.0)
    assert np.abs(ce4 - ce4o).max() <= 2e-5 * np.abs(ce4o).max()
    ch.free()


def test_chest_interpolate_refused(U, ora):
    """INTERPOLATE in a special subframe with 2 CRS symbols: the reference interpolates towards estimate rows it did
    not write in that call (chest_dl.c:520-527), so the GPU estimator refuses instead of guessing"""
    rng = np.random.default_rng(5)
    Y, _, _ = make_subframe(ora, rng, nof_prb=25, cell_id=3, nports=2, nrx=1, sf_idx=1)
    ch = U.ChestDl(U.cell(25, 2, 3, tdd=True), 1)
    with pytest.raises(RuntimeError):
        ch.estimate(Y, 1, U.chest_cfg(1, 0), tdd=(1, 9))  # DwPTS 6: 2 CRS symbols
    ch.estimate(Y, 1, U.chest_cfg(1, 0), tdd=(1, 4))  # DwPTS 12: 4 CRS symbols
    ch.free()


def test_chest_batch_special_subframes(U, ora):
    """srsran_chest_dl_gpu_estimate_batch_cfg over a frame of a TDD cell (configuration 1, special-subframe
    configuration 9: 2 CRS symbols in subframes 1 / 6) after srsran_chest_dl_gpu_set_tdd_config: every subframe's
    estimate row and stats equal the oracle's for its CRS symbol count"""
    rng = np.random.default_rng(9)
    nof_prb, nports, cell_id, nrx = 50, 2, 44, 2
    tdd = (1, 9)
    sfs = [i for i in range(10) if pdsch_np.tdd_type(1, i) != "U"]
    Ys = [make_subframe(ora, rng, nof_prb=nof_prb, cell_id=cell_id, nports=nports, nrx=nrx, sf_idx=i)[0] for i in sfs]
    ch = U.ChestDl(U.cell(nof_prb, nports, cell_id, tdd=True), nrx)
    t = U.srsran_tdd_config_t()
    t.sf_config, t.ss_config, t.configured = tdd[0], tdd[1], True
    assert U.lib().srsran_chest_dl_gpu_set_tdd_config(ctypes.byref(ch.q), t) == 0
    nre = 12 * nof_prb
    d_grid = torch.from_numpy(np.stack(Ys).view(np.float32)).cuda()
    d_ce = torch.zeros((len(sfs), nports, nrx, nre, 2), dtype=torch.float32, device="cuda")
    d_res = torch.zeros((len(sfs), 4), dtype=torch.float32, device="cuda")
    d_idx = torch.tensor(sfs, dtype=torch.int32, device="cuda")
    f = U.lib().srsran_chest_dl_gpu_estimate_batch_cfg
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                  ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    assert f(ctypes.byref(ch.q), None, d_idx.data_ptr(), len(sfs), d_grid.data_ptr(), nrx * 14 * nre, d_ce.data_ptr(),
             nports * nrx * nre, 0, d_res.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got = d_ce.cpu().numpy().view(np.complex64).reshape(len(sfs), nports, nrx, nre)
    res = d_res.cpu().numpy()
    N = U.lib().srsran_symbol_sz(nof_prb)
    for b, i in enumerate(sfs):
        nsym = crs_nsym(pdsch_np.TDD_SS_SYMBOLS[tdd[1]][0]) if pdsch_np.tdd_type(1, i) == "S" else (4, 2)
        ceo, st = ora.chest_dl(Ys[b], nof_prb, cell_id, nports, i, N, nsym=nsym)
        assert np.abs(got[b] - ceo[:, :, :nre]).max() <= 2e-5 * np.abs(ceo).max(), i
        assert res[b, 0] == pytest.approx(st["noise"], rel=1e-4), i
        assert res[b, 1] == pytest.approx(st["rsrp"], rel=1e-4), i
    ch.free()


def test_chest_batch_cfo_kept_in_special_subframes(U, ora):
    """CFO estimation on (srsUE: cfo_estimate_enable, mask 1023) over a TDD frame whose special subframes carry 2 CRS
    symbols: the reference's chest_estimate_cfo needs 4 (chest_dl.c:618-641), so the host-synchronous path keeps
    q->cfo from the last full subframe (chest_api.cpp); the batch reports the same, subframe by subframe -- including
    a special subframe first in a batch, which takes the last estimate of the batch before it"""
    rng = np.random.default_rng(19)
    nof_prb, nports, cell_id, nrx = 50, 2, 44, 2
    tdd = (1, 9)
    sfs = [i for i in range(10) if pdsch_np.tdd_type(1, i) != "U"]
    Ys = []
    for i in sfs:
        Y = make_subframe(ora, rng, nof_prb=nof_prb, cell_id=cell_id, nports=nports, nrx=nrx, sf_idx=i)[0]
        rot = np.exp(1j * (0.02 + 0.01 * i) * np.arange(14))[None, :, None]
        Ys.append((Y.reshape(nrx, 14, -1) * rot).astype(np.complex64).reshape(Y.shape))
    cfg = U.srsue_chest_cfg()
    # host-synchronous reference, subframe by subframe
    ch = U.ChestDl(U.cell(nof_prb, nports, cell_id, tdd=True), nrx)
    host = []
    for b, i in enumerate(sfs):
        _, res = ch.estimate(Ys[b], i, cfg, tdd=tdd)
        host.append(res.cfo)
    ch.free()
    assert len({round(h, 9) for h in host}) > 2  # distinct estimates per full subframe
    # batch: the frame as two batches, the second starting at special subframe 6 (carried from the first batch)
    ch = U.ChestDl(U.cell(nof_prb, nports, cell_id, tdd=True), nrx)
    t = U.srsran_tdd_config_t()
    t.sf_config, t.ss_config, t.configured = tdd[0], tdd[1], True
    assert U.lib().srsran_chest_dl_gpu_set_tdd_config(ctypes.byref(ch.q), t) == 0
    nre = 12 * nof_prb
    f = U.lib().srsran_chest_dl_gpu_estimate_batch_cfg
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                  ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    cut = sfs.index(6)
    got = []
    for part in (range(0, cut), range(cut, len(sfs))):
        idx = [sfs[b] for b in part]
        d_grid = torch.from_numpy(np.stack([Ys[b] for b in part]).view(np.float32)).cuda()
        d_ce = torch.zeros((len(idx), nports, nrx, nre, 2), dtype=torch.float32, device="cuda")
        d_res = torch.zeros((len(idx), 4), dtype=torch.float32, device="cuda")
        d_idx = torch.tensor(idx, dtype=torch.int32, device="cuda")
        assert f(ctypes.byref(ch.q), ctypes.byref(cfg), d_idx.data_ptr(), len(idx), d_grid.data_ptr(), nrx * 14 * nre,
                 d_ce.data_ptr(), nports * nrx * nre, 0, d_res.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got += list(d_res.cpu().numpy()[:, 3])
    ch.free()
    for b, i in enumerate(sfs):
        assert got[b] == pytest.approx(host[b], rel=1e-4, abs=1e-7), (i, got[b], host[b])


def _tdd_frame(U, ora, rng, tdd, nof_prb, nports, cell_id, snr_db):
    """one frame of a TDD cell from synth/: (tti, samples, nre, nsl, tbs, payloads, oracle-chain result) per downlink
    or special subframe; TBS from 36.213 with a special subframe's 0.75 N_PRB and a code rate <= ~0.75"""
    out = []
    lib = U.lib()
    for tti in range(10):
        t = pdsch_np.tdd_type(tdd[0], tti)
        if t == "U":
            continue
        nsl = pdsch_np.tdd_nof_symb_slot(tdd[0], tdd[1], tti)
        mask = S.pdsch_mask(nof_prb, nports, cell_id, 1, tti, tdd=tdd)
        nre = int(mask.sum())
        n_eff = max(1, int(0.75 * nof_prb)) if t == "S" else nof_prb
        i_tbs = max(i for i in range(27) if lib.srsran_ra_tbs_from_idx(i, n_eff) + 24 <= 0.75 * 6 * nre)
        tbs = lib.srsran_ra_tbs_from_idx(i_tbs, n_eff)
        pls = [rng.integers(0, 256, tbs // 8, dtype=np.uint8) for _ in range(2)]
        x, nre2 = S.pdsch_subframe(nof_prb, cell_id, nports, tti, 1, 0x1234, tbs, 6, 0, pls, snr_db=snr_db, rng=rng,
                                   N=2048 if nof_prb == 100 else None, tdd=tdd, sync=True)
        assert nre2 == nre
        g, ce, st = PC.fft_estimate(ora, x, nof_prb, cell_id, nports, tti, tdd=tdd)
        want = PC.pdsch_decode(ora, g, ce, st["noise"], nof_prb, cell_id, nports, tti, 1, 0x1234, [tbs, tbs], [6, 6],
                               [0, 0], tdd=tdd)
        out.append((tti, x, nre, nsl, tbs, pls, want))
    return out


@pytest.mark.parametrize("tdd", [(1, 7), (2, 0), (5, 9), (6, 4)])
def test_ue_dl_tdd_frame_matches_oracle_chain(U, SCH, ora, tdd):
    """A TDD frame (uplink-downlink configuration tdd[0], special-subframe configuration tdd[1]) through the GPU UE DL
    chain: srsran_ue_dl_decode_fft_estimate + srsran_ue_dl_decode_pdsch per subframe and srsran_ue_dl_gpu_decode_batch
    over all of them; every TB equals the oracle chain (return, payload bytes).  Every TB decodes to what synth/
    sent except in special subframes whose DwPTS holds 3 CRS symbols (9-11 DwPTS symbols, here configuration 7):
    there the reference's AVERAGE estimator sums the first two CRS symbols and scales by 2 / 3 (average_pilots,
    chest_dl.c:571-586: the loop adds pairs (2, 3), ... only while l < nsymbols - 1), so its channel estimate is 2 / 3
    of the channel and 64QAM fails in the reference -- and here, identically."""
    nof_prb, nports, cell_id = 100, 2, 3
    rng = np.random.default_rng(100 * tdd[0] + tdd[1])
    frame = _tdd_frame(U, ora, rng, tdd, nof_prb, nports, cell_id, 30.0)
    cell = U.cell(nof_prb, nports, cell_id, tdd=True)
    ue = U.UeDl(cell, 2, tdd=tdd)
    keep = []
    def three_crs(tti):
        return pdsch_np.tdd_type(tdd[0], tti) == "S" and crs_nsym(pdsch_np.TDD_SS_SYMBOLS[tdd[1]][0])[0] == 3

    for tti, x, nre, nsl, tbs, pls, want in frame:  # host-synchronous
        assert ue.fft_estimate(x, tti, 1) == 0
        assert ue.last_cfi == 1
        sb = [SCH.SoftbufferRx(nof_prb=nof_prb) for _ in range(2)]
        keep.append(sb)
        cfg = U.pdsch_cfg(nof_prb, nre, (tbs, tbs), (6, 6), softbuffers=sb, nsl=nsl)
        ret, out = ue.decode_pdsch(cfg, tti, 1)
        for q in range(2):
            assert (want[q]["ret"] == 0) == (not three_crs(tti)), (tti, q)
            assert bool(out[q][0]) == (want[q]["ret"] == 0), (tti, q)
            if want[q]["ret"] == 0:
                assert np.array_equal(out[q][1][: tbs // 8], pls[q]), (tti, q)
                assert np.array_equal(out[q][1][: tbs // 8 + 3], want[q]["data"][: tbs // 8 + 3]), (tti, q)
    # the batch: the whole frame in one call
    ue2 = U.UeDl(cell, 2, tdd=tdd)
    tmax = max(f[4] for f in frame)
    d_pl = torch.zeros((len(frame), 2, tmax // 8 + 64), dtype=torch.uint8, device="cuda")
    entries = []
    for b, (tti, x, nre, nsl, tbs, pls, want) in enumerate(frame):
        sb = [SCH.SoftbufferRx(nof_prb=nof_prb) for _ in range(2)]
        cfg = U.pdsch_cfg(nof_prb, nre, (tbs, tbs), (6, 6), softbuffers=sb, nsl=nsl)
        keep += [sb, cfg]
        entries.append((tti, 1, cfg, [d_pl[b, 0].data_ptr(), d_pl[b, 1].data_ptr()], [1, 1]))
    d_x = torch.from_numpy(np.stack([f[1] for f in frame]).view(np.float32)).cuda()
    d_res = torch.full((2 * len(frame),), 7, dtype=torch.int32, device="cuda")
    d_avg = torch.zeros(2 * len(frame), dtype=torch.float32, device="cuda")
    assert ue2.gpu_decode_batch(entries, d_x.data_ptr(), d_res.data_ptr(), d_avg.data_ptr(), 0.0, None) == 2 * len(frame)
    torch.cuda.synchronize()
    res, pl = d_res.cpu().numpy(), d_pl.cpu().numpy()
    for b, (tti, x, nre, nsl, tbs, pls, want) in enumerate(frame):
        for q in range(2):
            assert res[2 * b + q] == want[q]["ret"], (tti, q)
            if want[q]["ret"] == 0:
                assert np.array_equal(pl[b, q, : tbs // 8], pls[q]), (tti, q)
                assert np.array_equal(pl[b, q, : tbs // 8 + 3], want[q]["data"][: tbs // 8 + 3]), (tti, q)
    ue.free()
    ue2.free()
