"""The oracle's restatement of the DL channel estimator (oracle/phy_oracle.c: oracle_chest_dl_tdd, _ext_f, _ext_tdd,
_mbsfn) against fixtures recorded from the reference's own compiled chest_dl.c (tests/golden/make_chest_golden.py;
case table and tolerances in tests/chest_cases.py).  Every GPU test that compares the estimator with the restatement
(test_chest_gpu.py, test_tdd_gpu.py, test_extcp_gpu.py, test_mbsfn_gpu.py) inherits this pin.

Per call the restatement returns the estimate, the noise estimate (averaged and per [rx][port]), RSRP, RSSI, the CFO,
the sync error and the corrected grids; each is compared at the tolerance chest_cases.TOL gives its kind.  The
restatement keeps no state but the noise estimates, so its CFO is compared where the subframe has an estimate of its
own (4 CRS symbols, not MBSFN, CFO estimation on) with `cfo_expect`: the reference's value, or in a 4-port cell the
value of ports 0 / 1 ("4-port CFO").

Measured (the restatement against the reference, largest over all cases): estimates 5.2e-7 of the largest estimate,
noise 6.3e-7 (1.1e-6 per [rx][port]), RSRP 2.7e-7, CFO 1.0e-7 relative, sync error 2.1e-6 of max(|value|, 1e-2), RSSI
7.1e-5 dB, corrected grids 1.9e-7 of the largest sample.  TDD special subframes and MBSFN hold like FDD."""
import os

import numpy as np
import pytest

import chest_cases as C
from oracle import Oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return C.Fixture(GOLDEN)


@pytest.fixture(scope="module")
def ora():
    return Oracle()


def test_fixture_holds_the_case_table(fx):
    """every case of the table is in its file and no other; each file within the size of the largest fixture"""
    for key, name in C.FILES.items():
        want = [cs["name"] for cs in C.CASES if fx.scenes[cs["scene"]]["file"] == key]
        assert fx.index[key] == want
        assert os.path.getsize(os.path.join(GOLDEN, name)) <= C.MAX_FIXTURE_BYTES
    assert len({cs["name"] for cs in C.CASES}) == len(C.CASES)
    for knob, a, b in C.KNOB_PAIRS:
        ca, cb = C.by_name(C.CASES)[a], C.by_name(C.CASES)[b]
        assert {k for k in ca if k != "name" and ca[k] != cb[k]} <= set(C.KNOB_FIELDS[knob])
    assert {k for k, _, _ in C.KNOB_PAIRS} == set(C.KNOB_FIELDS)


@pytest.mark.parametrize("cs", C.CASES, ids=[c["name"] for c in C.CASES])
def test_reference_builds_agree(fx, cs):
    """the reference's -Ofast / AVX2 build and its plain scalar build differ by at most a quarter of each tolerance,
    and the values a relative tolerance is applied to are away from 0"""
    sc, _, ref, spread = fx.case(cs)
    for name in C.QUANTITIES:
        assert spread[name] <= C.TOL[C.KIND[name]] / 4, name
    if not cs["zero"]:
        assert (np.abs(ref["cfo_expect"]) >= C.CFO_FLOOR).all()
    if cs["sync"] and sc["delay"] >= 0.1:
        assert (np.abs(ref["sync_error"]) >= C.SYNC_FLOOR).all() and "grid" in ref
    else:
        assert "grid" not in ref


def restatement(ora, sc, cs, Y):
    """the case's calls through the restatement, the kept noise estimates and the estimate buffers carried from
    call to call -> per call dict(ce, noise, q_noise, and where the restatement has them rsrp, rssi, cfo,
    sync_error, grid), plus the same from the narrower entry points where the configuration is theirs"""
    nprb, cid, ports, cp = sc["nof_prb"], sc["cell_id"], sc["ports"], sc["cp"]
    N = C.SYMBOL_SZ[nprb]
    state, ce, calls, extra = np.zeros((4, 4), np.float32), None, [], []
    for i, tti in enumerate(sc["ttis"]):
        sf, nsym = tti % 10, C.crs_nsym(sc, tti)
        if sc["mbsfn"][i]:
            ce, noise, state = ora.chest_dl_mbsfn(Y[i], nprb, cid, ports, sf, sc["areas"][i], noise_alg=cs["noise"],
                                                  filter_type=cs["ftype"], coef0=cs["c0"], coef1=cs["c1"],
                                                  noise_state=state, cp=cp, ce_init=ce)
            calls.append(dict(ce=ce, noise=noise, q_noise=state))
            continue
        before = state
        ce, st, Yo, state = ora.chest_dl_ext(Y[i], nprb, cid, ports, sf, N, cp, cs["est"], cs["noise"], cs["c0"], cs["c1"],
                                             sync=bool(cs["sync"]), noise_state=before, nsym=nsym,
                                             filter_type=cs["ftype"])
        calls.append(dict(ce=ce, noise=st["noise"], q_noise=state, rsrp=st["rsrp"], rssi=st["rssi"], cfo=st["cfo"],
                          sync_error=st["sync_error"], grid=Yo))
        if cs["ftype"] == C.GAUSS:  # oracle_chest_dl_ext_tdd: Gauss filters of integer order
            ce2, st2, Y2, state2 = ora.chest_dl_ext_tdd(Y[i], nprb, cid, ports, sf, N, cp, cs["est"], cs["noise"],
                                                        cs["c0"], cs["c1"], sync=bool(cs["sync"]), noise_state=before,
                                                        nsym=nsym)
            extra.append((i, dict(ce=ce2, noise=st2["noise"], q_noise=state2, rsrp=st2["rsrp"], rssi=st2["rssi"],
                                  cfo=st2["cfo"], sync_error=st2["sync_error"], grid=Y2)))
        if (cs["est"], cs["noise"], cs["ftype"], cs["c0"], cs["c1"], cs["sync"]) == (0, 0, 0, 4.0, 1.0, 0):
            ce3, st3 = ora.chest_dl(Y[i], nprb, cid, ports, sf, N, cp=cp, nsym=nsym)  # oracle_chest_dl_tdd: srsUE's defaults
            extra.append((i, dict(ce=ce3, noise=st3["noise"], rsrp=st3["rsrp"], rssi=st3["rssi"], cfo=st3["cfo"])))
    return calls, extra


def distances(sc, cs, ref, i, got):
    """name -> (kind, distance) of one call's restatement results from the fixture's"""
    nrx, ports = sc["nrx"], sc["ports"]
    rows = ref["ce"].shape[3]
    ce = got["ce"].reshape(ports, nrx, -1, 12 * sc["nof_prb"])
    want = np.broadcast_to(ref["ce"][i], ce.shape) if rows == 1 else ref["ce"][i]
    d = {"ce": ("ce", C.err("ce", ce, want)), "noise_estimate": ("lin", C.err("lin", got["noise"], ref["noise_estimate"][i]))}
    if "q_noise" in got:
        d["q_noise"] = ("lin", C.err("lin", got["q_noise"][:nrx, :ports], ref["q_noise"][i]))
    if "rsrp" in got:
        d["rsrp"] = ("lin", C.err("lin", got["rsrp"], ref["rsrp"][i]))
        d["rssi_dbm"] = ("db", C.err("db", 10 * np.log10(np.float64(got["rssi"])) + 30, ref["rssi_dbm"][i]))
        if not cs["zero"] and C.crs_nsym(sc, sc["ttis"][i])[0] == 4:
            d["cfo"] = ("lin", C.err("lin", got["cfo"], ref["cfo_expect"][i]))
    if "sync_error" in got:
        d["sync_error"] = ("sync", C.err("sync", got["sync_error"], ref["sync_error"][i]))
    if "grid" in got:
        d["grid"] = ("grid", C.err("grid", got["grid"], ref["grid"][i]))
    return d


@pytest.mark.parametrize("cs", C.CASES, ids=[c["name"] for c in C.CASES])
def test_restatement_matches_reference(fx, ora, cs):
    sc, Y, ref, _ = fx.case(cs)
    if "grid" not in ref:  # nothing was rotated: the grids must come back as they went in
        ref = dict(ref, grid=Y)
    calls, extra = restatement(ora, sc, cs, Y)
    assert len(calls) == len(sc["ttis"])
    for i, got in list(enumerate(calls)) + extra:
        for name, (kind, dist) in distances(sc, cs, ref, i, got).items():
            print(cs["name"], i, name, dist)
            assert dist <= C.TOL[kind], (i, name, dist)
