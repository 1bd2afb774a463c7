"""The GPU channel estimator against fixtures recorded from the reference's own compiled chest_dl.c
(tests/golden/make_chest_golden.py; case table, tolerances and distances in tests/chest_cases.py): no result here is
compared with this project's own restatement.

* host API (srsran_chest_dl_estimate_cfg / srsran_chest_dl_estimate): every case of the table, call by call on one
  object -- the estimate, every scalar and table of srsran_chest_dl_res_t, the object's noise_estimate / rsrp / rssi
  per [rx][port] and cfo, and the caller's grids after correct_sync_error;
* device API (srsran_chest_dl_gpu_estimate): an AVERAGE case with one row per (port, rx) and one with full grids,
  with the four floats of d_res;
* batch API (srsran_chest_dl_gpu_estimate_batch_cfg): every case it accepts (Gauss filters, no MBSFN), the case's
  subframes in one call and again as 2 + 1 calls on a fresh object, so that the kept PSS / EMPTY noise and the CFO
  carry inside a batch and across calls; TDD cases set srsran_chest_dl_gpu_set_tdd_config first.

res->cfo is compared with `cfo_expect`: the reference's value; in a 4-port cell the value a 2-port reference object
finds on the same grids, and in a TDD special subframe the last full subframe's (the two documented
deviations).  The device and batch APIs have no configuration switch for the CFO estimate: d_res[3] is not compared
for the zeroed configuration, which turns it off."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chest_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLES = ("snr_ant_port_db", "rsrp_ant_port_dbm", "rsrq_ant_port_db")


@pytest.fixture(scope="module")
def fx():
    return C.Fixture(GOLDEN)


@pytest.fixture(scope="module")
def U():
    from srsran_4g_amd import ue_dl
    ue_dl.use_standard_symbol_size(False)  # the reference's default rates, which the fixtures were recorded at
    return ue_dl


def new_chest(U, sc):
    ch = U.ChestDl(U.cell(sc["nof_prb"], sc["ports"], sc["cell_id"], cp=sc["cp"], tdd=sc["tdd"] is not None), sc["nrx"])
    for a in sorted(set(sc["areas"])):
        if a:
            assert ch.set_mbsfn_area_id(a) == 0
    assert U.lib().srsran_symbol_sz(sc["nof_prb"]) == C.SYMBOL_SZ[sc["nof_prb"]]
    return ch


def chest_cfg(U, cs, area=0):
    if cs["zero"]:
        return U.srsran_chest_dl_cfg_t()
    return U.chest_cfg(cs["est"], cs["noise"], cs["c0"], cs["c1"], sync_error=bool(cs["sync"]), filter_type=cs["ftype"],
                       mbsfn_area_id=area)


class Check:
    """collects every distance of a test, prints it, and fails at the end with all that miss their tolerance"""

    def __init__(self, name):
        self.name, self.bad = name, []

    def __call__(self, where, quantity, kind, got, want):
        d = C.err(kind, got, want)
        print(self.name, where, quantity, "%.3g" % d)
        if not d <= C.TOL[kind]:
            self.bad.append((where, quantity, d))

    def ce(self, where, sc, ref, i, got):
        """got: (ports, nrx, rows * nre) or (ports, nrx, nre) against the fixture's rows (1: every row is that row)"""
        got = got.reshape(sc["ports"], sc["nrx"], -1, 12 * sc["nof_prb"])
        want = ref["ce"][i]
        if want.shape[2] == 1:
            want = np.broadcast_to(want, got.shape)
        self(where, "ce", "ce", got, want)

    def done(self):
        assert not self.bad, self.bad


@pytest.mark.parametrize("cs", C.CASES, ids=[c["name"] for c in C.CASES])
def test_host_api(U, fx, cs):
    sc, Y, ref, _ = fx.case(cs)
    nrx, ports = sc["nrx"], sc["ports"]
    ch, ck = new_chest(U, sc), Check(cs["name"])
    for i, tti in enumerate(sc["ttis"]):
        grids = [Y[i, r].copy() for r in range(nrx)]
        cfg = None if cs["zero"] else chest_cfg(U, cs, sc["areas"][i])
        ce, res = ch.estimate(grids, tti, cfg, tdd=sc["tdd"], mbsfn=bool(sc["mbsfn"][i]))
        ck.ce(i, sc, ref, i, ce)
        for name in C.SCALARS:
            ck(i, name, C.KIND[name], getattr(res, name), ref["cfo_expect" if name == "cfo" else name][i])
        ck(i, "rsrp_port_dbm", "db", [res.rsrp_port_dbm[p] for p in range(ports)], ref["rsrp_port_dbm"][i])
        for name in TABLES:
            t = getattr(res, name)
            ck(i, name, "db", [[t[r][p] for p in range(ports)] for r in range(nrx)], ref[name][i])
        for name, t in (("q_noise", ch.q.noise_estimate), ("q_rsrp", ch.q.rsrp), ("q_rssi", ch.q.rssi)):
            ck(i, name, "lin", [[t[r][p] for p in range(ports)] for r in range(nrx)], ref[name][i])
        ck(i, "q_cfo", "lin", ch.q.cfo, ref["cfo_expect"][i])
        want = ref["grid"][i] if "grid" in ref else Y[i]  # rotated in place, or back as they went in
        ck(i, "grid", "grid", np.stack(grids), want)
        if "grid" not in ref:
            assert np.array_equal(np.stack(grids), Y[i])
    ch.free()
    ck.done()


def d_res_checks(ck, where, cs, ref, i, r):
    """the four floats of d_res: noise_estimate, rsrp, rssi (linear; the fixture has it in dBm), cfo"""
    ck(where, "noise_estimate", "lin", r[0], ref["noise_estimate"][i])
    ck(where, "rsrp", "lin", r[1], ref["rsrp"][i])
    ck(where, "rssi_dbm", "db", 10 * np.log10(np.float64(r[2])) + 30, ref["rssi_dbm"][i])
    if not cs["zero"]:
        ck(where, "cfo", "lin", r[3], ref["cfo_expect"][i])


@pytest.mark.parametrize("name,full", [("f50a_avg", 0), ("f6a_avg", 1)])
def test_device_api(U, fx, name, full):
    """srsran_chest_dl_gpu_estimate (srsUE's defaults: AVERAGE, Gauss 4 / 1.0, REFS): rows of 12 nof_prb, or full
    grids whose every row is the fixture's row"""
    cs = C.by_name(C.CASES)[name]
    assert (cs["est"], cs["noise"], cs["ftype"], cs["c0"], cs["c1"], cs["sync"], cs["zero"]) == (0, 0, 0, 4.0, 1.0, 0, 0)
    sc, Y, ref, _ = fx.case(cs)
    nrx, ports, nre = sc["nrx"], sc["ports"], 12 * sc["nof_prb"]
    rows = 2 * (6 if sc["cp"] else 7) if full else 1
    ch, ck = new_chest(U, sc), Check(name)
    f = U.lib().srsran_chest_dl_gpu_estimate
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                  ctypes.c_void_p]
    for i, tti in enumerate(sc["ttis"]):
        d_grid = torch.from_numpy(Y[i].view(np.float32)).cuda()
        d_ce = torch.zeros(ports * nrx * rows * nre * 2, dtype=torch.float32, device="cuda")
        d_res = torch.zeros(4, dtype=torch.float32, device="cuda")
        assert f(ctypes.byref(ch.q), tti, d_grid.data_ptr(), d_ce.data_ptr(), full, d_res.data_ptr(), None) == 0
        torch.cuda.synchronize()
        ck.ce(i, sc, ref, i, d_ce.cpu().numpy().view(np.complex64))
        d_res_checks(ck, i, cs, ref, i, d_res.cpu().numpy())
    ch.free()
    ck.done()


BATCH_CASES = [c for c in C.CASES if c["ftype"] == C.GAUSS and not any(C.by_name(C.SCENES)[c["scene"]]["mbsfn"])]


@pytest.mark.parametrize("cs", BATCH_CASES, ids=[c["name"] for c in BATCH_CASES])
def test_batch_api(U, fx, cs):
    sc, Y, ref, _ = fx.case(cs)
    nrx, ports, nre = sc["nrx"], sc["ports"], 12 * sc["nof_prb"]
    nsf, n = len(sc["ttis"]), Y.shape[2]
    full = 1 if cs["est"] == C.INTERPOLATE else 0
    rows = n // nre if full else 1
    f = U.lib().srsran_chest_dl_gpu_estimate_batch_cfg
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                  ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    ck = Check(cs["name"])
    for split in ([nsf], [2, nsf - 2]) if nsf > 2 else ([nsf],):
        ch = new_chest(U, sc)
        if sc["tdd"]:
            t = U.srsran_tdd_config_t()
            t.sf_config, t.ss_config, t.configured = sc["tdd"][0], sc["tdd"][1], True
            assert U.lib().srsran_chest_dl_gpu_set_tdd_config(ctypes.byref(ch.q), t) == 0
        cfg = chest_cfg(U, cs)
        start = 0
        for count in split:
            d_grid = torch.from_numpy(np.ascontiguousarray(Y[start:start + count]).view(np.float32)).cuda()
            d_ce = torch.zeros(count * ports * nrx * rows * nre * 2, dtype=torch.float32, device="cuda")
            d_res = torch.zeros((count, 4), dtype=torch.float32, device="cuda")
            d_idx = torch.tensor([t % 10 for t in sc["ttis"][start:start + count]], dtype=torch.int32, device="cuda")
            assert f(ctypes.byref(ch.q), ctypes.byref(cfg), d_idx.data_ptr(), count, d_grid.data_ptr(), nrx * n,
                     d_ce.data_ptr(), ports * nrx * rows * nre, full, d_res.data_ptr(), None) == 0
            torch.cuda.synchronize()
            ce = d_ce.cpu().numpy().view(np.complex64).reshape(count, -1)
            res = d_res.cpu().numpy()
            grids = d_grid.cpu().numpy().view(np.complex64).reshape(count, nrx, n)
            for b in range(count):
                i, where = start + b, "%s:%d" % ("+".join(map(str, split)), start + b)
                ck.ce(where, sc, ref, i, ce[b])
                d_res_checks(ck, where, cs, ref, i, res[b])
                ck(where, "grid", "grid", grids[b], ref["grid"][i] if "grid" in ref else Y[i])
            start += count
        ch.free()
    ck.done()
