"""UE transmit -> channel -> eNB receive for PUCCH, all on the GPU: srsran_ue_ul_encode samples, a 3-tap channel, a
timing offset and AWGN at 20 dB in numpy, srsran_ofdm_rx with freq_shift_f = -0.5, then srsran_pucch_gpu_get_batch.
Every case is taken from tests/golden/pucch_golden.npz (the reference decides them with >= 0.05 room at 20 dB) and has
to be detected with the UCI that was sent: the decoded fields equal the fixture's, which the reference decoded from
its own transmission of the same UCI.  The three mux3_f1a UEs go through one srsran_ue_ul_gpu_tx_batch, are summed
after per-UE phase rotations and are each decoded; one case also goes through srsran_chest_ul_estimate_pucch +
srsran_pucch_decode."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pucch_cases as C  # noqa: E402
import pucch_rx as R  # noqa: E402
import pucch_tx_cases as X  # noqa: E402
from srsran_4g_amd import pucch as P  # noqa: E402
from srsran_4g_amd import tdec  # noqa: E402
from srsran_4g_amd import ue_dl  # noqa: E402
from srsran_4g_amd import ue_ul as UL  # noqa: E402

pytestmark = pytest.mark.gpu

SNR_DB = 20.0
TAPS = np.array([1.0, 0.25 * np.exp(0.7j), 0.12 * np.exp(-1.9j)])  # one sample apart
DELAY = 1  # samples, inside the cyclic prefix together with the taps
# at least one case per format, SR + ACK with SR sent and not sent, channel selection over 4 resources, format 3 with
# SR, extended CP, a shortened subframe, the 25-PRB m = 3 resource
LOOP = ["f1_cp0_sh0", "f1a_cp0_sh0", "f1b_cp0_sh0", "f1a_cp0_sh1", "f2_wb11_2", "f2_ri1", "f2a_ack1", "f2b_10",
        "f3_cp0_sh0", "f3_sr", "sr_ack_sr_sent", "sr_ack_no_sr", "cs4_2", "f1b_cp1_sh0", "f3_cp1_sh0", "prb25_m3"]
MUX = ["mux3_f1a_0", "mux3_f1a_1", "mux3_f1a_2"]


class Env:
    def __init__(self):
        self.G = C.Golden.get()
        self.rig = R.Rig()
        self.ues, self.rxs = {}, {}

    def case(self, name):
        i = next(k for k, sp in enumerate(self.G.cases) if sp["name"] == name)
        return i, self.G.cases[i]

    def ue(self, s, cell):
        key = (s["nof_prb"], s["cell_id"], s["cp"])
        if key not in self.ues:
            self.ues[key] = UL.UeUl(cell)
            self.rxs[key] = ue_dl.OfdmRx(s["nof_prb"], cp=s["cp"], freq_shift_f=-0.5)
            assert self.rxs[key].symbol_sz == self.ues[key].q.fft.cfg.symbol_sz
        return self.ues[key], self.rxs[key]

    def free(self):
        for u in self.ues.values():
            u.free()
        self.rig.free()


@pytest.fixture(scope="module")
def env():
    if not tdec.gpu_available():
        pytest.fail("no HIP device on a GPU test run")
    e = Env()
    yield e
    e.free()


def through_the_channel(rx, x, on, rng, power=1.0):
    """the samples through the taps and the delay, scaled to the mean power `power` on the PUCCH REs of the received
    grid (one per UE), plus white noise SNR_DB below one UE; returns the received grid [2 nsym, 12 nof_prb]"""
    y = np.convolve(x.astype(np.complex128), TAPS)[:x.size]
    y = np.concatenate([np.zeros(DELAY), y[:-DELAY]])
    clean = rx.rx_inplace(np.ascontiguousarray(y, np.complex64)).reshape(on.shape)
    p_re = float(np.mean(np.abs(clean[on]) ** 2))
    assert p_re > 0
    y = y * np.sqrt(power / p_re)
    # srsran_ofdm_rx without normalize sums N samples: noise of variance v per sample gives N v per RE
    sigma = np.sqrt(10 ** (-SNR_DB / 10) / rx.symbol_sz / 2)
    y = y + sigma * (rng.standard_normal(y.size) + 1j * rng.standard_normal(y.size))
    return rx.rx_inplace(np.ascontiguousarray(y, np.complex64)).reshape(on.shape)


def check_decoded(env, i, spec, res):
    gi, _ = C.res_arrays(res)
    want = env.G.z[f"g_res_i_{i}"]
    names = C.RES_FIELDS[:12]  # everything but ta_valid
    assert list(gi[:12]) == list(want[:12]), (spec["name"], dict(zip(names, gi[:12])), dict(zip(names, want[:12])))
    assert gi[0] == 1, spec["name"]  # detected
    tx = spec["tx"]
    if C.full(spec)["sr_tti"]:
        assert gi[6] == int(tx.get("sr", 0)), spec["name"]
    if tx.get("cqi") is not None and C.full(spec)["simul"]:
        assert gi[7] == tx["cqi"][0] and gi[10] == 1, spec["name"]
    if "ri" in tx:
        assert gi[11] == tx["ri"], spec["name"]
    if len(tx.get("ack", [])) <= 2 and C.full(spec)["mode"] == 0:
        assert list(gi[2:2 + len(tx.get("ack", []))]) == list(tx.get("ack", [])), spec["name"]


@pytest.mark.parametrize("name", LOOP)
def test_loop(env, name):
    i, spec = env.case(name)
    s, cell, ucfg, v, sf = X.ue_setup(spec)
    ue, rx = env.ue(s, cell)
    ret, x = ue.encode(sf, ucfg, None, v)
    assert ret == 1
    pc = ucfg.ul_cfg.pucch
    assert (pc.format, pc.n_pucch) == (spec["fmt"], spec["n_pucch"])
    on = np.logical_or(*X.masks(s, pc.format, pc.n_pucch, bool(s["shortened"])))
    grid = through_the_channel(rx, x.copy(), on, np.random.default_rng(900 + i))
    ret, res, _ = R.get_one(env.rig, spec, grid)
    assert ret == 0
    check_decoded(env, i, spec, res)


def test_three_multiplexed_ues_through_one_batch(env):
    import torch
    rng = np.random.default_rng(77)
    built, keep, total, on = [], [], None, None
    for name in MUX:
        i, spec = env.case(name)
        s, cell, ucfg, v, sf = X.ue_setup(spec, mode=UL.NORMALIZE_FORCE_AMPLITUDE, peak=0.5)
        ue, rx = env.ue(s, cell)
        d_out = torch.zeros(2 * ue.sf_len, dtype=torch.float32, device="cuda")
        keep.extend([ucfg, v, sf])
        built.append((i, spec, s, ucfg, (ue, sf, ucfg, v, None, d_out.data_ptr(), None), d_out))
    assert UL.tx_batch([b[4] for b in built]) == 0
    torch.cuda.synchronize()
    for i, spec, s, ucfg, _, d_out in built:
        pc = ucfg.ul_cfg.pucch
        assert (pc.format, pc.n_pucch) == (spec["fmt"], spec["n_pucch"])
        m = np.logical_or(*X.masks(s, pc.format, pc.n_pucch, False))
        on = m if on is None else on | m
        x = d_out.cpu().numpy().view(np.complex64) * np.exp(2j * np.pi * rng.random())
        total = x if total is None else total + x
    assert int(on.sum()) == 14 * 12  # the three share one PRB per slot
    grid = through_the_channel(rx, total, on, rng, power=3.0)  # orthogonal UEs of unit power each
    for i, spec, _, _, _, _ in built:
        ret, res, _ = R.get_one(env.rig, spec, grid)
        assert ret == 0
        check_decoded(env, i, spec, res)


def test_direct_estimate_and_decode(env):
    i, spec = env.case("f1b_cp0_sh0")
    s, cell, ucfg, v, sf = X.ue_setup(spec)
    ue, rx = env.ue(s, cell)
    ret, x = ue.encode(sf, ucfg, None, v)
    assert ret == 1
    pc = ucfg.ul_cfg.pucch
    on = np.logical_or(*X.masks(s, pc.format, pc.n_pucch, False))
    grid = through_the_channel(rx, x.copy(), on, np.random.default_rng(5))
    _, chest, pucch = env.rig.get(s)
    cfg = R.direct_cfg(env.G, i)
    assert P.estimate(chest, C.build_sf(s), cfg, grid) == 0
    ret, res = pucch.decode(C.build_sf(s), cfg, chest.res, grid)
    assert ret == 0 and res.detected and res.uci_data.ack.valid
    assert list(res.uci_data.ack.ack_value)[:2] == list(spec["tx"]["ack"])
    assert res.correlation > 0.9
