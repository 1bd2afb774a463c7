"""GPU NR SCH transmit parity through the C-ABI (srsran_dlsch_nr_encode / srsran_ulsch_nr_encode /
srsran_sch_nr_gpu_encode_batch / srsran_ldpc_rm_tx) against the reference's own transmitter compiled into
oracle/_ref (RefNr.encode = srsran_dlsch_nr_encode of sch_nr.c over ldpc_encoder.c and ldpc_rm.c).
Everything is bits: every e_bits byte must be equal.  The loop test feeds the batch encoder's output to the
batch decoder without leaving the device."""
import ctypes

import numpy as np
import pytest
import torch

import nr_sch as ON
from nr_sch import RefNr
from srsran_4g_amd import ldpc as GL
from srsran_4g_amd import sch_nr as S
from srsran_4g_amd import tdec
from srsran_4g_amd.sch import MOD_FROM_QM
from synth.nr_tx import CRC16, CRC24A, crc_bytes

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
ERROR, INVALID_INPUTS = -1, -2

# (N_re, R, Qm, N_L, lbrm, nof_prb); G = N_re Qm N_L, TBS from the reference's srsran_ra_nr_tbs
CASES = [
    (400, 0.3, 2, 1, False, 52),
    (3000, 0.5, 4, 1, False, 52),
    (8112, 0.6, 6, 2, False, 52),      # C = 7, E in {13896, 13908}
    (15264, 0.75, 6, 2, True, 106),    # C = 17, Ncb < N
    (100, 0.2, 2, 1, False, 25),
    (14400, 0.9, 8, 2, True, 273),     # C = 25, Ncb < N
    (4680, 0.2, 4, 1, True, 52),       # BG2 Z = 384, Ncb < N and wrap
    (42588, 0.85, 8, 1, False, 273),   # C = 35
    (24, 0.5, 2, 1, False, 25),        # TBS 24, Z = 7: BG2 high-rate case 4
    (120, 0.3, 1, 1, False, 25),       # BPSK, no interleave
    (1200, 0.04, 2, 1, False, 25),     # E = 2400 on Z = 20: wraps several times, F = 88
    (8113, 0.6, 6, 2, False, 52),
    (2501, 0.7, 4, 3, False, 52),      # three layers, C = 3, two E values
    (3120, 0.1, 2, 1, True, 25),       # wrap
    (1300, 0.93, 4, 1, False, 25),     # BG1 Z = 224, E shorter than the high-rate region plus one row
]


class Shared:
    """The reference and what it computed, once for the module."""

    def __init__(self):
        self.ref = RefNr()
        self.tbs, self.pl, self.e = {}, {}, {}

    def case(self, i):
        n_re, R, Qm, Nl, lbrm, nof_prb = CASES[i]
        if i not in self.tbs:
            self.tbs[i] = self.ref.tbs(n_re, R, Qm, Nl)
            self.pl[i] = np.random.default_rng(1000 + i).integers(0, 256, self.tbs[i] // 8).astype(np.uint8)
        return dict(tbs=self.tbs[i], R=R, Qm=Qm, G=n_re * Qm * Nl, Nl=Nl, lbrm=lbrm, nof_prb=nof_prb,
                    mcs256=Qm == 8, pl=self.pl[i])

    def want(self, i, rv, nof_prb=None):
        c = self.case(i)
        prb = c["nof_prb"] if nof_prb is None else nof_prb
        key = (i, rv, prb)
        if key not in self.e:
            e = self.ref.encode(c["tbs"], c["R"], c["Qm"], c["G"], c["Nl"], rv, c["pl"], lbrm=c["lbrm"], nof_prb=prb,
                                mcs256=c["mcs256"])
            e.setflags(write=False)
            self.e[key] = e
        return self.e[key]


@pytest.fixture(scope="module")
def sh():
    if not tdec.gpu_available():
        pytest.skip("no HIP device")
    if not ON.ref_available():  # on a HIP box the parity checker must be there: fail, never skip
        pytest.fail("oracle/_ref/libsrsref.so missing: run build()")
    return Shared()


@pytest.fixture(scope="module")
def tx(sh):
    q = S.SchNr(nof_prb=273, tx=True)
    yield q
    q.free()


@pytest.fixture(scope="module")
def sbtx(sh):
    sb = S.nr_softbuffer_tx()
    yield sb
    sb.free()


@pytest.mark.parametrize("i", range(len(CASES)))
@pytest.mark.parametrize("uplink", [False, True])
def test_encode_matches_reference(sh, tx, sbtx, i, uplink):
    c = sh.case(i)
    tx.set_nof_prb(c["nof_prb"])
    for rv in range(4):
        want = sh.want(i, rv)
        assert want.max() <= 1
        ret, e = tx.encode(sbtx, c["tbs"], c["R"], c["Qm"], c["G"], c["Nl"], rv, c["pl"], lbrm=c["lbrm"],
                           mcs256=c["mcs256"], uplink=uplink, fill=SENTINEL)
        assert ret == 0
        assert np.array_equal(e, want), (CASES[i], rv, int(np.flatnonzero(e != want)[0]))


def _batch(sh, tx, sbtx, order, rvs, keep):
    entries, outs = [], {}
    for i in order:
        c = sh.case(i)
        cfg = S.make_cfg(c["lbrm"], c["mcs256"])
        tb = S.make_tb(c["tbs"], c["R"], c["Qm"], c["G"], c["Nl"], rvs[i], sbtx)
        d_p = torch.from_numpy(c["pl"]).cuda()
        d_e = torch.full((c["G"] + 3,), SENTINEL, dtype=torch.uint8, device="cuda")[3 * (i % 2):]  # odd and even starts
        keep += [cfg, tb, d_p, d_e]
        entries.append((cfg, tb, d_p.data_ptr(), d_e.data_ptr()))
        outs[i] = d_e
    assert tx.encode_batch(entries) == 0
    return outs


def test_batch_matches_single_calls_in_any_order(sh, tx, sbtx):
    tx.set_nof_prb(273)
    n = len(CASES)
    rvs = [(i + 1) % 4 for i in range(n)]
    single = {}
    for i in range(n):
        c = sh.case(i)
        ret, single[i] = tx.encode(sbtx, c["tbs"], c["R"], c["Qm"], c["G"], c["Nl"], rvs[i], c["pl"], lbrm=c["lbrm"],
                                   mcs256=c["mcs256"])
        assert ret == 0
        # one carrier for the whole batch: N_ref, where it is limited, is that of 273 PRB
        assert np.array_equal(single[i], sh.want(i, rvs[i], nof_prb=273)), CASES[i]
    for order in (list(range(n)), list(reversed(range(n)))):
        keep = []
        outs = _batch(sh, tx, sbtx, order, rvs, keep)
        torch.cuda.synchronize()
        for i in order:
            G = sh.case(i)["G"]
            assert np.array_equal(outs[i].cpu().numpy()[:G], single[i]), (CASES[i], order[0])


def test_rm_tx_alone_matches_reference(sh):
    rm = GL.LdpcRmTx()
    done = 0
    for i in range(len(CASES)):
        c = sh.case(i)
        t = S.tb_info(c["tbs"], c["R"], c["Qm"], c["G"], c["Nl"], lbrm=c["lbrm"], nof_prb=c["nof_prb"],
                      mcs256=c["mcs256"])
        if t.C != 1:
            continue
        # the single code block as sch_nr.c:483-517 builds it: payload, TB CRC, filler bytes
        crc = crc_bytes(c["pl"], CRC24A if t.L_tb == 24 else CRC16, t.L_tb)
        msg = np.full(t.Kr, 254, np.uint8)
        msg[:t.A] = np.unpackbits(c["pl"])
        msg[t.A:t.Kp] = [(crc >> (t.L_tb - 1 - b)) & 1 for b in range(t.L_tb)]
        enc = GL.LdpcEncoder(t.bg, t.Z)
        r, cw = enc.encode(msg)
        enc.free()
        assert r == 0 and np.all(cw[t.Kp - 2 * t.Z:t.Kr - 2 * t.Z] == 254)
        for rv in range(4):
            r, e = rm.rm_tx(cw, c["G"], t.bg, t.Z, rv, MOD_FROM_QM[c["Qm"]], t.Nref, fill=SENTINEL)
            assert r == 0 and np.array_equal(e, sh.want(i, rv)), (CASES[i], rv)
        if c["Qm"] > 1:
            assert rm.rm_tx(cw, c["G"] + 1, t.bg, t.Z, 0, MOD_FROM_QM[c["Qm"]], t.Nref)[0] == -1  # E % Qm != 0
        done += 1
    assert done >= 8
    assert rm.rm_tx(cw, 273 * 13 * 12 * 8 * 4 + 8, t.bg, t.Z, 0, MOD_FROM_QM[4], t.Nref)[0] == -1  # E > MAXE
    assert rm.rm_tx(cw, 8, t.bg, t.Z, 0, 7, t.Nref)[0] == -1  # no such modulation
    rm.free()


def test_refusals_then_a_good_encode(sh, tx, sbtx):
    L = S.lib()
    i = 2
    c = sh.case(i)
    tx.set_nof_prb(c["nof_prb"])
    cfg = S.make_cfg(c["lbrm"], c["mcs256"])
    pl = c["pl"]
    e = np.zeros(c["G"], np.uint8)

    def call(q=tx.q, cfg=cfg, tb=None, data=pl.ctypes.data, e_bits=e.ctypes.data, sb=sbtx, tbs=c["tbs"], R=c["R"],
             fn=L.srsran_dlsch_nr_encode):
        tb = S.make_tb(tbs, R, c["Qm"], c["G"], c["Nl"], 0, sb) if tb is None else tb
        return fn(ctypes.byref(q) if q is not None else None, ctypes.byref(cfg) if cfg is not None else None,
                  ctypes.byref(tb) if tb is not False else None, data, e_bits)

    # a NULL pointer among q, sch_cfg, tb, data, e_bits (sch_nr.c:414-416)
    assert call(q=None) == INVALID_INPUTS
    assert call(cfg=None) == INVALID_INPUTS
    assert call(tb=False) == INVALID_INPUTS
    assert call(data=None) == INVALID_INPUTS
    assert call(e_bits=None) == INVALID_INPUTS
    # a missing tx soft buffer (sch_nr.c:418-421)
    assert call(sb=None) == ERROR
    # max_cb < C, max_cb_size < liftN - 2Z (sch_nr.c:447-462)
    t = S.tb_info(c["tbs"], c["R"], c["Qm"], c["G"], c["Nl"])
    assert t.C == 7
    small = S.nr_softbuffer_tx(max_cb=t.C - 1)
    assert call(sb=small) == ERROR
    small.free()
    n = t.Z * (66 if t.bg == 0 else 50)
    short = S.nr_softbuffer_tx(max_cb_size=n - 1)
    assert call(sb=short) == ERROR
    short.free()
    exact = S.nr_softbuffer_tx(max_cb=t.C, max_cb_size=n)
    assert call(sb=exact) == 0
    exact.free()
    # srsran_sch_nr_fill_tb_info failing: more code blocks than SRSRAN_SCH_NR_MAX_NOF_CB_LDPC
    assert call(tbs=400000, R=0.9) == ERROR
    # C > 1 with code blocks that are no whole bytes: (9008 + 24) / 2 = 4516 bits
    assert S.cbsegm_ldpc(0, 9008)["C"] == 2
    assert call(tbs=9008, R=0.9) == ERROR
    assert call(tbs=9000, R=0.9) == 0
    # an object is a transmitter or a receiver
    rx = S.SchNr(nof_prb=c["nof_prb"])
    assert call(q=rx.q) == ERROR
    rx.free()
    sbrx = S.nr_softbuffer()
    ret, _, _, _ = tx.decode(sbrx, c["tbs"], c["R"], c["Qm"], c["G"], c["Nl"], 0, np.zeros(c["G"], np.int8))
    assert ret == ERROR
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert tx.decode_batch([], d.data_ptr(), d.data_ptr()) == ERROR
    sbrx.free()
    # and the object still encodes
    for fn in (L.srsran_dlsch_nr_encode, L.srsran_ulsch_nr_encode):
        e[:] = SENTINEL
        assert call(fn=fn) == 0
        assert np.array_equal(e, sh.want(i, 0))


def test_loop_encode_batch_to_decode_batch_on_the_device(sh, tx, sbtx):
    """rv 0 of every case with R <= 0.75: batch encode, LLR = 10 (1 - 2 bit) as int8 on the device, batch decode."""
    tx.set_nof_prb(273)
    rx = S.SchNr(nof_prb=273, max_nof_iter=10)
    order = [i for i in range(len(CASES)) if CASES[i][1] <= 0.75]
    assert len(order) == 12
    keep = []
    outs = _batch(sh, tx, sbtx, order, [0] * len(CASES), keep)
    entries, sbs, d_pl = [], [], {}
    d_crc = torch.full((len(order),), 77, dtype=torch.uint8, device="cuda")
    d_avg = torch.zeros(len(order), dtype=torch.float32, device="cuda")
    for i in order:
        c = sh.case(i)
        llr = (10 - 20 * outs[i][:c["G"]].to(torch.int16)).to(torch.int8).contiguous()
        sb = S.nr_softbuffer()
        cfg = S.make_cfg(c["lbrm"], c["mcs256"])
        tb = S.make_tb(c["tbs"], c["R"], c["Qm"], c["G"], c["Nl"], 0, sb)
        d_pl[i] = torch.zeros(c["tbs"] // 8 + 8, dtype=torch.uint8, device="cuda")
        keep += [llr, cfg, tb]
        sbs.append(sb)
        entries.append((cfg, tb, llr.data_ptr(), d_pl[i].data_ptr(), 1))
    assert rx.decode_batch(entries, d_crc.data_ptr(), d_avg.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    crc = d_crc.cpu().numpy()
    for k, i in enumerate(order):
        c = sh.case(i)
        assert crc[k] == 1, CASES[i]
        assert np.array_equal(d_pl[i].cpu().numpy()[:c["tbs"] // 8], c["pl"]), CASES[i]
    for sb in sbs:
        sb.free()
    rx.free()
