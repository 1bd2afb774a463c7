"""GPU NR SCH transmit sweep: srsran_sch_nr_gpu_encode_batch over the case lists of nr_sch_tx_sweep_cases.py
against the reference's transmitter compiled into oracle/_ref (RefNr.encode), every e_bits byte equal.

All outputs of a batch lie in one device buffer preset to a sentinel, 1, 2 and 3 bytes apart in turn, so the
start addresses take every alignment; after the batch every gap byte and the tail still hold the sentinel.  A
batch runs 64-thread workgroups when its largest Z is <= 32 and 256-thread ones otherwise, so the small lifting
sizes are run both among themselves and mixed with larger ones.  The loop tests hand the encoder's output to
srsran_sch_nr_gpu_decode_batch as LLRs without leaving the device."""
import bisect
import time

import numpy as np
import pytest
import torch

import nr_sch as ON
import nr_sch_tx_sweep_cases as K
from nr_sch import RefNr
from srsran_4g_amd import sch_nr as S
from srsran_4g_amd import tdec

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


class Shared:
    """The reference and what it computed, once for the module."""

    def __init__(self):
        self.ref = RefNr()
        self.shapes = K.reachable_shapes(self.ref.tb_info)
        self.pl, self.e = {}, {}

    def payload(self, tbs):
        if tbs not in self.pl:
            self.pl[tbs] = np.random.default_rng(7000 + tbs).integers(0, 256, tbs // 8).astype(np.uint8)
            self.pl[tbs].setflags(write=False)
        return self.pl[tbs]

    def want(self, it, lbrm=False, nof_prb=52):
        key = (it["tbs"], it["R"], it["Qm"], it["G"], it["Nl"], it["rv"], lbrm, nof_prb)
        if key not in self.e:
            e = self.ref.encode(it["tbs"], it["R"], it["Qm"], it["G"], it["Nl"], it["rv"], self.payload(it["tbs"]),
                                lbrm=lbrm, nof_prb=nof_prb, mcs256=it["Qm"] == 8)
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
    q = S.SchNr(nof_prb=52, tx=True)
    yield q
    q.free()


@pytest.fixture(scope="module")
def rx(sh):
    q = S.SchNr(nof_prb=52, max_nof_iter=10)
    yield q
    q.free()


@pytest.fixture(scope="module")
def sbtx(sh):
    sb = S.nr_softbuffer_tx()
    yield sb
    sb.free()


def _report(t0, sh, n0, what):
    print(f"\n[sweep] {what}: {time.perf_counter() - t0:.2f} s, {len(sh.e) - n0} reference encodes")


def _payloads(sh, items):
    """The payloads of a batch in one device buffer (each TBS once), at whatever byte offsets they fall."""
    offs, o = {}, 0
    for it in items:
        if it["tbs"] not in offs:
            offs[it["tbs"]] = o
            o += it["tbs"] // 8
    host = np.empty(o, np.uint8)
    for tbs, at in offs.items():
        host[at:at + tbs // 8] = sh.payload(tbs)
    return torch.from_numpy(host).cuda(), offs


def encode_batch(sh, tx, sbtx, items, lbrm=False):
    """One srsran_sch_nr_gpu_encode_batch over `items` -> (device buffer, offsets)."""
    offs, total = K.layout([it["G"] for it in items])
    d_e = torch.full((total,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_p, p_off = _payloads(sh, items)
    entries = []
    for it, o in zip(items, offs):
        cfg = S.make_cfg(lbrm, it["Qm"] == 8)
        tb = S.make_tb(it["tbs"], it["R"], it["Qm"], it["G"], it["Nl"], it["rv"], sbtx)
        entries.append((cfg, tb, d_p.data_ptr() + p_off[it["tbs"]], d_e.data_ptr() + o))
    assert d_e.data_ptr() % 4 == 0
    assert tx.encode_batch(entries) == 0
    torch.cuda.synchronize()
    return d_e, offs


def check(sh, d_e, offs, items, lbrm=False, nof_prb=52):
    """Every output byte equals the reference's; every byte between and behind the outputs is the sentinel."""
    got = d_e.cpu().numpy()
    exp = np.full_like(got, SENTINEL)
    for it, o in zip(items, offs):
        w = sh.want(it, lbrm, nof_prb)
        assert w.size == it["G"] and w.max() <= 1
        exp[o:o + it["G"]] = w
    if not np.array_equal(got, exp):
        at = int(np.flatnonzero(got != exp)[0])
        n = bisect.bisect_right(offs, at) - 1
        where = at - offs[n]
        kind = "output byte" if where < items[n]["G"] else "sentinel behind"
        pytest.fail(f"{kind} {where} of entry {n} {items[n]} (start alignment {offs[n] % 4}): "
                    f"got {got[at]}, want {exp[at]}; {int((got != exp).sum())} bytes differ in the batch")
    return got


def decode_batch(sh, rx, d_e, offs, items):
    """The encoder's output as LLR = 10 (1 - 2 bit) through srsran_sch_nr_gpu_decode_batch, one soft buffer per
    TB sized for its code blocks: every TB CRC true, every payload back, nothing written beside the payloads.
    An item marked tiles=False (nr_sch_tx_sweep_cases.tiles) is a TB whose code blocks leave out its last bytes:
    there the reference's own receiver decides -- it returns the bytes that were sent and TB CRC false."""
    llr = (10 - 20 * d_e.to(torch.int16)).to(torch.int8).contiguous()
    p_offs, p_total = K.layout([it["tbs"] // 8 for it in items])
    d_pl = torch.full((p_total,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_crc = torch.full((len(items),), 77, dtype=torch.uint8, device="cuda")
    d_avg = torch.zeros(len(items), dtype=torch.float32, device="cuda")
    entries, sbs = [], []
    for it, o, po in zip(items, offs, p_offs):
        sb = S.nr_softbuffer(max_cb=it.get("C", 1))
        cfg = S.make_cfg(False, it["Qm"] == 8)
        tb = S.make_tb(it["tbs"], it["R"], it["Qm"], it["G"], it["Nl"], it["rv"], sb)
        sbs.append(sb)
        entries.append((cfg, tb, llr.data_ptr() + o, d_pl.data_ptr() + po, 1))
    assert rx.decode_batch(entries, d_crc.data_ptr(), d_avg.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    crc, pl = d_crc.cpu().numpy(), d_pl.cpu().numpy()
    exp = np.full_like(pl, SENTINEL)
    want_crc = np.ones(len(items), np.uint8)
    for k, (it, po) in enumerate(zip(items, p_offs)):
        n = it["tbs"] // 8
        if not it.get("tiles", True):
            n = it["delivered"]
            sb = sh.ref.softbuffer()
            sb.reset()
            e = (10 - 20 * sh.want(it).astype(np.int16)).astype(np.int8)
            want_crc[k], _, ref_pl = sh.ref.decode(sb, it["tbs"], it["R"], it["Qm"], it["G"], it["Nl"], it["rv"], e,
                                                   mcs256=it["Qm"] == 8)
            sb.free()
            assert want_crc[k] == 0 and n < it["tbs"] // 8 and np.array_equal(ref_pl[:n], sh.payload(it["tbs"])[:n])
        exp[po:po + n] = sh.payload(it["tbs"])[:n]
    bad = [(it["tbs"], it["R"], it["rv"], it["G"], int(crc[k])) for k, it in enumerate(items) if crc[k] != want_crc[k]]
    assert not bad, (len(bad), bad)
    if not np.array_equal(pl, exp):
        at = int(np.flatnonzero(pl != exp)[0])
        n = bisect.bisect_right(p_offs, at) - 1
        pytest.fail(f"payload buffer byte {at - p_offs[n]} of entry {n} {items[n]}: got {pl[at]}, want {exp[at]}")
    for sb in sbs:
        sb.free()


def _with_rv(items, rv):
    return [dict(it, rv=rv) for it in items]


def test_every_reachable_lifting_size(sh, tx, sbtx):
    """Every (base graph, Z) a single-block TB reaches, at its smallest and largest filler count, rv 0-3, at a
    short G (about 1.1 K': rows pruned) and a long one (>= 1.3 N: wraps); Z <= 32 and Z > 32 as separate batches
    (the two launch widths), and at rv 0 also as one mixed batch."""
    t0, n0 = time.perf_counter(), len(sh.e)
    tx.set_nof_prb(52)
    items = K.lifting_items(sh.shapes)
    assert len({(it["bg"], it["Z"]) for it in items}) == 84
    small = [it for it in items if it["Z"] <= 32]
    large = [it for it in items if it["Z"] > 32]
    split = {}
    for rv in range(4):
        for part in (small, large):
            its = _with_rv(part, rv)
            d_e, offs = encode_batch(sh, tx, sbtx, its)
            got = check(sh, d_e, offs, its)
            if rv == 0:
                for it, o in zip(its, offs):
                    split[(it["tbs"], it["R"], it["Qm"], it["G"])] = got[o:o + it["G"]]
    its = _with_rv(items, 0)
    d_e, offs = encode_batch(sh, tx, sbtx, its)
    got = check(sh, d_e, offs, its)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    for it, o in zip(its, offs):
        assert np.array_equal(got[o:o + it["G"]], split[(it["tbs"], it["R"], it["Qm"], it["G"])]), it
    _report(t0, sh, n0, "every_reachable_lifting_size")


def test_limited_buffer_shapes(sh, tx, sbtx):
    """Limited-buffer rate matching on a 25 PRB carrier (N_ref = 11854, no multiple of any Z here): the 15 pairs
    whose N exceeds it, rv 0-3, a long and a short G."""
    t0, n0 = time.perf_counter(), len(sh.e)
    nref = sh.ref.tb_info(8424, 0.5, 2, 30000, 1, lbrm=True, nof_prb=25)["Nref"]
    assert nref == 11854
    items = K.lbrm_items(sh.shapes, nref)
    assert len({(it["bg"], it["Z"]) for it in items}) == 15
    for it in items:  # the product's TB info against the reference's, field by field
        a = S.tb_info(it["tbs"], it["R"], it["Qm"], it["G"], it["Nl"], lbrm=True, nof_prb=25).as_dict()
        b = sh.ref.tb_info(it["tbs"], it["R"], it["Qm"], it["G"], it["Nl"], lbrm=True, nof_prb=25)
        assert set(a) == set(b) and b["Nref"] == nref
        for f in b:
            assert a[f] == b[f], (f, it)
    tx.set_nof_prb(25)
    try:
        for rv in range(4):
            its = _with_rv(items, rv)
            d_e, offs = encode_batch(sh, tx, sbtx, its, lbrm=True)
            check(sh, d_e, offs, its, lbrm=True, nof_prb=25)
    finally:
        tx.set_nof_prb(52)
    _report(t0, sh, n0, "limited_buffer_shapes")


@pytest.mark.parametrize("rv", range(4))
def test_row_pruning_edges(sh, tx, sbtx, rv):
    """The coupling of the planner's row count to the selection's last position: every E from 1 to Ncb + Z for
    four small shapes, and for six more every E next to a row edge or the wrap (Qm = 1: E_r - 1, E_r, E_r + 1;
    Qm = 2: the even values on either side).  The edge shapes with Z <= 32 run under both launch widths."""
    t0, n0 = time.perf_counter(), len(sh.e)
    tx.set_nof_prb(52)
    its = K.exhaustive_items(sh.shapes, rv)
    assert len(its) == 2331
    d_e, offs = encode_batch(sh, tx, sbtx, its)
    check(sh, d_e, offs, its)
    edges = K.edge_items(sh.shapes, rv)
    assert {(it["bg"], it["Z"]) for it in edges} == set(K.EDGE_SHAPES)
    for its in ([it for it in edges if it["Z"] <= 32], edges):
        d_e, offs = encode_batch(sh, tx, sbtx, its)
        check(sh, d_e, offs, its)
    _report(t0, sh, n0, f"row_pruning_edges[rv {rv}]")


def test_tb_crc_slice_edges(sh, tx, rx, sbtx):
    """Payload lengths next to the 16-byte chunk edges, the CRC16 / CRC24A switch and the 4096-byte slice edges
    of nr_tb_crc.h, and every (base graph, Z) of C > 1 at its smallest and largest C (up to 41 blocks, two E
    values, N_L 1-4): the encode against the reference, then through the decoder, whose nr_tb_kernel uses the
    same slice tables.  Next to a slice edge the nearest length the product accepts can be one whose code blocks
    do not carry the whole TB (4093, 8189, 12272 bytes on BG2, 12286 on BG1); those are encoded like the rest,
    the nearest lengths that do are added, and decode_batch says what the receiver owes for each."""
    t0, n0 = time.perf_counter(), len(sh.e)
    tx.set_nof_prb(52)
    items = K.tb_crc_items(sh.ref.tb_info) + K.multi_cb_items(sh.ref.tb_info)
    assert max(it["C"] for it in items) == K.MAX_NOF_CB and sum(not it["tiles"] for it in items) == 8
    d_e, offs = encode_batch(sh, tx, sbtx, items)
    check(sh, d_e, offs, items)
    decode_batch(sh, rx, d_e, offs, items)
    _report(t0, sh, n0, "tb_crc_slice_edges")


def test_loop_every_shape_decodes(sh, tx, rx, sbtx):
    """The rv 0 long-G entries of the lifting-size sweep (every position transmitted at least once) through the
    batch decoder with one-block soft buffers: every entry decodes, CRC true and payload equal."""
    t0, n0 = time.perf_counter(), len(sh.e)
    tx.set_nof_prb(52)
    items = [it for it in _with_rv(K.lifting_items(sh.shapes), 0) if it["kind"] == "long"]
    assert len(items) == 156 and len({(it["bg"], it["Z"]) for it in items}) == 84
    d_e, offs = encode_batch(sh, tx, sbtx, items)
    check(sh, d_e, offs, items)
    decode_batch(sh, rx, d_e, offs, items)
    _report(t0, sh, n0, "loop_every_shape_decodes")
