"""The host-only units behind include/srsran_sch.h (csrc/fec_host.cpp: segmentation, table CRC; csrc/uci_host.cpp: CQI
reports, UCI offset tables, the transmitter's UCI channel coding), no GPU: tools/sch_host_check.cpp built with them
under the address and undefined-behaviour sanitizers runs every function on heap blocks of exactly the length it may
touch, checks the CQI pack -> unpack round trip and prints each result; here the results are compared with the oracle
(pinned to the reference by tests/test_sch_oracle.py) and with the reference's uci.c / block.c compiled into
oracle/_ref (oracle/uci.py).  tests/test_sch_host.py and tests/test_uci_host.py check the same code through the
shared library."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import LTE_CRC24A, LTE_CRC24B, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import uci as RU  # noqa: E402  (oracle/uci.py)
import uci_cases as UC  # noqa: E402
from srsran_4g_amd import sch as S  # noqa: E402  (the ctypes mirrors of the structures only)

needs_ref = pytest.mark.skipif(not RU.ref_available(), reason="oracle/_ref not built")

CSRC = os.path.join(ROOT, "srsran_4g_amd", "csrc")
TBS_ASKED = list(range(0, 400000, 8))[::37] + [75376, 97896, 6120, 6200, 40, 16, 20, 391656, 500000] + \
    [0, 16, 40, 6120, 6144 - 24 - 8, 6144 - 24 + 8, 391656]
CRC_LENGTHS = (1, 7, 8, 9, 64, 6144, 75400)
CRC_POLYS = ((LTE_CRC24A, 24), (LTE_CRC24B, 24), (0x11021, 16), (0x19B, 8))  # phy_common.h:72-75
# 36.213 Tables 8.6.3-1 (HARQ-ACK), 8.6.3-2 (RI), 8.6.3-3 (CQI, indices 0 and 1 reserved)
BETA_ACK = [2.0, 2.5, 3.125, 4.0, 5.0, 6.25, 8.0, 10.0, 12.625, 15.875, 20.0, 31.0, 50.0, 80.0, 126.0]
BETA_RI = [1.25, 1.625, 2.0, 2.5, 3.125, 4.0, 5.0, 6.25, 8.0, 10.0, 12.625, 15.875, 20.0]
BETA_CQI = [None, None, 1.125, 1.25, 1.375, 1.625, 1.75, 2.0, 2.25, 2.5, 2.875, 3.125, 3.5, 4.0, 5.0, 6.25]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("sch_host") / "sch_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "sch_host_check.cpp"), os.path.join(CSRC, "fec_host.cpp"),
                    os.path.join(CSRC, "uci_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        out.setdefault(w[0], []).append(w[1:])
    return out


def bits(s):
    return np.zeros(0, np.uint8) if s == "-" else np.frombuffer(s.encode(), np.uint8) - ord("0")


def test_host_units_take_no_hip_header():
    """they build with a plain C++ compiler because nothing they include, directly or not, is a HIP header"""
    r = subprocess.run([shutil.which("g++"), "-std=c++17", "-M", os.path.join(CSRC, "fec_host.cpp")],
                       capture_output=True, text=True, check=True)
    r2 = subprocess.run([shutil.which("g++"), "-std=c++17", "-M", os.path.join(CSRC, "uci_host.cpp")],
                        capture_output=True, text=True, check=True)
    deps = [os.path.basename(w) for w in (r.stdout + r2.stdout).split() if w.endswith((".h", ".hpp", ".inc"))]
    assert deps and not [d for d in deps if "hip" in d.lower() or d in ("dev_buf.h", "devkey.h")], deps


def test_segmentation_matches_oracle(lines):
    ora = Oracle()
    fields = ("C", "K1", "K2", "K1_idx", "K2_idx", "C1", "C2", "F")
    assert [int(w[0]) for w in lines["cbsegm"]] == TBS_ASKED
    for w in lines["cbsegm"]:
        tbs, rc, got = int(w[0]), int(w[1]), [int(x) for x in w[2:]]
        orc, o = ora.cbsegm(tbs)
        assert rc == orc, tbs
        if rc == 0:
            assert got == [o[f] for f in fields], (tbs, got, o)


def test_crc_matches_oracle(lines):
    ora = Oracle()
    assert [(int(w[0], 16), int(w[1]), int(w[2])) for w in lines["crc"]] == \
        [(p, o, n) for p, o in CRC_POLYS for n in CRC_LENGTHS]
    for w in lines["crc"]:
        poly, order, nbits, got = int(w[0], 16), int(w[1]), int(w[2]), int(w[3], 16)
        data = np.frombuffer(bytes.fromhex("" if w[4] == "-" else w[4]), np.uint8)
        assert data.size == nbits // 8
        assert got == ora.crc_byte(poly, order, np.concatenate([data, np.zeros(1, np.uint8)]), nbits), (poly, nbits)
        if nbits >= 64:
            assert got != 0 or not data.any()


def cqi_case(w):
    """a 'cqi' line -> (srsran_cqi_cfg_t, srsran_cqi_value_t, size, packed length, unpack's return, packed bits)"""
    t, N, L, four, pmi, rank, lab2, size, n, m = (int(x) for x in w[:10])
    c = S.srsran_cqi_cfg_t()
    c.data_enable, c.type, c.N, c.L = True, t, N, L
    c.four_antenna_ports, c.pmi_present, c.rank_is_not_one, c.subband_label_2_bits = four, pmi, rank, lab2
    a = [int(x) for x in w[11:16]]
    v = S.srsran_cqi_value_t()
    if t == UC.WB:
        v.wideband.wideband_cqi, v.wideband.spatial_diff_cqi, v.wideband.pmi = a[:3]
    elif t == UC.SB_UE:
        v.subband_ue.subband_cqi, v.subband_ue.subband_label = a[:2]
    elif t == UC.SB_DIFF:
        v.subband_ue_diff.wideband_cqi, v.subband_ue_diff.subband_diff_cqi = a[:2]
    else:
        h = v.subband_hl
        h.wideband_cqi_cw0, h.subband_diff_cqi_cw0, h.wideband_cqi_cw1, h.subband_diff_cqi_cw1, h.pmi = a
    return c, v, size, n, m, bits(w[10])


def test_cqi_cases_cover_the_reports(lines):
    seen = {tuple(int(x) for x in w[:7]) for w in lines["cqi"]}
    for t in (UC.WB, UC.SB_UE, UC.SB_DIFF, UC.HL):
        for N, L, lab2 in ((1, 2, 0), (13, 6, 1)) if t != UC.WB else ((1, 2, 0),):
            for four in (0, 1):
                for pmi in (0, 1):
                    for rank in (0, 1):
                        assert (t, N, L, four, pmi, rank, lab2) in seen
    assert len(lines["cqi"]) == 8 * 7
    # the largest report fills the buffer to its last bit
    assert max(int(w[8]) for w in lines["cqi"]) == 64


@needs_ref
def test_cqi_matches_reference(lines):
    ref = RU.RefUci()
    for w in lines["cqi"]:
        c, v, size, n, m, packed = cqi_case(w)
        assert size == ref.cqi_size(c), w[:7]
        want = ref.cqi_pack(c, v)
        assert n == len(want) and np.array_equal(packed, want), w[:7]
        # unpack returns the bits read, except that the wideband report answers 4 whatever it read (cqi.c:206); what
        # it unpacked is compared by the program (the round trip)
        assert m == (4 if c.type == UC.WB else n), w[:7]


def test_offset_tables(lines):
    """srsran_sch_beta_* and the three srsran_sch_find_Ioffset_* at every index 0..16, and the probes of
    tests/test_uci_host.py::test_offset_tables"""
    rows = lines["beta"]
    assert [int(w[0]) for w in rows] == list(range(17))

    def getter(tab, lo):  # outside the table: its first valid entry (sch.c:43-95)
        return lambda j: tab[j] if lo <= j < len(tab) else tab[lo]

    def first(get, b):  # the first of 16 indices whose offset reaches b, read through the same getter (sch.c:108-136)
        return next((j for j in range(16) if get(j) >= b), 0)

    get_ack, get_ri, get_cqi = getter(BETA_ACK, 0), getter(BETA_RI, 0), getter(BETA_CQI, 2)
    for w in rows:
        i = int(w[0])
        pub_ack, pub_cqi, ack, ri, cqi = (float(x) for x in w[1:6])
        assert (ack, ri, cqi) == (get_ack(i), get_ri(i), get_cqi(i)), i
        # the public getters answer 0 from index 16 on
        assert (pub_ack, pub_cqi) == ((get_ack(i), get_cqi(i)) if i < 16 else (0.0, 0.0)), i
        assert [int(x) for x in w[6:9]] == [first(get_ack, ack), first(get_ri, ri), first(get_cqi, cqi)], i
    got = {(w[0], float(w[1])): int(w[2]) for w in lines["find"]}
    assert got[("ack", 10.0)] == 7 and got[("ack", 1000.0)] == 0 and got[("cqi", 2.0)] == 7 and got[("ri", 3.0)] == 4
    assert got[("ack", 0.5)] == 0 and got[("ri", 0.5)] == 0 and got[("cqi", 0.5)] == 0
    by = {int(w[0]): w for w in rows}
    assert [float(by[i][1]) for i in (0, 5, 14, 15, 16)] == [2.0, 6.25, 126.0, 2.0, 0.0]
    assert [float(by[i][2]) for i in (0, 2, 7, 15, 16)] == [1.125, 1.125, 2.0, 6.25, 0.0]


@needs_ref
def test_block_code_matches_reference(lines):
    """block_encode against the reference's srsran_block_encode (block.c:78-104)"""
    ref = RU.RefUci()
    u8p = ctypes.POINTER(ctypes.c_uint8)
    ref.L.srsran_block_encode.argtypes = [u8p, ctypes.c_uint32, u8p, ctypes.c_uint32]
    ref.L.srsran_block_encode.restype = None
    assert [(int(w[0]), int(w[1])) for w in lines["block"]] == [(n, q) for n in range(1, 12) for q in (32, 40)]
    for w in lines["block"]:
        nin, nout, i, o = int(w[0]), int(w[1]), bits(w[2]).copy(), bits(w[3])
        want = np.zeros(nout, np.uint8)
        ref.L.srsran_block_encode(i.ctypes.data_as(u8p), nin, want.ctypes.data_as(u8p), nout)
        assert i.size == nin and np.array_equal(o, want), (nin, nout)


@needs_ref
def test_long_cqi_code_matches_reference(lines):
    """cqi_encode_long against the reference's srsran_uci_encode_cqi_pusch (uci.c:225-257, 302-320): a CQI-only PUSCH
    of one PRB (no TB: the CQI takes every symbol) carrying a higher-layer subband report whose packed bits are the
    program's input, sent through the reference transmitter and read back from the interleaver"""
    ref = RU.RefUci()
    assert [int(w[0]) for w in lines["cqilong"]] == [12, 64]
    for w in lines["cqilong"]:
        nbits, Q, i, o = int(w[0]), int(w[1]), bits(w[2]), bits(w[3])
        val = lambda b: int("".join(str(x) for x in b), 2)  # noqa: E731
        if nbits == 12:
            cqi, N = (UC.HL, dict(N=4)), 4
        else:
            cqi, N = (UC.HL, dict(N=13, pmi_present=True, rank_is_not_one=True, four_antenna_ports=True)), 13
        cfg = UC.make_cfg(2, 1, 12, 0, 0, 0, cqi)
        assert Q == cfg.grant.tb.nof_bits
        u = S.srsran_uci_value_t()
        h = u.cqi.subband_hl
        h.wideband_cqi_cw0, h.subband_diff_cqi_cw0 = val(i[:4]), val(i[4:4 + 2 * N])
        if nbits == 64:
            h.wideband_cqi_cw1, h.subband_diff_cqi_cw1, h.pmi = val(i[30:34]), val(i[34:60]), val(i[60:64])
        assert np.array_equal(ref.cqi_pack(cfg.uci_cfg.cqi, u.cqi), i)
        types, (Qri, Qcqi, G, Qack) = ref.tx(cfg, u, np.zeros(0, np.uint8))
        assert (Qri, Qcqi * 2, G, Qack) == (0, Q, 0, 0)
        # ulsch_interleave writes g row by row into q[(column * rows + row) * Qm + bit]
        rows, cols = Q // 2 // 12, 12
        g = types.reshape(cols, rows, 2).transpose(1, 0, 2).ravel()
        assert np.array_equal(o, g), (nbits, np.flatnonzero(o != g)[:8])
