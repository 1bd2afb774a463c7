"""PBCH cases shared by tests/golden/make_pbch_golden.py and the PBCH tests: the smallest sequences of calls at which
each piece of the decoder can go wrong.  Plain numbers only (they are stored as JSON in the fixture).

Per case: the cell (nof_prb, ports = what the cell really transmits, cell id, cp 0 normal / 1 extended, phich_len,
phich_res 0..3 = Ng 1/6, 1/2, 1, 2), search (True: the decoder is given nof_ports = 0), sfn0 (the SFN of the first
call; calls are consecutive radio frames), and per call its SNR in dB (None: noise only, nothing was sent), zero_noise
(the decoder is given a zero noise estimate).  `expect` is the return value the case is built for, per call: the
generator looks for a noise seed with which the reference behaves so."""

R16, R12, R1, R2 = 0, 1, 2, 3
HI = 30.0  # dB: decodes from one frame

FIXTURE = "pbch_golden.npz"
# Larger distance of either reference build's LLRs from the float64 evaluation, relative to max |LLR| of the frame;
# printed by make_pbch_golden.py and stored in the fixture (test_pbch_host.py holds the two equal)
MEASURED = 2.8747408943995964e-07
LLR_TOL = max(4 * MEASURED, 1e-6)


def _case(name, nof_prb, ports, cell_id, sfn0, snr, expect, cp=0, search=False, zero_noise=False, phich_len=0,
          phich_res=R1):
    assert len(snr) == len(expect)
    return dict(name=name, nof_prb=nof_prb, ports=ports, cell_id=cell_id, cp=cp, search=bool(search), sfn0=sfn0,
                snr=list(snr), expect=list(expect), zero_noise=bool(zero_noise), phich_len=phich_len,
                phich_res=phich_res)


CASES = [
    # bandwidth x cell id mod 3 x CP x known port count, one clean frame each; the first frame at every position of
    # the 40 ms period (sfn0 mod 4 = the expected sfn_offset)
    _case("p6_id0_1p", 6, 1, 150, 4, [HI], [1]),
    _case("p6_id1_2p_ext", 6, 2, 301, 9, [HI], [1], cp=1),
    _case("p6_id2_4p", 6, 4, 503, 1022, [HI], [1]),
    _case("p15_id0_2p", 15, 2, 0, 7, [HI], [1], phich_len=1, phich_res=R2),
    _case("p15_id1_4p_ext", 15, 4, 1, 512, [HI], [1], cp=1),
    _case("p15_id2_1p_n0", 15, 1, 2, 1, [HI], [1], zero_noise=True),
    _case("p25_id0_4p_ext", 25, 4, 150, 2, [HI], [1], cp=1, phich_res=R12),
    _case("p25_id1_1p", 25, 1, 301, 3, [HI], [1]),
    _case("p25_id2_2p_ext", 25, 2, 503, 100, [HI], [1], cp=1),
    _case("p100_id0_1p_ext_n0", 100, 1, 0, 1021, [HI], [1], cp=1, zero_noise=True),
    _case("p100_id1_2p", 100, 2, 1, 6, [HI], [1], phich_res=R16),
    _case("p100_id2_4p", 100, 4, 2, 255, [HI], [1]),
    # port search on cells that really have 1, 2 and 4 ports
    _case("search_1p", 25, 1, 151, 5, [HI], [1], search=True),
    _case("search_2p", 6, 2, 2, 10, [HI], [1], search=True),
    _case("search_4p_ext", 15, 4, 302, 3, [HI], [1], cp=1, search=True),
    # combining at low SNR: a miss, then a decode on the second, third, fourth call.  comb3 starts at position 2: its
    # first two frames end a period, the third begins the next one, so the reference must wait for a fourth
    _case("comb2_1p", 25, 1, 150, 8, [-8.0, -8.0], [0, 1]),
    _case("comb3_2p", 15, 2, 301, 16, [-10.0, -10.0, -10.0], [0, 0, 1]),
    _case("comb_straddle", 25, 2, 503, 2, [-8.5, -8.5, -8.5, -8.5], [0, 0, 0, 1]),
    _case("comb4_search", 6, 1, 1, 4, [-11.5, -11.5, -11.5, -11.5], [0, 0, 0, 1], search=True),
    # history shift: five and six misses on noise alone, then a clean frame
    _case("shift5_2p", 15, 2, 2, 1, [None] * 5 + [HI], [0] * 5 + [1]),
    _case("shift6_search", 25, 4, 150, 3, [None] * 6 + [HI], [0] * 6 + [1], search=True),
    # the all-zero MIB: 6 PRB, normal PHICH duration, Ng = 1/6, SFN 0..3
    _case("zero_mib", 6, 1, 0, 0, [HI, HI, HI], [0, 0, 0], phich_res=R16),
]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def nof_symbols(c):
    return 216 if c["cp"] else 240


def re_table(nof_prb, cell_id, cp):
    """36.211 6.6.4: the PBCH occupies the 72 centre subcarriers of symbols 0..3 of slot 1, without the resource
    elements reserved for the cell-specific reference signals of antenna ports 0..3 whatever the real port count:
    subcarriers k with k mod 3 = cell id mod 3 in symbols 0 and 1, and in symbol 3 with the extended CP (there the
    second CRS symbol of ports 0 / 1 is l = 3).  Indices into the subframe's grid [2 nsymb][12 nof_prb], in the
    mapping order (k ascending, then l)."""
    nsymb, nre = (6 if cp else 7), 12 * nof_prb
    out = []
    for l in range(4):
        crs = l in (0, 1) or (l == 3 and cp)
        for k in range(nre // 2 - 36, nre // 2 + 36):
            if not (crs and k % 3 == cell_id % 3):
                out.append((nsymb + l) * nre + k)
    return out
