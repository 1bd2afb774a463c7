"""PHICH cases shared by tests/golden/make_phich_golden.py and the PHICH tests: the smallest shapes at which each
branch of the transmitter / receiver can go wrong.  Plain numbers only (they are stored as JSON in the fixture).

Per case: the cell (nof_prb, ports, cell id, cp 0 normal / 1 extended, phich_len 0 normal / 1 extended duration,
phich_res 0..3 = Ng 1/6, 1/2, 1, 2, frame 0 FDD / 1 TDD), the REG-table options (mi = PHICH m_i, sf1_6 = the
two-symbol extended duration of TDD subframes 1 / 6), nrx, tti, the items put in order (ngroup, nseq, ack), the
resources queried at the receiver (the sent ones first, then ones on which nothing was sent while neighbours in the
group were) and resources at and above the limits, which both directions must refuse."""

R16, R12, R1, R2 = 0, 1, 2, 3


def _case(name, nof_prb, ports, nrx, cell_id, tti, items, unsent=(), invalid=(), cp=0, phich_len=0, phich_res=R1,
          frame=0, mi=1, sf1_6=False):
    return dict(name=name, nof_prb=nof_prb, ports=ports, nrx=nrx, cell_id=cell_id, tti=tti, cp=cp, phich_len=phich_len,
                phich_res=phich_res, frame=frame, mi=mi, sf1_6=bool(sf1_6), items=[list(i) for i in items],
                unsent=[list(u) for u in unsent], invalid=[list(i) for i in invalid])


CASES = [
    # 6 PRB, Ng = 1/6: one group; all 8 sequences superposed with mixed ACK / NACK
    _case("p6_ng16_1p_all8", 6, 1, 1, 0, 0, [(0, s, a) for s, a in zip(range(8), (1, 0, 0, 1, 1, 1, 0, 0))],
          phich_res=R16, invalid=[(0, 8), (1, 0), (0, 9), (7, 7)]),
    # 6 PRB, Ng = 2: two groups, 2 ports, 2 rx; resources left empty beside used ones; the REG index wraps (id 150)
    _case("p6_ng2_2p_2rx", 6, 2, 2, 150, 4, [(0, 0, 1), (0, 3, 0), (1, 6, 1), (0, 5, 1), (1, 1, 0)],
          unsent=[(0, 1), (1, 0), (1, 7)], phich_res=R2, invalid=[(2, 0), (1, 8)]),
    # 15 PRB, 4 ports, cell id 503, subframe 9
    _case("p15_4p", 15, 4, 1, 503, 9, [(0, 2, 1), (1, 7, 0), (1, 4, 1), (0, 6, 0)], unsent=[(0, 0)], phich_res=R1),
    # 25 PRB, Ng = 1: four groups, two items in one group
    _case("p25_ng1_2p", 25, 2, 1, 1, 4, [(3, 0, 0), (0, 4, 1), (3, 5, 1), (2, 7, 1)], unsent=[(1, 0), (3, 1)],
          phich_res=R1, invalid=[(4, 0), (3, 8)]),
    # 100 PRB, Ng = 2: 25 groups (index range)
    _case("p100_ng2_1p", 100, 1, 1, 150, 0, [(0, 1, 1), (12, 6, 0), (24, 7, 1), (24, 0, 0), (17, 3, 1)],
          unsent=[(24, 1), (5, 0)], phich_res=R2, invalid=[(25, 0), (24, 8)]),
    # extended CP: the even and the odd group of one mapping unit at once, 1 port
    _case("extcp_1p", 6, 1, 1, 0, 0, [(0, 0, 1), (1, 3, 0), (0, 2, 0), (1, 1, 1), (3, 0, 1)], unsent=[(2, 0), (0, 1)],
          cp=1, phich_res=R2, invalid=[(4, 0), (0, 4), (3, 7)]),
    # extended CP, 2 ports, 2 rx
    _case("extcp_2p_2rx", 15, 2, 2, 503, 9, [(1, 1, 0), (0, 1, 1), (3, 2, 1), (2, 3, 0)], unsent=[(1, 0)], cp=1,
          phich_res=R1),
    # extended CP, 4 ports
    _case("extcp_4p", 6, 4, 1, 150, 4, [(0, 3, 1), (1, 0, 0), (1, 2, 1)], unsent=[(0, 0)], cp=1, phich_res=R1),
    # extended duration: REGs in symbols 0..2, 4 ports (two REGs a PRB in symbol 1)
    _case("extdur_4p", 15, 4, 2, 150, 0, [(0, 0, 1), (1, 5, 0), (1, 2, 1)], unsent=[(0, 4)], phich_len=1, phich_res=R1),
    # extended duration, 2 ports, 6 PRB (4 control symbols)
    _case("extdur_2p_p6", 6, 2, 1, 503, 4, [(0, 7, 0), (0, 1, 1)], unsent=[(0, 2)], phich_len=1, phich_res=R1),
    # TDD subframe 1: the two-symbol variant of the extended duration
    _case("tdd_sf1_2sym", 25, 2, 1, 150, 1, [(0, 0, 1), (3, 6, 0), (1, 1, 1), (2, 3, 0)], unsent=[(3, 0)], phich_len=1,
          phich_res=R1, frame=1, sf1_6=True),
    # m_i = 2 (TDD configuration 0, subframe 0): groups of I_phich = 1 lie above ngroups_m1
    _case("mi2_iphich1", 15, 1, 2, 503, 0, [(0, 0, 1), (2, 4, 0), (3, 7, 1), (2, 1, 1)], unsent=[(1, 0), (3, 0)],
          phich_res=R1, frame=1, mi=2, invalid=[(4, 0)]),
    # m_i = 0: the subframe has no PHICH, every resource is refused
    _case("mi0_none", 6, 1, 1, 0, 3, [], phich_res=R1, frame=1, mi=0, invalid=[(0, 0), (1, 3)]),
]

# srsran_phich_calc sweep: (case name, n_prb_lowest 0 .. nof_prb - 1, n_dmrs 0 .. 7, I_phich)
CALC = [("p6_ng16_1p_all8", 0), ("p25_ng1_2p", 0), ("p100_ng2_1p", 0), ("extcp_1p", 0), ("mi2_iphich1", 1)]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def queries(c):
    """resources asked of the receiver: the sent ones in put order (a case puts a resource at most once), then the
    unsent ones"""
    seen, out = set(), []
    for g, s, _ in c["items"]:
        if (g, s) not in seen:
            seen.add((g, s))
            out.append([g, s])
    return out + [list(u) for u in c["unsent"]]
