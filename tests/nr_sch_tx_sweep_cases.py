"""Case lists of the NR SCH transmit sweep (plain Python, no GPU): which transport blocks the sweep encodes.

Everything that depends on TB segmentation comes from a `tb_info(tbs, R, Qm, G, Nl, ...)` callable returning the
fields of srsran_sch_nr_tb_info_t as a dict -- the compiled reference's (RefNr.tb_info) in the tests.  The
bit-selection walk is written out here on its own (the loop of ldpc_rm.c:173-193 over a circular buffer with one
filler range); it shares nothing with csrc/nr_rm_tx_pos.h, whose closed forms the kernel and the planner use.

1. reachable_shapes   every (base graph, Z) a single-block TB of 8 .. 8424 bits reaches, at its smallest and
                      its largest filler count
2. row_edges          per base-graph row r >= 4 the smallest E whose last selected bit lies in row r's parity chunk
3. tb_crc_items       payload lengths at the 16-byte chunk edges, the CRC16 / CRC24A switch and the 4096-byte
                      slice edges of nr_tb_crc.h
4. multi_cb_items     every (base graph, Z) of a TB with C > 1, at its smallest and its largest C
"""
from collections import namedtuple

MAX_NREF = 384 * 66          # SRSRAN_LDPC_MAX_LEN_ENCODED_CB: no limited-buffer rate matching
MAX_NOF_CB = 41              # SRSRAN_SCH_NR_MAX_NOF_CB_LDPC
BG_N = (66, 50)              # stored codeword chunks (the first two punctured)
BG_K = (22, 10)
BG_M = (46, 42)              # base-graph rows
BASEK0 = ((0, 17, 33, 56), (0, 13, 25, 43))  # ldpc_rm.c:50, [bg][rv]
QMS = (1, 2, 4, 6, 8)
RATES = (0.2, 0.5, 0.9)      # the R of a TB only selects its base graph; G sets what is transmitted
TB_SLICE = 4096              # NR_TB_SLICE
TB_CHUNK = 16                # NR_TB_BYTES

# (bg, Z) -> one TB of a single code block
Shape = namedtuple("Shape", "tbs R bg Z F Kp Kr")


def set_index(Z):
    """Lifting-size set index i_LS of Z = a 2^j (38.212 table 5.3.2-1): a = 2, 3, 5, 7, 9, 11, 13, 15."""
    while Z % 2 == 0:
        Z //= 2
    return {1: 0, 3: 1, 5: 2, 7: 3, 9: 4, 11: 5, 13: 6, 15: 7}[Z]


def hr_case(bg, Z):
    """Which of the four high-rate solutions (encode_high_rate_case1..4, ldpc_enc_c.c:110-224) the pair uses."""
    i = set_index(Z)
    if bg == 0:
        return 2 if i == 6 else 1
    return 3 if i in (3, 7) else 4


def accepted(t):
    """The product refuses C > 1 unless every code block carries whole bytes."""
    return t["A"] % 8 == 0 and (t["C"] == 1 or (t["Kp"] - t["L_cb"]) % 8 == 0)


def tiles(t):
    """The code blocks carry the whole TB: B = TBS + L_tb is a multiple of C (and of 8 C: whole bytes).  K' is
    B' / C rounded down (sch_nr.c:145), so an accepted TB need not tile: the transmitter then leaves out the last
    bytes of the payload (sch_nr.c:483-506) while the TB CRC covers all of it, and no receiver, the reference's
    included, finds the TB CRC true (sch_nr.c:739 runs over TBS bits, the last of which never arrive).  The TBS
    tables of 38.214 only give sizes that tile."""
    return accepted(t) and (t["C"] == 1 or t["B"] % (8 * t["C"]) == 0)


def delivered_bytes(t):
    """Payload bytes the code blocks of a TB carry."""
    return (t["C"] * (t["Kp"] - t["L_cb"]) - t["L_tb"]) // 8


def _shape(t, tbs, R):
    return Shape(tbs, R, t["bg"], t["Z"], t["F"], t["Kp"], t["Kr"])


def reachable_shapes(tb_info):
    """{(bg, Z): [Shape with the smallest F, Shape with the largest F]} (one Shape where all F are equal) over
    the byte-aligned TBS 8 .. 8424 at R in RATES that make one code block."""
    seen = {}
    for R in RATES:
        for tbs in range(8, 8424 + 1, 8):
            t = tb_info(tbs, R, 1, 8 * tbs, 1)
            if t["C"] == 1:
                seen.setdefault((t["bg"], t["Z"]), []).append(_shape(t, tbs, R))
    out = {}
    for key in sorted(seen):
        v = sorted(seen[key], key=lambda s: (s.F, s.tbs, s.R))
        out[key] = [v[0]] if v[0].F == v[-1].F else [v[0], v[-1]]
    return out


def k0_ncb(bg, Z, rv, Nref=MAX_NREF):
    """init_rm, ldpc_rm.c:157-164."""
    N = Z * BG_N[bg]
    if N <= Nref:
        return Z * BASEK0[bg][rv], N
    return Z * ((BASEK0[bg][rv] * Nref) // N), Nref


def selection_order(bg, Z, Kp, Kr, rv, Nref=MAX_NREF):
    """Stored-codeword positions in the order bit selection takes them, one period: the walk of
    ldpc_rm.c:185-192 from k0 once round the circle, stepping over the fillers [Kp - 2Z, Kr - 2Z).  The k-th
    selected bit (k = 0, 1, ...) sits at order[k % len(order)]."""
    k0, Ncb = k0_ncb(bg, Z, rv, Nref)
    order = []
    for j in range(Ncb):
        icwd = (k0 + j) % Ncb
        if not Kp - 2 * Z <= icwd < Kr - 2 * Z:
            order.append(icwd)
    return order


def last_position(order, E):
    """Position of the last of E selected bits."""
    return order[(E - 1) % len(order)]


def row_boundary(bg, Z, r):
    """First stored position of the parity chunk of base-graph row r (column bgK + r, two columns punctured)."""
    return (BG_K[bg] + r - 2) * Z


def row_edges(s, rv, Nref=MAX_NREF):
    """[(r, E_r)] for the rows r >= 4 the first lap enters: E_r is the smallest E whose last selected position is
    at or beyond row r's boundary.  Rows at or below the one k0 lies in have no edge (E = 1 is in them already), nor
    have rows beyond Ncb.  Positions rise until the walk wraps, so the last position is the largest one."""
    order = selection_order(s.bg, s.Z, s.Kp, s.Kr, rv, Nref)
    lap1 = wrap_edge(s, rv, Nref) - 1
    edges = []
    for r in range(4, BG_M[s.bg]):
        b = row_boundary(s.bg, s.Z, r)
        if order[0] >= b or order[lap1 - 1] < b:
            continue
        k = next(k for k in range(lap1) if order[k] >= b)
        edges.append((r, k + 1))
    return edges


def wrap_edge(s, rv, Nref=MAX_NREF):
    """The smallest E whose last selected bit lies behind the wrap of the circular buffer."""
    order = selection_order(s.bg, s.Z, s.Kp, s.Kr, rv, Nref)
    for k in range(1, len(order)):
        if order[k] < order[k - 1]:
            return k + 1
    return len(order) + 1


def pick(shapes, bg, Z):
    """The largest-F shape of a pair: fillers inside the span are what separates pos(E - 1) + 1 from k0 + E."""
    return shapes[(bg, Z)][-1]


def round_up(x, m):
    return -(-int(x) // m) * m


def short_G(s, Qm):
    """About 1.1 K': a high rate, which prunes rows."""
    return round_up(-(-11 * s.Kp // 10), Qm)


def long_G(s, Qm, Nref=MAX_NREF):
    """At least 1.3 N (1.3 Ncb of a limited buffer): wraps, and transmits every position."""
    n = min(s.Z * BG_N[s.bg], Nref)
    return round_up(-(-13 * n // 10), Qm)


def lifting_items(shapes):
    """List 1 as encode items without rv: every shape at a short and a long G, Qm cycling by case index."""
    items = []
    for key in sorted(shapes):
        for s in shapes[key]:
            for kind in ("short", "long"):
                Qm = QMS[len(items) % len(QMS)]
                G = short_G(s, Qm) if kind == "short" else long_G(s, Qm)
                items.append(dict(tbs=s.tbs, R=s.R, Qm=Qm, G=G, Nl=1, bg=s.bg, Z=s.Z, kind=kind))
    return items


def lbrm_items(shapes, Nref):
    """The pairs whose N exceeds Nref, each shape at a long and a short G.  Qm stays below 8: the 256QAM table
    would give the carrier another Nref."""
    items = []
    for key in sorted(shapes):
        bg, Z = key
        if Z * BG_N[bg] <= Nref:
            continue
        for s in shapes[key]:
            for kind in ("long", "short"):
                Qm = QMS[(len(items) // 2 + len(items) % 2) % 4]  # both kinds meet every Qm
                G = short_G(s, Qm) if kind == "short" else long_G(s, Qm, Nref)
                items.append(dict(tbs=s.tbs, R=s.R, Qm=Qm, G=G, Nl=1, bg=bg, Z=Z, kind=kind))
    return items


GAPS = (1, 2, 3)
TAIL = 64


def layout(lengths):
    """Offsets of consecutive outputs in one buffer, separated by gaps of 1, 2 and 3 bytes in turn (so the start
    addresses take all four alignments), and the buffer's size with a tail behind the last one."""
    offs, o = [], 0
    for n, length in enumerate(lengths):
        offs.append(o)
        o += length + GAPS[n % 3]
    return offs, o + TAIL


EXHAUSTIVE = ((0, 15), (1, 4), (1, 7), (1, 15))
EDGE_SHAPES = ((0, 26), (1, 32), (1, 36), (1, 64), (0, 384), (1, 384))


def exhaustive_items(shapes, rv):
    """Every E from 1 to Ncb + Z at Qm = 1 for the EXHAUSTIVE pairs."""
    items = []
    for bg, Z in EXHAUSTIVE:
        s = pick(shapes, bg, Z)
        for E in range(1, Z * BG_N[bg] + Z + 1):
            items.append(dict(tbs=s.tbs, R=s.R, Qm=1, G=E, Nl=1, bg=bg, Z=Z, rv=rv))
    return items


def edge_E_values(E_r):
    """Around an edge: E_r - 1, E_r, E_r + 1 at Qm = 1; at Qm = 2 the nearest even values on either side (the
    largest even E below E_r and the smallest at or above it)."""
    below = (E_r - 1) // 2 * 2
    out = [(1, E) for E in (E_r - 1, E_r, E_r + 1) if E >= 1]
    return out + [(2, E) for E in (below, below + 2) if E >= 2]


def edge_items(shapes, rv, pairs=EDGE_SHAPES):
    """The row edges (and the wrap edge) of the EDGE_SHAPES pairs at one rv."""
    items, seen = [], set()
    for bg, Z in pairs:
        s = pick(shapes, bg, Z)
        for r, E_r in row_edges(s, rv) + [("wrap", wrap_edge(s, rv))]:
            for Qm, E in edge_E_values(E_r):
                if (bg, Z, Qm, E) not in seen:
                    seen.add((bg, Z, Qm, E))
                    items.append(dict(tbs=s.tbs, R=s.R, Qm=Qm, G=E, Nl=1, bg=bg, Z=Z, rv=rv, row=r))
    return items


SMALL_BYTE_COUNTS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 478, 479)  # 478: TBS 3824, the last CRC16 size


def slice_edge_counts(tb_info, R, rule=accepted, slices=(1, 2, 3)):
    """For each slice edge 4096 k the nearest payload byte counts below and above it that `rule` admits.  No
    admitted count is an edge itself: these TBs have C > 1 and L_tb = 24, and a TB that tiles needs
    (TBS + 24) / 8 = 4096 k + 3 to be a multiple of C, which it is for none of the C that segmentation gives these
    sizes; their rounded-down K' - 24 is no multiple of 8 either, so the product refuses them (the CPU test
    checks both)."""
    out = []
    for k in slices:
        for step in (-1, 1):
            n = TB_SLICE * k + step
            while not rule(tb_info(8 * n, R, 1, 64 * n, 1)):
                n += step
            out.append(n)
    return out


def _decodable_G(t, Nl, Qm, rv):
    """G of a TB that decodes without noise: about 2.2 K' per block at rv 0, 1.3 N (every position) otherwise;
    G / (Nl Qm) is made no multiple of C > 1, so the blocks take two E values."""
    per_cb = 22 * t["Kp"] // 10 if rv == 0 else 13 * t["Z"] * BG_N[t["bg"]] // 10 + 1
    n = -(-per_cb * t["C"] // (Nl * Qm))
    if t["C"] > 1 and n % t["C"] == 0:
        n += 1
    return n * Nl * Qm


def _tb_item(tb_info, tbs, R, Nl, Qm, rv):
    t = tb_info(tbs, R, Qm, 8 * tbs, Nl)
    return dict(tbs=tbs, R=R, Qm=Qm, G=_decodable_G(t, Nl, Qm, rv), Nl=Nl, bg=t["bg"], Z=t["Z"], C=t["C"], rv=rv,
                tiles=tiles(t), delivered=delivered_bytes(t))


def tb_crc_items(tb_info):
    """List 3: each payload length at rv 0 and at one other rv.  Next to the slice edges both the nearest lengths
    the product accepts and the nearest that tile (the ones a receiver can return)."""
    sizes = [(n, 0.5) for n in SMALL_BYTE_COUNTS[:-2]] + [(n, R) for n in SMALL_BYTE_COUNTS[-2:] for R in (0.2, 0.9)]
    for R in (0.9, 0.2):
        near = slice_edge_counts(tb_info, R) + slice_edge_counts(tb_info, R, tiles)
        sizes += [(n, R) for n in sorted(set(near))]
    items = []
    for i, (n, R) in enumerate(sizes):
        for rv in (0, 1 + i % 3):
            items.append(_tb_item(tb_info, 8 * n, R, 1, QMS[1 + i % 4], rv))
    return items


def multi_cb_pairs(tb_info):
    """{(bg, Z): ((C, TBS, R) at the smallest C, at the largest C)} over every byte-aligned TBS with 1 < C <= 41
    whose whole-byte code blocks tile it; R = 0.9 selects BG1 and R = 0.2 BG2 at these sizes."""
    out = {}
    for R, K_cb in ((0.9, 8448), (0.2, 3840)):
        # C = ceil((TBS + 24) / (K_cb - 24)) (38.212 5.2.2): stay at or below 41 blocks
        for tbs in range(3832, MAX_NOF_CB * (K_cb - 24) - 24 + 1, 8):
            t = tb_info(tbs, R, 1, 8 * tbs, 1)
            assert t["C"] <= MAX_NOF_CB
            if t["C"] > 1 and tiles(t):
                lo, hi = out.get((t["bg"], t["Z"]), ((t["C"], tbs, R), (t["C"], tbs, R)))
                out[(t["bg"], t["Z"])] = (min(lo, (t["C"], tbs, R)), max(hi, (t["C"], tbs, R)))
    return out


def multi_cb_items(tb_info):
    """List 4: each pair at its smallest and its largest C, N_L cycling over 1 .. 4, at rv 0 and one other rv."""
    items = []
    pairs = multi_cb_pairs(tb_info)
    for i, key in enumerate(sorted(pairs)):
        for j, (C, tbs, R) in enumerate(pairs[key]):
            n = 2 * i + j
            for rv in (0, 1 + n % 3):
                items.append(_tb_item(tb_info, tbs, R, 1 + n % 4, QMS[1 + n % 4], rv))
    return items
