"""Case table and float64 model of the PUSCH transmit tests (tests/test_pusch_tx_host.py, test_pusch_tx_gpu.py,
test_ue_ul_gpu.py, test_ue_enb_ul_loop_gpu.py).

Every case is one transmitted subframe; the shapes are the smallest at which each piece of the transmit chain can
still go wrong:

  t1    6-PRB cell, L = 1 at the top PRB, QPSK, no UCI        M = 12, grid edge, integer nof_prb / 15 = 0 in the norm
  t2    15-PRB, L = 2, 16QAM, 1 ACK bit                        [o y x x] placeholders; radices 4 2 3
  t3    15-PRB, extended CP, L = 3, QPSK, 2 ACK + 1-bit RI      RI skipping in the interleaver; extended-CP column sets
  t4    25-PRB, L = 5, 64QAM, shortened, 4-bit wideband CQI     radix 5; 11 symbols; Q'_CQI Qm not a multiple of 8
  t5    25-PRB, L = 6, n_prb_tilde[0] != n_prb_tilde[1] != n_prb, sequence hopping     mapper and DMRS put per slot
  t6    25-PRB, L = 4, 16-bit subband CQI + 2-bit RI + 2 ACK, 64QAM     convolutional CQI path, all three UCI kinds
  t7    15-PRB, L = 2, tbs = 0 with CQI and ACK                 CQI-only beta division, no TB
  t8    25-PRB, L = 25, a 64QAM grant with enable_64qam = false the write-back
  t9    25-PRB, L = 20, 16QAM, 2 code blocks, CQI + ACK, G' odd CB CRC, per-CB E, ACK over multi-CB data
  t10   100-PRB, L = 100, QPSK                                  M = 1200, the largest LDS footprint
  t11a  25-PRB, L = 6, 16QAM, rv 0
  t11b  rv 2 of the same payload                                re-encoding from the data

The fixture (tests/golden/pusch_tx_golden.npz, written by tests/golden/make_pusch_tx_golden.py) holds, per case, what
the compiled reference transmitter gave: srsran_ulsch_encode's return, K_segm, packed g and q bits, then
srsran_pusch_encode's written-back tb.mod / tb.nof_bits, scrambled bits, modulation symbols (cases of at most 6 PRB)
and, after srsran_refsignal_dmrs_pusch_put, the grid's columns between the grant's lowest and highest subcarrier.
Two builds of the reference agree in every bit and return value, or the generator writes nothing; t11b was read by
the reference from the transmit soft buffer t11a filled.

The model (tx_model) is the numpy transmitter of tests/pusch_tx.py without its channel: the reference's own UCI
encoder and interleaver (uci.c compiled into oracle/_ref, driven by oracle/ref_uci_harness.c), the oracle's UL-SCH
encoder, scrambling with the placeholder rule, modulation, a float64 DFT / sqrt(M), the mapper and the oracle's DMRS.
tests/test_pusch_tx_host.py holds it to the fixture on the CPU.

Tolerances.  Bits are compared for equality.  MEASURED is, per float quantity, the largest distance of either
reference build from a float64 evaluation of the same formulas (d: max |x - x64| / max |x64|; grid: max |x - x64| /
rms(x64) over the grant's data REs).  The tests allow max(4 x MEASURED, 1e-6 of the largest value): the reference's
own float rounding is the yardstick, 4 x covers another summation order, and 1e-6 max|x| is one float rounding of
the inputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import pusch_cases as PC  # noqa: E402

WB, HL = 0, 3  # SRSRAN_CQI_TYPE_WIDEBAND, SRSRAN_CQI_TYPE_SUBBAND_HL

FIXTURE = "pusch_tx_golden.npz"
# ---- measured by tests/golden/make_pusch_tx_golden.py (its last lines print this table; test_pusch_tx_host.py holds it
# to the copy inside the fixture): the largest distance of either reference build from the float64 evaluation
MEASURED = dict(
    d=6.283e-08,
    grid=2.525e-07,
)
FLOOR = 1e-6                              # of the largest value: one float rounding of the inputs
D_TOL = max(4 * MEASURED["d"], FLOOR)     # modulation symbols: max |got - want| / max |want|
GRID_TOL = 4 * MEASURED["grid"]           # grid: max |got - want| / rms(want) over the grant's data REs, or FLOOR max / rms
GRID_FLOOR = FLOOR


def case(name, nof_prb, cell_id, L, n_prb, Qm, i_tbs, cp=0, tti=0, shortened=False, dmrs=(0, 0, False, False), n_dmrs=0,
         nack=0, ri=0, cqi=None, n_tilde=None, rv=0, enable_64qam=True, seed=0, payload_of=None, rnti=0x46):
    """i_tbs: the TBS index of the grant's TBS at L PRB (-1: no TB); n_tilde: (slot 0, slot 1) or None = n_prb"""
    return dict(name=name, nof_prb=nof_prb, cell_id=cell_id, L=L, n_prb=n_prb, Qm=Qm, i_tbs=i_tbs, cp=cp, tti=tti,
                shortened=shortened, dmrs=dmrs, n_dmrs=n_dmrs, nack=nack, ri=ri, cqi=cqi,
                n_tilde=(n_prb, n_prb) if n_tilde is None else n_tilde, rv=rv, enable_64qam=enable_64qam, seed=seed,
                payload_of=payload_of, rnti=rnti)


CASES = [
    case("t1", 6, 3, 1, 5, 2, 5, tti=0, seed=1),
    case("t2", 15, 150, 2, 6, 4, 10, tti=4, dmrs=(1, 3, True, False), n_dmrs=2, nack=1, seed=2),
    case("t3", 15, 77, 3, 11, 2, 4, cp=1, tti=5, dmrs=(2, 5, False, True), n_dmrs=1, nack=2, ri=1, seed=3),
    case("t4", 25, 501, 5, 7, 6, 20, tti=9, shortened=True, dmrs=(3, 11, True, False), n_dmrs=4, cqi=(WB, dict()), seed=4),
    case("t5", 25, 29, 6, 19, 2, 6, tti=7, dmrs=(7, 29, False, True), n_dmrs=7, n_tilde=(2, 13), seed=5),
    case("t6", 25, 30, 4, 8, 6, 18, tti=3, dmrs=(4, 7, True, False), n_dmrs=3, nack=2, ri=2, cqi=(HL, dict(N=6)), seed=6),
    case("t7", 15, 44, 2, 3, 2, -1, tti=6, dmrs=(1, 9, True, False), n_dmrs=2, nack=1, cqi=(WB, dict(pmi_present=True)),
         seed=7),
    case("t8", 25, 30, 25, 0, 6, 14, tti=2, dmrs=(4, 7, True, False), n_dmrs=3, enable_64qam=False, seed=8),
    case("t9", 25, 9, 20, 2, 4, 15, tti=8, dmrs=(5, 17, False, True), n_dmrs=5, nack=1, cqi=(WB, dict()), seed=9),
    case("t10", 100, 10, 100, 0, 2, 6, tti=1, dmrs=(6, 20, True, False), n_dmrs=6, seed=10),
    case("t11a", 25, 57, 6, 12, 4, 9, tti=8, dmrs=(0, 2, True, False), seed=11),
    case("t11b", 25, 57, 6, 12, 4, 9, tti=8, dmrs=(0, 2, True, False), seed=11, rv=2, payload_of="t11a"),
]
BY_NAME = {c["name"]: c for c in CASES}


def data_rows(c):
    """grid symbols that carry PUSCH data (pusch_cp, pusch.c:48-95)"""
    import pusch as OP
    return OP.data_symbols(c["cp"], c["shortened"])


def columns(c):
    """the grid columns the fixture stores: from the grant's lowest to its highest subcarrier over both slots"""
    return 12 * min(c["n_tilde"]), 12 * (max(c["n_tilde"]) + c["L"])


def tbs_of(c):
    from srsran_4g_amd import pdcch
    return 0 if c["i_tbs"] < 0 else int(pdcch.lib().srsran_ra_tbs_from_idx(c["i_tbs"], c["L"]))


def make(c, softbuffer=None):
    """-> (cell, dmrs cfg, sf cfg, pusch cfg) of the case, as the library's ctypes structures"""
    import pusch_tx as TX
    from srsran_4g_amd import pusch as P
    from srsran_4g_amd.ue_dl import cell as make_cell
    cell = make_cell(nof_prb=c["nof_prb"], cell_id=c["cell_id"])
    cell.cp = c["cp"]
    d = P.srsran_refsignal_dmrs_pusch_cfg_t()
    d.cyclic_shift, d.delta_ss, d.group_hopping_en, d.sequence_hopping_en = c["dmrs"]
    sf = P.srsran_ul_sf_cfg_t()
    sf.tti, sf.shortened = c["tti"], c["shortened"]
    cfg = TX.make_cfg(c["nof_prb"], c["Qm"], c["L"], c["n_prb"], tbs_of(c), c["nack"], c["ri"], c["cqi"], cp=c["cp"],
                      shortened=c["shortened"], rnti=c["rnti"], n_dmrs=c["n_dmrs"], rv=c["rv"], softbuffer=softbuffer)
    cfg.grant.n_prb_tilde[0], cfg.grant.n_prb_tilde[1] = c["n_tilde"]
    cfg.enable_64qam = c["enable_64qam"]
    return cell, d, sf, cfg


def ue_cfg(c, cfg, d, mode=0, peak=0.0, cfo=None):
    """srsran_ue_ul_cfg_t with a grant: the PUSCH and DMRS configurations copied in, the normalize mode, the CFO"""
    import ctypes
    from srsran_4g_amd import ue_ul as UL
    u = UL.srsran_ue_ul_cfg_t()
    ctypes.memmove(ctypes.byref(u.ul_cfg.pusch), ctypes.byref(cfg), ctypes.sizeof(cfg))
    ctypes.memmove(ctypes.byref(u.ul_cfg.dmrs), ctypes.byref(d), ctypes.sizeof(d))
    u.grant_available = True
    u.normalize_mode, u.force_peak_amplitude = mode, peak
    if cfo is not None:
        u.cfo_en, u.cfo_value = True, cfo
    return u


def payload_uci(c, cfg):
    """the case's payload and UCI value, from its seed (t11b shares t11a's)"""
    import uci_cases as UC
    rng = np.random.default_rng(7000 + (BY_NAME[c["payload_of"]] if c["payload_of"] else c)["seed"])
    payload = rng.integers(0, 256, cfg.grant.tb.tbs // 8, dtype=np.uint8)
    return payload, UC.random_uci(cfg, rng)


class Fixture:
    """tests/golden/pusch_tx_golden.npz"""

    def __init__(self):
        import json
        self.z = np.load(os.path.join(HERE, "golden", FIXTURE))
        self.measured = json.loads(bytes(self.z["measured"]).decode())

    def has(self, c, key):
        return key + "." + c["name"] in self.z.files

    def get(self, c, key):
        return self.z[key + "." + c["name"]]

    def uci(self, c):
        from srsran_4g_amd import sch as S
        return S.srsran_uci_value_t.from_buffer_copy(self.get(c, "uci").tobytes())

    def grid(self, c):
        """the whole subframe grid (zeros outside the stored columns)"""
        g = self.get(c, "grid")
        lo, hi = columns(c)
        full = np.zeros((g.shape[0], 12 * c["nof_prb"]), np.complex64)
        full[:, lo:hi] = g
        return full


def pack(bits):
    return np.packbits(np.asarray(bits, np.uint8))


def tx_model(po, c, cfg, payload, u):
    """float64 / bit model of srsran_pusch_encode + the DMRS put for configuration cfg (64QAM limit already applied
    by the caller when the case has it) -> dict(ret, types, q, s, d, grid, dmrs, rows, Qri, Qcqi, Qack, G, e)"""
    import pusch as OP
    import uci as RU
    from synth.synth import modulate
    ref = RU.RefUci()
    Qm = {1: 2, 2: 4, 3: 6}[cfg.grant.tb.mod]
    tbs, L, cp = cfg.grant.tb.tbs, cfg.grant.L_prb, c["cp"]
    Qri, Qcqi, G = ref.tx_sizes(cfg, u)
    e = po.ora.dlsch_encode(tbs, Qm, cfg.grant.tb.rv, G * Qm, payload) if tbs else np.zeros(0, np.uint8)
    types, sizes = ref.tx(cfg, u, e)
    nb = types.size
    seq = po.ora.sequence_bits(OP.pusch_seed(cfg.rnti, 2 * (c["tti"] % 10), c["cell_id"]), nb)
    t = np.asarray(types)
    q = np.where(t <= 1, t, 0).astype(np.uint8)
    s = q ^ seq
    s[t == RU.TYPE_PLACEHOLDER] = 1
    rep = np.nonzero((t == RU.TYPE_REPETITION) & (np.arange(nb) > 1))[0]
    s[rep] = s[rep - 1]
    d = np.asarray(modulate(s, Qm), np.complex128)  # complex64 table values: the transform below must run in double
    M, nsym = 12 * L, OP.nsymb_slot(cp)
    grid = np.zeros((2 * nsym, 12 * c["nof_prb"]), np.complex128)
    rows = OP.data_symbols(cp, c["shortened"])
    assert len(rows) * M == d.size
    for i, g in enumerate(rows):
        n0 = cfg.grant.n_prb_tilde[g // nsym] * 12
        grid[g, n0:n0 + M] = np.fft.fft(d[i * M:(i + 1) * M]) / np.sqrt(M)
    cs, dss, gh, sh = c["dmrs"]
    r = po.dmrs(c["cell_id"], cp, cs, dss, gh, sh, L, c["tti"] % 10, cfg.grant.n_dmrs)
    return dict(ret=(sizes[3] + Qri) * Qm, types=t, q=q, s=s, d=d, grid=grid, dmrs=np.asarray(r), rows=rows, Qri=Qri,
                Qcqi=Qcqi, Qack=sizes[3], G=G, e=np.asarray(e, np.uint8), Qm=Qm, M=M, nsym=nsym)


def grant_mask(c, m):
    """boolean grid masks (data REs, DMRS REs) of the case's grant"""
    ns2, nre = 2 * m["nsym"], 12 * c["nof_prb"]
    data, dm = np.zeros((ns2, nre), bool), np.zeros((ns2, nre), bool)
    for g in m["rows"]:
        n0 = c["n_tilde"][g // m["nsym"]] * 12
        data[g, n0:n0 + m["M"]] = True
    for sl in (0, 1):
        n0 = c["n_tilde"][sl] * 12
        dm[(sl + 1) * m["nsym"] - 4, n0:n0 + m["M"]] = True
    return data, dm


def grid_dist(got, want):
    """(distance, bound): max |got - want| / rms(want) over the given REs against max(GRID_TOL, GRID_FLOOR max / rms)"""
    rms = float(np.sqrt(np.mean(np.abs(want) ** 2)))
    return float(np.abs(got - want).max() / rms), max(GRID_TOL, GRID_FLOOR * float(np.abs(want).max()) / rms)
