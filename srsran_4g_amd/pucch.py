"""Python mirror of the PUCCH receive C API (include/srsran_pucch.h): the resource helpers, the PUCCH
channel estimator (chest_ul.c:462-610), srsran_pucch_decode (pucch.c:797-872) and the added batch call
that does srsran_enb_ul_get_pucch (enb_ul.c:156-273) for many UEs in one launch.  No CPU fallback."""
import ctypes

import numpy as np

from .pusch import lib as _pusch_lib
from .pusch import srsran_chest_ul_res_t, srsran_chest_ul_t, srsran_ul_sf_cfg_t
from .sch import srsran_uci_cfg_t, srsran_uci_value_t
from .ue_dl import srsran_cell_t

u32 = ctypes.c_uint32
_f = ctypes.c_float
_b = ctypes.c_bool
_cfp = ctypes.c_void_p  # cf_t*

FORMAT_1, FORMAT_1A, FORMAT_1B, FORMAT_2, FORMAT_2A, FORMAT_2B, FORMAT_3, FORMAT_ERROR = range(8)
MODE_NORMAL, MODE_CS, MODE_PUCCH3 = range(3)
NcsTable = (u32 * 7) * 20


class srsran_pucch_cfg_t(ctypes.Structure):
    _fields_ = [("rnti", ctypes.c_uint16), ("uci_cfg", srsran_uci_cfg_t), ("delta_pucch_shift", u32), ("n_rb_2", u32),
                ("N_cs", u32), ("N_pucch_1", u32), ("group_hopping_en", _b), ("I_sr", u32), ("sr_configured", _b),
                ("n_pucch_1", u32 * 4), ("n_pucch_2", u32), ("n_pucch_sr", u32), ("simul_cqi_ack", _b),
                ("tdd_ack_multiplex", _b), ("sps_enabled", _b), ("ack_nack_feedback_mode", ctypes.c_int),
                ("n1_pucch_an_cs", (u32 * 2) * 4), ("n3_pucch_an_list", u32 * 4), ("threshold_format1", _f),
                ("threshold_data_valid_format1a", _f), ("threshold_data_valid_format2", _f),
                ("threshold_data_valid_format3", _f), ("threshold_dmrs_detection", _f), ("meas_ta_en", _b),
                ("use_cedron_alg", _b), ("format", ctypes.c_int), ("n_pucch", ctypes.c_uint16),
                ("pucch2_drs_bits", ctypes.c_uint8 * 64)]


class srsran_pucch_t(ctypes.Structure):
    _fields_ = [("cell", srsran_cell_t), ("is_ue", _b), ("n_cs_cell", NcsTable), ("f_gh", u32 * 20),
                ("gpu", ctypes.c_void_p)]


class srsran_pucch_res_t(ctypes.Structure):
    _fields_ = [("uci_data", srsran_uci_value_t), ("dmrs_correlation", _f), ("snr_db", _f), ("rssi_dbFs", _f),
                ("ni_dbFs", _f), ("correlation", _f), ("detected", _b), ("ta_valid", _b), ("ta_us", _f)]


class srsran_pucch_gpu_ue_t(ctypes.Structure):
    _fields_ = [("chest", ctypes.POINTER(srsran_chest_ul_t)), ("sf", ctypes.POINTER(srsran_ul_sf_cfg_t)),
                ("cfg", ctypes.POINTER(srsran_pucch_cfg_t)), ("d_sf_symbols", ctypes.c_void_p)]


_bound = False


def lib():
    global _bound
    L = _pusch_lib()
    if not _bound:
        CELL = ctypes.POINTER(srsran_cell_t)
        CFG = ctypes.POINTER(srsran_pucch_cfg_t)
        UCFG = ctypes.POINTER(srsran_uci_cfg_t)
        UVAL = ctypes.POINTER(srsran_uci_value_t)
        PU = ctypes.POINTER(srsran_pucch_t)
        SF = ctypes.POINTER(srsran_ul_sf_cfg_t)
        RES = ctypes.POINTER(srsran_pucch_res_t)
        NCS = ctypes.POINTER(NcsTable)
        P32 = ctypes.POINTER(u32)
        sig = {
            "srsran_pucch_n_prb": ([CELL, CFG, u32], u32),
            "srsran_pucch_m": ([CFG, ctypes.c_int], u32),
            "srsran_pucch_n_cs_cell": ([srsran_cell_t, NCS], ctypes.c_int),
            "srsran_pucch_alpha_format1": ([NCS, CFG, ctypes.c_int, _b, u32, u32, P32, P32], _f),
            "srsran_pucch_alpha_format2": ([NCS, CFG, u32, u32], _f),
            "srsran_pucch_format2ab_mod_bits": ([ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), _cfp], ctypes.c_int),
            "srsran_pucch_nof_ack_format": ([ctypes.c_int], u32),
            "srsran_pucch_cfg_isvalid": ([CFG, u32], _b),
            "srsran_pucch_cfg_assert": ([CELL, CFG], ctypes.c_int),
            "srsran_pucch_collision": ([CELL, CFG, CFG], ctypes.c_int),
            "srsran_pucch_format_text": ([ctypes.c_int], ctypes.c_char_p),
            "srsran_pucch_format_text_short": ([ctypes.c_int], ctypes.c_char_p),
            "srsran_pucch_proc_select_format": ([CELL, CFG, UCFG, UVAL], ctypes.c_int),
            "srsran_pucch_proc_get_resources": ([CELL, CFG, UCFG, UVAL, P32], ctypes.c_int),
            "srsran_pucch_proc_get_npucch": ([CELL, CFG, UCFG, UVAL, ctypes.POINTER(ctypes.c_uint8)], u32),
            "srsran_pucch_cs_get_ack": ([CFG, UCFG, u32, ctypes.POINTER(ctypes.c_uint8), UVAL], ctypes.c_int),
            "srsran_refsignal_dmrs_N_rs": ([ctypes.c_int, ctypes.c_int], u32),
            "srsran_refsignal_dmrs_pucch_symbol": ([u32, ctypes.c_int, ctypes.c_int], u32),
            "srsran_pucch_init_enb": ([PU], ctypes.c_int),
            "srsran_pucch_free": ([PU], None),
            "srsran_pucch_set_cell": ([PU, srsran_cell_t], ctypes.c_int),
            "srsran_chest_ul_estimate_pucch": ([ctypes.POINTER(srsran_chest_ul_t), SF, CFG, _cfp,
                                                ctypes.POINTER(srsran_chest_ul_res_t)], ctypes.c_int),
            "srsran_pucch_decode": ([PU, SF, CFG, ctypes.POINTER(srsran_chest_ul_res_t), _cfp, RES], ctypes.c_int),
            "srsran_pucch_gpu_get_batch": ([PU, u32, ctypes.POINTER(srsran_pucch_gpu_ue_t), RES], ctypes.c_int),
            "srsran_pucch_init_ue": ([PU], ctypes.c_int),
            "srsran_pucch_encode": ([PU, SF, CFG, UVAL, _cfp], ctypes.c_int),
            "srsran_refsignal_dmrs_pucch_gen_cell": ([CELL, SF, CFG, _cfp], ctypes.c_int),
            "srsran_refsignal_dmrs_pucch_put_cell": ([CELL, CFG, _cfp, _cfp], ctypes.c_int),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _bound = True
    return L


def default_cfg(rnti=0x46):
    """A srsran_pucch_cfg_t with the default thresholds (pucch.h:55-58), DMRS detection off, delta_shift 1."""
    c = srsran_pucch_cfg_t()
    c.rnti = rnti
    c.delta_pucch_shift = 1
    c.threshold_format1 = c.threshold_data_valid_format1a = 0.5
    c.threshold_data_valid_format2 = c.threshold_data_valid_format3 = 0.5
    return c


def n_cs_cell(cell):
    t = NcsTable()
    assert lib().srsran_pucch_n_cs_cell(cell, ctypes.byref(t)) == 0
    return t


class Pucch:
    """srsran_pucch_t of one eNB worker; raises RuntimeError without a HIP device."""

    def __init__(self, cell):
        self.q = srsran_pucch_t()
        L = lib()
        if L.srsran_pucch_init_enb(ctypes.byref(self.q)) != 0:
            raise RuntimeError("srsran_pucch_init_enb failed: no HIP device?")
        if L.srsran_pucch_set_cell(ctypes.byref(self.q), cell) != 0:
            self.free()
            raise ValueError("srsran_pucch_set_cell: invalid cell")

    def decode(self, sf, cfg, chest_res, grid, res=None):
        """srsran_pucch_decode on a host grid; returns (ret, srsran_pucch_res_t)."""
        g = np.ascontiguousarray(grid, dtype=np.complex64)
        res = res if res is not None else srsran_pucch_res_t()
        ret = lib().srsran_pucch_decode(ctypes.byref(self.q), ctypes.byref(sf), ctypes.byref(cfg),
                                        ctypes.byref(chest_res), g.ctypes.data, ctypes.byref(res))
        return ret, res

    def get_batch(self, entries):
        """entries: (srsran_chest_ul_t, srsran_ul_sf_cfg_t, srsran_pucch_cfg_t, device pointer of the grid).
        One launch; returns (ret, array of srsran_pucch_res_t).  The cfgs are written as the reference does."""
        n = len(entries)
        ues = (srsran_pucch_gpu_ue_t * max(n, 1))()
        res = (srsran_pucch_res_t * max(n, 1))()
        for i, (chest, sf, cfg, dptr) in enumerate(entries):
            ues[i].chest = ctypes.pointer(chest)
            ues[i].sf = ctypes.pointer(sf)
            ues[i].cfg = ctypes.pointer(cfg)
            ues[i].d_sf_symbols = dptr
        ret = lib().srsran_pucch_gpu_get_batch(ctypes.byref(self.q), n, ues, res)
        return ret, res

    def free(self):
        if self.q.gpu:
            lib().srsran_pucch_free(ctypes.byref(self.q))


class PucchUe(Pucch):
    """srsran_pucch_t initialised for the UE side (transmit); raises RuntimeError without a HIP device."""

    def __init__(self, cell):
        self.q = srsran_pucch_t()
        self.cell = cell
        L = lib()
        if L.srsran_pucch_init_ue(ctypes.byref(self.q)) != 0:
            raise RuntimeError("srsran_pucch_init_ue failed: no HIP device?")
        if L.srsran_pucch_set_cell(ctypes.byref(self.q), cell) != 0:
            self.free()
            raise ValueError("srsran_pucch_set_cell: invalid cell")

    def encode(self, sf, cfg, uci_value, grid):
        """srsran_pucch_encode into the host grid (contiguous complex64 array, modified in place)"""
        return lib().srsran_pucch_encode(ctypes.byref(self.q), ctypes.byref(sf), ctypes.byref(cfg),
                                         ctypes.byref(uci_value), grid.ctypes.data)

    def put_dmrs(self, sf, cfg, grid):
        """srsran_refsignal_dmrs_pucch_gen_cell + _put_cell into the host grid; returns (ret, r_pucch)"""
        r = np.zeros(2 * 3 * 12, np.complex64)
        L = lib()
        ret = L.srsran_refsignal_dmrs_pucch_gen_cell(ctypes.byref(self.cell), ctypes.byref(sf), ctypes.byref(cfg),
                                                     r.ctypes.data)
        if ret == 0:
            ret = L.srsran_refsignal_dmrs_pucch_put_cell(ctypes.byref(self.cell), ctypes.byref(cfg), r.ctypes.data,
                                                         grid.ctypes.data)
        return ret, r


def estimate(chest, sf, cfg, grid):
    """srsran_chest_ul_estimate_pucch with a pusch.ChestUl object (its srsran_chest_ul_res_t is written)."""
    g = np.ascontiguousarray(grid, dtype=np.complex64)
    return lib().srsran_chest_ul_estimate_pucch(ctypes.byref(chest.q), ctypes.byref(sf), ctypes.byref(cfg),
                                                g.ctypes.data, ctypes.byref(chest.res))
