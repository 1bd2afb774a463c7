"""Python mirror of the UE uplink transmit C API (include/srsran_ue_ul.h with the transmit additions of
srsran_sch.h / srsran_pusch.h): srsran_ulsch_encode, srsran_pusch_encode, the DMRS put, srsran_ue_ul_encode and the
device batch srsran_ue_ul_gpu_tx_batch, and the host helpers of the sounding reference signal.  No CPU fallback: everything but the UCI coding runs the HIP kernels."""
import ctypes

import numpy as np

from .pucch import srsran_pucch_cfg_t, srsran_uci_cfg_t
from .pusch import (lib as _pusch_lib, srsran_pusch_t, srsran_refsignal_dmrs_pusch_cfg_t, srsran_refsignal_srs_cfg_t,
                    srsran_ul_sf_cfg_t)
from .sch import Sch, _memcpy_d2h, srsran_pusch_cfg_t, srsran_sch_t, srsran_uci_value_t
from .ue_dl import srsran_cell_t, srsran_ofdm_t

u32 = ctypes.c_uint32
_f = ctypes.c_float
_b = ctypes.c_bool
ERROR, ERROR_INVALID_INPUTS = -1, -2
NORMALIZE_AUTO, NORMALIZE_FORCE_AMPLITUDE = 0, 1


class srsran_pusch_data_t(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("uci", srsran_uci_value_t)]


class srsran_pusch_hopping_cfg_t(ctypes.Structure):
    _fields_ = [("hop_mode", ctypes.c_int), ("hopping_offset", u32), ("n_sb", u32), ("n_rb_ho", u32),
                ("current_tx_nb", u32), ("hopping_enabled", _b)]


class srsran_ue_ul_powerctrl_t(ctypes.Structure):
    _fields_ = [("p0_nominal_pusch", _f), ("alpha", _f), ("p0_nominal_pucch", _f), ("delta_f_pucch", _f * 5),
                ("delta_preamble_msg3", _f), ("p0_ue_pusch", _f), ("delta_mcs_based", _b), ("acc_enabled", _b),
                ("p0_ue_pucch", _f), ("p_srs_offset", _f)]


class srsran_ul_cfg_t(ctypes.Structure):
    _fields_ = [("pucch", srsran_pucch_cfg_t), ("pusch", srsran_pusch_cfg_t), ("hopping", srsran_pusch_hopping_cfg_t),
                ("power_ctrl", srsran_ue_ul_powerctrl_t), ("dmrs", srsran_refsignal_dmrs_pusch_cfg_t),
                ("srs", srsran_refsignal_srs_cfg_t)]


class srsran_ue_ul_cfg_t(ctypes.Structure):
    _fields_ = [("ul_cfg", srsran_ul_cfg_t), ("grant_available", _b), ("cc_idx", u32), ("normalize_mode", ctypes.c_int),
                ("force_peak_amplitude", _f), ("cfo_en", _b), ("cfo_tol", _f), ("cfo_value", _f)]


class srsran_ue_ul_t(ctypes.Structure):
    _fields_ = [("cell", srsran_cell_t), ("signals_pregenerated", _b), ("fft", srsran_ofdm_t),
                ("pusch", srsran_pusch_t), ("out_buffer", ctypes.c_void_p), ("gpu", ctypes.c_void_p)]


class srsran_uci_data_t(ctypes.Structure):
    _fields_ = [("cfg", srsran_uci_cfg_t), ("value", srsran_uci_value_t)]


class srsran_ue_ul_gpu_entry_t(ctypes.Structure):
    _fields_ = [("q", ctypes.POINTER(srsran_ue_ul_t)), ("sf", ctypes.POINTER(srsran_ul_sf_cfg_t)),
                ("cfg", ctypes.POINTER(srsran_ue_ul_cfg_t)), ("uci", ctypes.POINTER(srsran_uci_value_t)),
                ("d_data", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_grid", ctypes.c_void_p)]


_bound = False


def lib():
    global _bound
    L = _pusch_lib()
    if not _bound:
        P = ctypes.c_void_p
        Q = ctypes.POINTER(srsran_ue_ul_t)
        PU = ctypes.POINTER(srsran_pusch_t)
        SF = ctypes.POINTER(srsran_ul_sf_cfg_t)
        CFG = ctypes.POINTER(srsran_pusch_cfg_t)
        UCFG = ctypes.POINTER(srsran_ue_ul_cfg_t)
        DATA = ctypes.POINTER(srsran_pusch_data_t)
        SRS = ctypes.POINTER(srsran_refsignal_srs_cfg_t)
        CELL = ctypes.POINTER(srsran_cell_t)
        sig = {
            "srsran_ulsch_encode": ([ctypes.POINTER(srsran_sch_t), CFG, P, ctypes.POINTER(srsran_uci_value_t), P, P],
                                    ctypes.c_int),
            "srsran_pusch_init_ue": ([PU, u32], ctypes.c_int),
            "srsran_pusch_encode": ([PU, SF, CFG, DATA, P], ctypes.c_int),
            "srsran_refsignal_dmrs_pusch_put_cell": ([ctypes.POINTER(srsran_cell_t), CFG, P, P], ctypes.c_int),
            "srsran_ue_ul_init": ([Q, P, u32], ctypes.c_int),
            "srsran_ue_ul_free": ([Q], None),
            "srsran_ue_ul_set_cell": ([Q, srsran_cell_t], ctypes.c_int),
            "srsran_ue_ul_set_cfr": ([Q, P], ctypes.c_int),
            "srsran_ue_ul_pregen_signals": ([Q, UCFG], ctypes.c_int),
            "srsran_ue_ul_encode": ([Q, SF, UCFG, DATA], ctypes.c_int),
            "srsran_ue_ul_gpu_tx_batch": ([u32, ctypes.POINTER(srsran_ue_ul_gpu_entry_t), P], ctypes.c_int),
            "srsran_ue_ul_gpu_last": ([Q, ctypes.POINTER(P), ctypes.POINTER(u32), ctypes.POINTER(P),
                                       ctypes.POINTER(u32), ctypes.POINTER(P), ctypes.POINTER(u32)], ctypes.c_int),
            "srsran_ue_ul_pucch_resource_selection": ([ctypes.POINTER(srsran_cell_t), ctypes.POINTER(srsran_pucch_cfg_t),
                                                       ctypes.POINTER(srsran_uci_cfg_t),
                                                       ctypes.POINTER(srsran_uci_value_t),
                                                       ctypes.POINTER(ctypes.c_uint8)], None),
            "srsran_ue_ul_sr_send_tti": ([ctypes.POINTER(srsran_pucch_cfg_t), u32], ctypes.c_int),
            "srsran_ue_ul_gen_sr": ([UCFG, SF, ctypes.POINTER(srsran_uci_data_t), _b], _b),
            "srsran_refsignal_srs_pucch_shortened_cfg": ([SF, ctypes.POINTER(srsran_refsignal_srs_cfg_t),
                                                          ctypes.POINTER(srsran_pucch_cfg_t)], None),
            "srsran_refsignal_srs_cfg_isvalid": ([SRS, u32], _b),
            "srsran_refsignal_srs_send_cs": ([u32, u32], ctypes.c_int),
            "srsran_refsignal_srs_send_ue": ([u32, u32], ctypes.c_int),
            "srsran_refsignal_srs_rb_start_cs": ([u32, u32], u32),
            "srsran_refsignal_srs_rb_L_cs": ([u32, u32], u32),
            "srsran_refsignal_srs_M_sc_cell": ([CELL, SRS], u32),
            "srsran_refsignal_srs_k0_cell": ([CELL, SRS, u32], u32),
            "srsran_refsignal_srs_pusch_shortened_cfg": ([CELL, SF, SRS, CFG], None),
            "srsran_refsignal_srs_gen_cell": ([CELL, SRS, ctypes.POINTER(srsran_refsignal_dmrs_pusch_cfg_t), u32, P],
                                              ctypes.c_int),
            "srsran_refsignal_srs_put_cell": ([CELL, SRS, u32, P, P], ctypes.c_int),
            "srsran_refsignal_srs_get_cell": ([CELL, SRS, u32, P, P], ctypes.c_int),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _bound = True
    return L


def sf_len_prb(nof_prb):
    """SRSRAN_SF_LEN_PRB"""
    L = lib()
    L.srsran_symbol_sz.argtypes = [u32]
    L.srsran_symbol_sz.restype = ctypes.c_int
    return 15 * L.srsran_symbol_sz(nof_prb)


def ulsch_encode(sch, cfg, data, uci):
    """srsran_ulsch_encode -> (ret, packed g bits, packed q bits); data: uint8 payload or None"""
    nb = cfg.grant.tb.nof_bits
    g = np.zeros(nb // 8 + 16, np.uint8)
    q = np.zeros(nb // 8 + 16, np.uint8)
    d = None if data is None else np.ascontiguousarray(data, dtype=np.uint8)
    ret = lib().srsran_ulsch_encode(ctypes.byref(sch.q), ctypes.byref(cfg), None if d is None else d.ctypes.data,
                                    ctypes.byref(uci), g.ctypes.data, q.ctypes.data)
    return ret, g, q


def make_data(payload, uci):
    """srsran_pusch_data_t of a uint8 payload (kept alive by the caller) and a UCI value"""
    d = srsran_pusch_data_t()
    d.ptr = None if payload is None else payload.ctypes.data
    ctypes.memmove(ctypes.byref(d.uci), ctypes.byref(uci), ctypes.sizeof(srsran_uci_value_t))
    return d


def dmrs_put(cell, cfg, r, grid):
    """srsran_refsignal_dmrs_pusch_put_cell on a host grid (complex64, modified in place)"""
    r = np.ascontiguousarray(r, dtype=np.complex64)
    return lib().srsran_refsignal_dmrs_pusch_put_cell(ctypes.byref(cell), ctypes.byref(cfg), r.ctypes.data,
                                                      grid.ctypes.data)


def srs_cfg_isvalid(srs, nof_prb):
    return bool(lib().srsran_refsignal_srs_cfg_isvalid(ctypes.byref(srs), nof_prb))


def srs_M_sc(cell, srs):
    return lib().srsran_refsignal_srs_M_sc_cell(ctypes.byref(cell), ctypes.byref(srs))


def srs_k0(cell, srs, tti):
    return lib().srsran_refsignal_srs_k0_cell(ctypes.byref(cell), ctypes.byref(srs), tti)


def srs_pusch_shortened(cell, sf, srs, pusch_cfg):
    """srsran_refsignal_srs_pusch_shortened_cfg: writes and returns sf.shortened"""
    lib().srsran_refsignal_srs_pusch_shortened_cfg(ctypes.byref(cell), ctypes.byref(sf), ctypes.byref(srs),
                                                   ctypes.byref(pusch_cfg))
    return bool(sf.shortened)


def srs_gen(cell, srs, dmrs, sf_idx):
    """srsran_refsignal_srs_gen_cell -> (ret, the 2 M_sc values of the subframe's two slots)"""
    r = np.zeros(2 * max(srs_M_sc(cell, srs), 1), np.complex64)
    ret = lib().srsran_refsignal_srs_gen_cell(ctypes.byref(cell), ctypes.byref(srs), ctypes.byref(dmrs), sf_idx,
                                              r.ctypes.data)
    return ret, r


def srs_put(cell, srs, tti, r, grid):
    """srsran_refsignal_srs_put_cell on a host grid (complex64, modified in place)"""
    r = np.ascontiguousarray(r, dtype=np.complex64)
    return lib().srsran_refsignal_srs_put_cell(ctypes.byref(cell), ctypes.byref(srs), tti, r.ctypes.data, grid.ctypes.data)


def srs_get(cell, srs, tti, grid):
    """srsran_refsignal_srs_get_cell -> (ret, the M_sc comb REs of the last symbol)"""
    r = np.zeros(max(srs_M_sc(cell, srs), 1), np.complex64)
    g = np.ascontiguousarray(grid, dtype=np.complex64)
    ret = lib().srsran_refsignal_srs_get_cell(ctypes.byref(cell), ctypes.byref(srs), tti, r.ctypes.data, g.ctypes.data)
    return ret, r


class PuschUe:
    """srsran_pusch_t initialised for the UE side"""

    def __init__(self, cell, max_prb=100):
        self.q = srsran_pusch_t()
        L = lib()
        assert L.srsran_pusch_init_ue(ctypes.byref(self.q), max_prb) == 0
        assert L.srsran_pusch_set_cell(ctypes.byref(self.q), cell) == 0
        assert self.q.is_ue

    def encode(self, sf, cfg, payload, uci, grid):
        """srsran_pusch_encode into the host grid (complex64 array, modified in place)"""
        p = None if payload is None else np.ascontiguousarray(payload, dtype=np.uint8)
        d = make_data(p, uci)
        return lib().srsran_pusch_encode(ctypes.byref(self.q), ctypes.byref(sf), ctypes.byref(cfg), ctypes.byref(d),
                                         grid.ctypes.data)

    def free(self):
        if self.q.gpu:
            lib().srsran_pusch_free(ctypes.byref(self.q))


class UeUl:
    """srsran_ue_ul_t with a host output buffer of one subframe"""

    def __init__(self, cell, max_prb=None):
        L = lib()
        self.cell = cell
        self.q = srsran_ue_ul_t()
        self.out = np.zeros(sf_len_prb(cell.nof_prb if max_prb is None else max_prb), np.complex64)
        if L.srsran_ue_ul_init(ctypes.byref(self.q), self.out.ctypes.data, cell.nof_prb if max_prb is None else max_prb):
            raise RuntimeError("srsran_ue_ul_init failed (no HIP device?)")
        if L.srsran_ue_ul_set_cell(ctypes.byref(self.q), cell):
            raise RuntimeError("srsran_ue_ul_set_cell failed")
        self.sf_len = sf_len_prb(cell.nof_prb)

    def encode(self, sf, cfg, payload, uci):
        """srsran_ue_ul_encode -> (ret, samples of the subframe (a view of the output buffer))"""
        p = None if payload is None else np.ascontiguousarray(payload, dtype=np.uint8)
        d = make_data(p, uci)
        ret = lib().srsran_ue_ul_encode(ctypes.byref(self.q), ctypes.byref(sf), ctypes.byref(cfg), ctypes.byref(d))
        return ret, self.out[:self.sf_len]

    def last(self):
        """srsran_ue_ul_gpu_last as host copies: (packed scrambled bits, modulation symbols, grid)"""
        import torch  # device copies go through torch's HIP runtime

        P = ctypes.c_void_p
        ds, dd, dg, nb, nr, ng = P(), P(), P(), u32(), u32(), u32()
        if lib().srsran_ue_ul_gpu_last(ctypes.byref(self.q), ctypes.byref(ds), ctypes.byref(nb), ctypes.byref(dd),
                                       ctypes.byref(nr), ctypes.byref(dg), ctypes.byref(ng)):
            raise RuntimeError("srsran_ue_ul_gpu_last: no encode to read")
        # after a PUCCH or an SRS-only subframe nof_bits = nof_re = 0: the grid alone
        s = torch.empty(nb.value // 8, dtype=torch.uint8)
        d = torch.empty(2 * nr.value, dtype=torch.float32)
        g = torch.empty(2 * ng.value, dtype=torch.float32)
        if nb.value:
            _memcpy_d2h(s, ds.value, nb.value // 8)
        if nr.value:
            _memcpy_d2h(d, dd.value, 8 * nr.value)
        _memcpy_d2h(g, dg.value, 8 * ng.value)
        return s.numpy(), d.numpy().view(np.complex64), g.numpy().view(np.complex64)

    def free(self):
        if self.q.gpu:
            lib().srsran_ue_ul_free(ctypes.byref(self.q))


def tx_batch(entries, stream=None):
    """srsran_ue_ul_gpu_tx_batch; entries: (UeUl, sf, cfg, uci or None, d_data ptr, d_out ptr, d_grid ptr)"""
    arr = (srsran_ue_ul_gpu_entry_t * len(entries))()
    for e, (ue, sf, cfg, uci, d_data, d_out, d_grid) in zip(arr, entries):
        e.q = ctypes.pointer(ue.q)
        e.sf = ctypes.pointer(sf)
        e.cfg = ctypes.pointer(cfg)
        if uci is not None:
            e.uci = ctypes.pointer(uci)
        e.d_data, e.d_out, e.d_grid = d_data, d_out, d_grid
    return lib().srsran_ue_ul_gpu_tx_batch(len(entries), arr, stream)


__all__ = ["Sch", "PuschUe", "UeUl", "tx_batch", "ulsch_encode", "dmrs_put", "srsran_ue_ul_cfg_t", "srs_cfg_isvalid",
           "srs_M_sc", "srs_k0", "srs_pusch_shortened", "srs_gen", "srs_put", "srs_get"]
