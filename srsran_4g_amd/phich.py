"""Python mirror of the PHICH C API (include/srsran_phich.h): the resource arithmetic, srsran_phich_encode /
srsran_phich_decode on host grids, the two batch calls on device buffers and srsran_ue_dl_decode_phich.
No CPU fallback: encode / decode need the HIP device."""
import ctypes

import numpy as np

from .pdcch import _ch, lib as _pdcch_lib, srsran_regs_t
from .ue_dl import srsran_cell_t, srsran_chest_dl_res_t, srsran_dl_sf_cfg_t, srsran_ue_dl_cfg_t, srsran_ue_dl_t

u32 = ctypes.c_uint32
ERROR_INVALID_INPUTS = -2


class srsran_phich_t(ctypes.Structure):
    _fields_ = [("cell", srsran_cell_t), ("nof_rx_antennas", u32), ("regs", ctypes.POINTER(srsran_regs_t)),
                ("gpu", ctypes.c_void_p)]


class srsran_phich_resource_t(ctypes.Structure):
    _fields_ = [("ngroup", u32), ("nseq", u32)]


class srsran_phich_grant_t(ctypes.Structure):
    _fields_ = [("n_prb_lowest", u32), ("n_dmrs", u32), ("I_phich", u32)]


class srsran_phich_res_t(ctypes.Structure):
    _fields_ = [("ack_value", ctypes.c_bool), ("distance", ctypes.c_float)]


class srsran_phich_gpu_item_t(ctypes.Structure):
    _fields_ = [("sf", u32), ("tti", u32), ("n_phich", srsran_phich_resource_t), ("ack", ctypes.c_uint8)]


class srsran_phich_gpu_res_t(ctypes.Structure):
    _fields_ = [("ack_value", u32), ("distance", ctypes.c_float)]


RES_DTYPE = np.dtype([("ack_value", np.uint32), ("distance", np.float32)])  # srsran_phich_gpu_res_t
_bound = False


def lib():
    global _bound
    L = _pdcch_lib()
    if not _bound:
        Q = ctypes.POINTER(srsran_phich_t)
        R = ctypes.POINTER(srsran_regs_t)
        SF = ctypes.POINTER(srsran_dl_sf_cfg_t)
        IT = ctypes.POINTER(srsran_phich_gpu_item_t)
        P = ctypes.c_void_p
        sig = {
            "srsran_phich_init": ([Q, u32], ctypes.c_int),
            "srsran_phich_free": ([Q], None),
            "srsran_phich_set_cell": ([Q, R, srsran_cell_t], ctypes.c_int),
            "srsran_phich_set_regs": ([Q, R], None),
            "srsran_phich_calc": ([Q, ctypes.POINTER(srsran_phich_grant_t), ctypes.POINTER(srsran_phich_resource_t)],
                                  None),
            "srsran_phich_ngroups": ([Q], u32),
            "srsran_phich_nsf": ([Q], u32),
            "srsran_phich_reset": ([Q, P], None),
            "srsran_phich_ack_encode": ([ctypes.c_uint8, ctypes.POINTER(ctypes.c_uint8)], None),
            "srsran_phich_ack_decode": ([ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)],
                                        ctypes.c_uint8),
            "srsran_phich_encode": ([Q, SF, srsran_phich_resource_t, ctypes.c_uint8, P], ctypes.c_int),
            "srsran_phich_decode": ([Q, SF, ctypes.POINTER(srsran_chest_dl_res_t), srsran_phich_resource_t, P,
                                     ctypes.POINTER(srsran_phich_res_t)], ctypes.c_int),
            "srsran_phich_gpu_encode_batch": ([Q, u32, IT, u32, P, P], ctypes.c_int),
            "srsran_phich_gpu_decode_batch": ([Q, u32, IT, u32, P, P, u32, P, u32, P, P], ctypes.c_int),
            "srsran_ue_dl_decode_phich": ([ctypes.POINTER(srsran_ue_dl_t), SF, ctypes.POINTER(srsran_ue_dl_cfg_t),
                                           ctypes.POINTER(srsran_phich_grant_t), ctypes.POINTER(srsran_phich_res_t)],
                                          ctypes.c_int),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _bound = True
    return L


def resource(ngroup, nseq):
    r = srsran_phich_resource_t()
    r.ngroup, r.nseq = ngroup, nseq
    return r


def calc(regs, cell, n_prb_lowest, n_dmrs, I_phich=0):
    """srsran_phich_calc on a pdcch.Regs of `cell` (host only) -> (ngroup, nseq)"""
    q = srsran_phich_t()
    q.cell, q.regs = cell, ctypes.pointer(regs.q)
    g = srsran_phich_grant_t()
    g.n_prb_lowest, g.n_dmrs, g.I_phich = n_prb_lowest, n_dmrs, I_phich
    r = srsran_phich_resource_t()
    lib().srsran_phich_calc(ctypes.byref(q), ctypes.byref(g), ctypes.byref(r))
    return r.ngroup, r.nseq


def make_items(items):
    """(sf, tti, ngroup, nseq[, ack]) tuples -> a srsran_phich_gpu_item_t array the batch calls take as it is (a
    caller that repeats a batch builds it once)"""
    if isinstance(items, ctypes.Array):
        return items
    arr = (srsran_phich_gpu_item_t * max(1, len(items)))()
    for a, it in zip(arr, items):
        a.sf, a.tti, a.n_phich.ngroup, a.n_phich.nseq = it[:4]
        a.ack = it[4] if len(it) > 4 else 0
    return arr


class Phich:
    """srsran_phich_t on a pdcch.Regs of one cell; raises RuntimeError without a HIP device."""

    def __init__(self, cell, regs, nrx=1):
        self.q = srsran_phich_t()
        self.cell, self.regs = cell, regs
        L = lib()
        if L.srsran_phich_init(ctypes.byref(self.q), nrx) != 0:
            raise RuntimeError("srsran_phich_init failed: no HIP device?")
        if L.srsran_phich_set_cell(ctypes.byref(self.q), ctypes.byref(regs.q), cell) != 0:
            self.free()
            raise ValueError("srsran_phich_set_cell failed")

    def ngroups(self):
        return lib().srsran_phich_ngroups(ctypes.byref(self.q))

    def encode(self, tti, ngroup, nseq, ack, grids):
        """srsran_phich_encode: adds into `grids`, a list of nof_ports contiguous complex64 host arrays"""
        sf = srsran_dl_sf_cfg_t()
        sf.tti = tti
        ptrs = (ctypes.c_void_p * 4)(*([g.ctypes.data for g in grids] + [None] * (4 - len(grids))))
        return lib().srsran_phich_encode(ctypes.byref(self.q), ctypes.byref(sf), resource(ngroup, nseq), ack, ptrs)

    def decode(self, tti, ngroup, nseq, grids, ce, noise):
        """srsran_phich_decode on host grids (nrx, rows, 12N) and estimates (ports, nrx, rows, 12N) ->
        (ret, ack_value, distance)"""
        ptrs, res, keep = _ch(grids, ce, noise, self.cell.nof_ports)
        sf = srsran_dl_sf_cfg_t()
        sf.tti = tti
        out = srsran_phich_res_t()
        r = lib().srsran_phich_decode(ctypes.byref(self.q), ctypes.byref(sf), ctypes.byref(res),
                                      resource(ngroup, nseq), ptrs, ctypes.byref(out))
        return r, bool(out.ack_value), float(out.distance)

    def encode_batch(self, items, nof_sf, d_grids, stream=None):
        """items: (sf, tti, ngroup, nseq, ack); d_grids: device pointer, [nof_sf][ports][2 nsymb][12N] complex64"""
        return lib().srsran_phich_gpu_encode_batch(ctypes.byref(self.q), len(items), make_items(items), nof_sf, d_grids,
                                                   stream)

    def decode_batch(self, items, nof_sf, d_grids, d_ce, ce_row_len, d_noise, noise_stride, d_out, stream=None):
        """items: (sf, tti, ngroup, nseq); d_out: device pointer of len(items) srsran_phich_gpu_res_t (RES_DTYPE)"""
        return lib().srsran_phich_gpu_decode_batch(ctypes.byref(self.q), len(items), make_items(items), nof_sf, d_grids,
                                                   d_ce, ce_row_len, d_noise, noise_stride, d_out, stream)

    def free(self):
        if self.q.gpu:
            lib().srsran_phich_free(ctypes.byref(self.q))


def ue_decode_phich(ue_q, sf, cfg, n_prb_lowest, n_dmrs, I_phich=0):
    """srsran_ue_dl_decode_phich on a srsran_ue_dl_t -> (ret, ack_value, distance)"""
    g = srsran_phich_grant_t()
    g.n_prb_lowest, g.n_dmrs, g.I_phich = n_prb_lowest, n_dmrs, I_phich
    out = srsran_phich_res_t()
    r = lib().srsran_ue_dl_decode_phich(ctypes.byref(ue_q), ctypes.byref(sf), ctypes.byref(cfg), ctypes.byref(g),
                                        ctypes.byref(out))
    return r, bool(out.ack_value), float(out.distance)
