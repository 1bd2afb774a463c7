"""Python mirror of the PBCH / MIB decoder C API (include/srsran_pbch.h): srsran_pbch_decode on host grids, the
batch on device buffers, srsran_ue_mib_* on samples and MIB unpacking.  No CPU fallback: decoding needs the HIP device."""
import ctypes

import numpy as np

from .pdcch import _ch
from .ue_dl import (lib as _ue_dl_lib, srsran_cell_t, srsran_chest_dl_res_t, srsran_chest_dl_t, srsran_ofdm_t)

u32 = ctypes.c_uint32
ERROR_INVALID_INPUTS = -2
BCH_PAYLOAD_LEN = 24
NOF_HYP = 90  # port counts 1 / 2 / 4 x 30 (nb, dst, src)
RES_DTYPE = np.dtype([("found", np.uint32), ("nof_tx_ports", np.uint32), ("sfn_offset", np.int32),
                      ("payload", np.uint8, (BCH_PAYLOAD_LEN,))])  # srsran_pbch_gpu_res_t
HYP_DTYPE = np.dtype([("ok", np.uint32), ("bits", np.uint8, (BCH_PAYLOAD_LEN,))])


class srsran_pbch_t(ctypes.Structure):
    _fields_ = [("cell", srsran_cell_t), ("nof_symbols", u32), ("frame_idx", u32), ("search_all_ports", ctypes.c_bool),
                ("gpu", ctypes.c_void_p)]


class srsran_ue_mib_t(ctypes.Structure):
    _fields_ = [("sf_symbols", ctypes.c_void_p), ("fft", srsran_ofdm_t), ("pbch", srsran_pbch_t),
                ("chest", srsran_chest_dl_t), ("chest_res", srsran_chest_dl_res_t), ("frame_cnt", u32)]


class srsran_pbch_gpu_entry_t(ctypes.Structure):
    _fields_ = [("q", ctypes.POINTER(srsran_pbch_t)), ("d_grid", ctypes.c_void_p), ("d_ce", ctypes.c_void_p),
                ("ce_row_len", u32), ("nof_rx", u32), ("d_noise", ctypes.c_void_p)]


class srsran_pbch_gpu_res_t(ctypes.Structure):
    _fields_ = [("found", u32), ("nof_tx_ports", u32), ("sfn_offset", ctypes.c_int32),
                ("payload", ctypes.c_uint8 * BCH_PAYLOAD_LEN)]


class srsran_ue_mib_gpu_entry_t(ctypes.Structure):
    _fields_ = [("q", ctypes.POINTER(srsran_ue_mib_t)), ("d_samples", ctypes.c_void_p)]


_bound = False


def lib():
    global _bound
    L = _ue_dl_lib()
    if not _bound:
        Q = ctypes.POINTER(srsran_pbch_t)
        M = ctypes.POINTER(srsran_ue_mib_t)
        P = ctypes.c_void_p
        U8 = ctypes.POINTER(ctypes.c_uint8)
        PU = ctypes.POINTER(u32)
        PI = ctypes.POINTER(ctypes.c_int)
        sig = {
            "srsran_pbch_init": ([Q], ctypes.c_int),
            "srsran_pbch_free": ([Q], None),
            "srsran_pbch_set_cell": ([Q, srsran_cell_t], ctypes.c_int),
            "srsran_pbch_decode_reset": ([Q], None),
            "srsran_pbch_decode": ([Q, ctypes.POINTER(srsran_chest_dl_res_t), P, U8, PU, PI], ctypes.c_int),
            "srsran_pbch_mib_unpack": ([U8, ctypes.POINTER(srsran_cell_t), PU], None),
            "srsran_pbch_exists": ([ctypes.c_int, ctypes.c_int], ctypes.c_bool),
            "srsran_pbch_put": ([P, P, srsran_cell_t], ctypes.c_int),
            "srsran_pbch_get": ([P, P, srsran_cell_t], ctypes.c_int),
            "srsran_pbch_nof_hypotheses": ([u32], u32),
            "srsran_pbch_gpu_decode_batch": ([u32, ctypes.POINTER(srsran_pbch_gpu_entry_t), P, P], ctypes.c_int),
            "srsran_pbch_gpu_last_llr": ([Q, ctypes.POINTER(P), PU, PU], ctypes.c_int),
            "srsran_pbch_gpu_last_hyp": ([Q, ctypes.POINTER(P), PU], ctypes.c_int),
            "srsran_ue_mib_init": ([M, P, u32], ctypes.c_int),
            "srsran_ue_mib_free": ([M], None),
            "srsran_ue_mib_set_cell": ([M, srsran_cell_t], ctypes.c_int),
            "srsran_ue_mib_reset": ([M], None),
            "srsran_ue_mib_decode": ([M, U8, PU, PI], ctypes.c_int),
            "srsran_ue_mib_gpu_decode_batch": ([u32, ctypes.POINTER(srsran_ue_mib_gpu_entry_t), P, P], ctypes.c_int),
            "srsran_ue_mib_gpu_sync": ([M], ctypes.c_int),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _bound = True
    return L


def mib_unpack(bits):
    """srsran_pbch_mib_unpack: 24 bits -> (nof_prb, phich_length, phich_resources, sfn)"""
    b = np.ascontiguousarray(bits, np.uint8)
    assert b.size == BCH_PAYLOAD_LEN
    c = srsran_cell_t()
    sfn = u32()
    lib().srsran_pbch_mib_unpack(b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(c), ctypes.byref(sfn))
    return c.nof_prb, c.phich_length, c.phich_resources, sfn.value


def hyp_list(frame_idx):
    """(nb, dst, src) of the hypotheses srsran_pbch_decode runs per port count with frame_idx stored frames (pbch.c:
    517-519), and the index of each in the fixed table of 30 (frame_idx = 4) the device uses"""
    full = [(nb, dst, src) for nb in range(4) for dst in range(4 - nb) for src in range(4 - nb)]
    return [(i, h) for i, h in enumerate(full) if h[0] < frame_idx and h[2] < frame_idx - h[0]]


def _device_array(ptr, count, dtype):
    """host copy of `count` items at device pointer `ptr`"""
    import torch

    from .sch import _memcpy_d2h

    out = torch.empty(count * np.dtype(dtype).itemsize, dtype=torch.uint8)
    _memcpy_d2h(out, ptr, out.numel())
    return out.numpy().view(dtype).copy()


class Pbch:
    """srsran_pbch_t of one cell (nof_ports = 0: search 1, 2, 4); raises RuntimeError without a HIP device."""

    def __init__(self, cell):
        self.q = srsran_pbch_t()
        L = lib()
        if L.srsran_pbch_init(ctypes.byref(self.q)) != 0:
            raise RuntimeError("srsran_pbch_init failed: no HIP device?")
        if L.srsran_pbch_set_cell(ctypes.byref(self.q), cell) != 0:
            self.free()
            raise ValueError("srsran_pbch_set_cell failed")

    def set_cell(self, cell):
        return lib().srsran_pbch_set_cell(ctypes.byref(self.q), cell)

    def reset(self):
        lib().srsran_pbch_decode_reset(ctypes.byref(self.q))

    def decode(self, grid, ce, noise):
        """srsran_pbch_decode on the host grid of rx antenna 0 (2 nsymb x 12N) and full-grid estimates (ports, 2 nsymb
        x 12N) -> (ret, payload[24], nof_tx_ports, sfn_offset)"""
        ptrs, res, keep = _ch([grid], [[c] for c in ce], noise, len(ce))
        pl = np.zeros(BCH_PAYLOAD_LEN, np.uint8)
        nports, off = u32(0), ctypes.c_int(0)
        r = lib().srsran_pbch_decode(ctypes.byref(self.q), ctypes.byref(res), ptrs,
                                     pl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(nports),
                                     ctypes.byref(off))
        return r, pl, nports.value, off.value

    def entry(self, d_grid, d_ce, ce_row_len, nof_rx, d_noise):
        e = srsran_pbch_gpu_entry_t()
        e.q, e.d_grid, e.d_ce, e.ce_row_len, e.nof_rx, e.d_noise = ctypes.pointer(self.q), d_grid, d_ce, ce_row_len, \
            nof_rx, d_noise
        return e

    def last_llr(self):
        """(history (4, 2 nof_symbols) float32, frame_idx); refreshes q.frame_idx"""
        p, n, fi = ctypes.c_void_p(), u32(), u32()
        if lib().srsran_pbch_gpu_last_llr(ctypes.byref(self.q), ctypes.byref(p), ctypes.byref(n), ctypes.byref(fi)):
            raise RuntimeError("srsran_pbch_gpu_last_llr failed")
        return _device_array(p.value, n.value, np.float32).reshape(4, -1), fi.value

    def last_hyp(self):
        """the last call's hypothesis records, (3, 30) of HYP_DTYPE"""
        p, n = ctypes.c_void_p(), u32()
        if lib().srsran_pbch_gpu_last_hyp(ctypes.byref(self.q), ctypes.byref(p), ctypes.byref(n)):
            raise RuntimeError("srsran_pbch_gpu_last_hyp failed")
        return _device_array(p.value, n.value, HYP_DTYPE).reshape(3, 30)

    def free(self):
        if self.q.gpu:
            lib().srsran_pbch_free(ctypes.byref(self.q))


def decode_batch(entries, d_out, stream=None):
    """srsran_pbch_gpu_decode_batch; entries: Pbch.entry(...) records; d_out: device pointer of len(entries)
    srsran_pbch_gpu_res_t (RES_DTYPE)"""
    arr = (srsran_pbch_gpu_entry_t * max(1, len(entries)))(*entries)
    return lib().srsran_pbch_gpu_decode_batch(len(entries), arr, d_out, stream)


class UeMib:
    """srsran_ue_mib_t on its own host sample buffer; raises RuntimeError without a HIP device."""

    def __init__(self, cell, max_prb=None):
        self.q = srsran_ue_mib_t()
        L = lib()
        max_prb = max_prb or cell.nof_prb
        self.inb = np.zeros(15 * L.srsran_symbol_sz(max_prb), np.complex64)
        if L.srsran_ue_mib_init(ctypes.byref(self.q), self.inb.ctypes.data, max_prb) != 0:
            raise RuntimeError("srsran_ue_mib_init failed: no HIP device?")
        if L.srsran_ue_mib_set_cell(ctypes.byref(self.q), cell) != 0:
            self.free()
            raise ValueError("srsran_ue_mib_set_cell failed")

    def decode(self, samples):
        """srsran_ue_mib_decode on one subframe of samples -> (ret, payload[24], nof_tx_ports, sfn_offset)"""
        x = np.ascontiguousarray(samples, np.complex64)
        assert x.size == self.q.fft.sf_sz
        self.inb[:x.size] = x
        pl = np.zeros(BCH_PAYLOAD_LEN, np.uint8)
        nports, off = u32(0), ctypes.c_int(0)
        r = lib().srsran_ue_mib_decode(ctypes.byref(self.q), pl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                       ctypes.byref(nports), ctypes.byref(off))
        return r, pl, nports.value, off.value

    def reset(self):
        lib().srsran_ue_mib_reset(ctypes.byref(self.q))

    def sync(self):
        """refreshes frame_cnt and pbch.frame_idx after a batch -> (frame_cnt, frame_idx)"""
        if lib().srsran_ue_mib_gpu_sync(ctypes.byref(self.q)):
            raise RuntimeError("srsran_ue_mib_gpu_sync failed")
        return self.q.frame_cnt, self.q.pbch.frame_idx

    def last_llr(self):
        p, n, fi = ctypes.c_void_p(), u32(), u32()
        if lib().srsran_pbch_gpu_last_llr(ctypes.byref(self.q.pbch), ctypes.byref(p), ctypes.byref(n), ctypes.byref(fi)):
            raise RuntimeError("srsran_pbch_gpu_last_llr failed")
        return _device_array(p.value, n.value, np.float32).reshape(4, -1), fi.value

    def free(self):
        if self.q.pbch.gpu:
            lib().srsran_ue_mib_free(ctypes.byref(self.q))


def ue_mib_decode_batch(mibs, d_samples, d_out, stream=None):
    """srsran_ue_mib_gpu_decode_batch; mibs: UeMib objects, d_samples: one device pointer each"""
    arr = (srsran_ue_mib_gpu_entry_t * max(1, len(mibs)))()
    for a, m, s in zip(arr, mibs, d_samples):
        a.q, a.d_samples = ctypes.pointer(m.q), s
    return lib().srsran_ue_mib_gpu_decode_batch(len(mibs), arr, d_out, stream)
