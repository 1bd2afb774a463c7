"""Python mirror of the PRACH C API (include/srsran_prach.h): the FDD occasion helpers, srsran_prach_set_cfg /
gen / detect / detect_offset (prach.c:553-1012) and the added batch, device-output and metrics entry points.
No CPU fallback."""
import ctypes

import numpy as np

from .tdec import load_library
from .ue_dl import srsran_tdd_config_t

u32 = ctypes.c_uint32
_f = ctypes.c_float
_b = ctypes.c_bool
N_ZC = 839
MAX_DET = 128
SRSRAN_SUCCESS, SRSRAN_ERROR, SRSRAN_ERROR_INVALID_INPUTS = 0, -1, -2


class srsran_prach_t(ctypes.Structure):
    _fields_ = [("is_nr", _b), ("config_idx", u32), ("f", u32), ("rsi", u32), ("hs", _b), ("zczc", u32),
                ("N_ifft_ul", u32), ("N_ifft_prach", u32), ("max_N_ifft_ul", u32), ("N_zc", u32), ("N_cs", u32),
                ("N_seq", u32), ("T_seq", _f), ("T_tot", _f), ("N_cp", u32), ("seqs", (_f * (2 * N_ZC)) * 64),
                ("root_seqs_idx", u32 * 64), ("N_roots", u32), ("detect_factor", _f), ("deadzone", u32),
                ("num_ra_preambles", u32), ("successive_cancellation", _b), ("freq_domain_offset_calc", _b),
                ("tdd_config", srsran_tdd_config_t), ("current_prach_idx", u32), ("gpu", ctypes.c_void_p)]


class srsran_prach_sf_config_t(ctypes.Structure):
    _fields_ = [("nof_sf", ctypes.c_int), ("sf", u32 * 5)]


class srsran_prach_cfg_t(ctypes.Structure):
    _fields_ = [("is_nr", _b), ("config_idx", u32), ("root_seq_idx", u32), ("zero_corr_zone", u32),
                ("freq_offset", u32), ("num_ra_preambles", u32), ("hs_flag", _b), ("tdd_config", srsran_tdd_config_t),
                ("enable_successive_cancellation", _b), ("enable_freq_domain_offset_calc", _b)]


class srsran_prach_gpu_occ_t(ctypes.Structure):
    _fields_ = [("prach", ctypes.POINTER(srsran_prach_t)), ("freq_offset", u32), ("d_signal", ctypes.c_void_p),
                ("sig_len", u32)]


class srsran_prach_gpu_res_t(ctypes.Structure):
    _fields_ = [("nof_det", u32), ("indices", u32 * MAX_DET), ("t_offsets", _f * MAX_DET),
                ("peak_to_avg", _f * MAX_DET)]


_bound = False


def lib():
    global _bound
    L = load_library()
    if not _bound:
        P = ctypes.POINTER(srsran_prach_t)
        P32 = ctypes.POINTER(u32)
        PF = ctypes.POINTER(_f)
        vp = ctypes.c_void_p
        sig = {
            "srsran_prach_get_preamble_format": ([u32], u32),
            "srsran_prach_get_sfn": ([u32], ctypes.c_int),
            "srsran_prach_tti_opportunity": ([P, u32, ctypes.c_int], _b),
            "srsran_prach_tti_opportunity_config_fdd": ([u32, u32, ctypes.c_int], _b),
            "srsran_prach_in_window_config_fdd": ([u32, u32, ctypes.c_int], _b),
            "srsran_prach_sf_config": ([u32, ctypes.POINTER(srsran_prach_sf_config_t)], None),
            "srsran_prach_init": ([P, u32], ctypes.c_int),
            "srsran_prach_set_cfg": ([P, ctypes.POINTER(srsran_prach_cfg_t), u32], ctypes.c_int),
            "srsran_prach_gen": ([P, u32, u32, vp], ctypes.c_int),
            "srsran_prach_detect": ([P, u32, vp, u32, P32, P32], ctypes.c_int),
            "srsran_prach_detect_offset": ([P, u32, vp, u32, P32, PF, PF, P32], ctypes.c_int),
            "srsran_prach_set_detect_factor": ([P, _f], None),
            "srsran_prach_free": ([P], ctypes.c_int),
            "srsran_prach_gpu_detect_batch": ([u32, ctypes.POINTER(srsran_prach_gpu_occ_t),
                                               ctypes.POINTER(srsran_prach_gpu_res_t)], ctypes.c_int),
            "srsran_prach_gpu_gen": ([P, u32, u32, vp], ctypes.c_int),
            "srsran_prach_gpu_get_metrics": ([P, PF, P32, P32, P32], ctypes.c_int),
            "srsran_prach_gpu_detect_time": ([P, _b, PF], ctypes.c_int),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _bound = True
    return L


def cfg(config_idx=0, root_seq_idx=0, zero_corr_zone=1, num_ra_preambles=0, is_nr=False, hs_flag=False,
        cancellation=False, freq_domain_offset=False, tdd=False):
    c = srsran_prach_cfg_t()
    c.is_nr = is_nr
    c.config_idx = config_idx
    c.root_seq_idx = root_seq_idx
    c.zero_corr_zone = zero_corr_zone
    c.num_ra_preambles = num_ra_preambles
    c.hs_flag = hs_flag
    c.enable_successive_cancellation = cancellation
    c.enable_freq_domain_offset_calc = freq_domain_offset
    c.tdd_config.configured = tdd
    return c


def sf_config(config_idx):
    s = srsran_prach_sf_config_t()
    lib().srsran_prach_sf_config(config_idx, ctypes.byref(s))
    return s.nof_sf, list(s.sf)


def _res_tuple(r):
    n = r.nof_det
    return (np.array(r.indices[:n], dtype=np.uint32), np.array(r.t_offsets[:n], dtype=np.float32),
            np.array(r.peak_to_avg[:n], dtype=np.float32))


def detect_batch(entries):
    """entries: (Prach, freq_offset, device pointer, sig_len).  One launch; returns (ret, results, raw) where
    results[i] is (indices, t_offsets, peak_to_avg), None when the call was refused, and raw the C array."""
    n = len(entries)
    occ = (srsran_prach_gpu_occ_t * max(n, 1))()
    res = (srsran_prach_gpu_res_t * max(n, 1))()
    for i, (p, fo, dptr, sig_len) in enumerate(entries):
        occ[i].prach = ctypes.pointer(p.q)
        occ[i].freq_offset = fo
        occ[i].d_signal = dptr
        occ[i].sig_len = sig_len
    ret = lib().srsran_prach_gpu_detect_batch(n, occ, res)
    return ret, ([_res_tuple(r) for r in res[:n]] if ret == 0 else None), res


class Prach:
    """srsran_prach_t; raises RuntimeError without a HIP device and ValueError for a refused configuration."""

    def __init__(self, max_N_ifft_ul=2048):
        self.q = srsran_prach_t()
        if lib().srsran_prach_init(ctypes.byref(self.q), max_N_ifft_ul) != 0:
            raise RuntimeError("srsran_prach_init failed: no HIP device?")

    def set_cfg(self, c, nof_prb):
        return lib().srsran_prach_set_cfg(ctypes.byref(self.q), ctypes.byref(c), nof_prb)

    def configure(self, c, nof_prb):
        if self.set_cfg(c, nof_prb) != 0:
            raise ValueError("srsran_prach_set_cfg refused the configuration")
        return self

    @property
    def seqs(self):
        return np.ctypeslib.as_array(self.q.seqs).view(np.complex64).reshape(64, N_ZC).copy()

    def set_detect_factor(self, factor):
        lib().srsran_prach_set_detect_factor(ctypes.byref(self.q), factor)

    def gen(self, seq_index, freq_offset):
        out = np.zeros(self.q.N_cp + self.q.N_seq, dtype=np.complex64)
        ret = lib().srsran_prach_gen(ctypes.byref(self.q), seq_index, freq_offset, out.ctypes.data)
        return ret, out

    def gpu_gen(self, seq_index, freq_offset, dptr):
        return lib().srsran_prach_gpu_gen(ctypes.byref(self.q), seq_index, freq_offset, dptr)

    def detect(self, freq_offset, signal):
        x = np.ascontiguousarray(signal, dtype=np.complex64)
        idx = (u32 * MAX_DET)()
        n = u32(0)
        ret = lib().srsran_prach_detect(ctypes.byref(self.q), freq_offset, x.ctypes.data, len(x), idx, ctypes.byref(n))
        return ret, list(idx[:n.value])

    def detect_offset(self, freq_offset, signal):
        """returns (ret, indices, t_offsets, peak_to_avg)"""
        x = np.ascontiguousarray(signal, dtype=np.complex64)
        idx, t, pk, n = (u32 * MAX_DET)(), (_f * MAX_DET)(), (_f * MAX_DET)(), u32(0)
        ret = lib().srsran_prach_detect_offset(ctypes.byref(self.q), freq_offset, x.ctypes.data, len(x), idx, t, pk,
                                               ctypes.byref(n))
        k = n.value
        return (ret, np.array(idx[:k], dtype=np.uint32), np.array(t[:k], dtype=np.float32),
                np.array(pk[:k], dtype=np.float32))

    def metrics(self):
        """(ratio[nof_roots][nof_wins], offset[nof_roots][nof_wins]) of the last detect"""
        r, o, nr, nw = (_f * MAX_DET)(), (u32 * MAX_DET)(), u32(0), u32(0)
        if lib().srsran_prach_gpu_get_metrics(ctypes.byref(self.q), r, o, ctypes.byref(nr), ctypes.byref(nw)) != 0:
            raise RuntimeError("srsran_prach_gpu_get_metrics: no detect yet")
        n = nr.value * nw.value
        return (np.array(r[:n], dtype=np.float32).reshape(nr.value, nw.value),
                np.array(o[:n], dtype=np.uint32).reshape(nr.value, nw.value))

    def detect_time(self, enable):
        """switch the device-event hook; returns the kernels' time (us) of the last timed detect on this object, or -1"""
        us = _f(-1.0)
        if lib().srsran_prach_gpu_detect_time(ctypes.byref(self.q), enable, ctypes.byref(us)) != 0:
            raise RuntimeError("srsran_prach_gpu_detect_time failed")
        return us.value

    def free(self):
        if self.q.gpu:
            lib().srsran_prach_free(ctypes.byref(self.q))
