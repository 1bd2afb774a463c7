"""Shared by the PUCCH GPU tests: one estimator / PUCCH object per cell, the direct and one-entry calls on a case of
tests/golden/pucch_golden.npz, and the eNB sequence of enb_ul.c:156-273 composed from the host-synchronous calls."""
import ctypes

import numpy as np
import torch

import pucch_cases as C
from srsran_4g_amd import pucch as P
from srsran_4g_amd import pusch as PU
from srsran_4g_amd.ue_dl import cell as make_cell


class Rig:
    """srsran_chest_ul_t + srsran_pucch_t of every cell the cases use"""

    def __init__(self):
        self.cells = {}

    def get(self, s):
        key = (s["nof_prb"], s["cell_id"], s["cp"])
        if key not in self.cells:
            cell = make_cell(s["nof_prb"], 1, s["cell_id"], cp=s["cp"])
            chest = PU.ChestUl(cell, PU.srsran_refsignal_dmrs_pusch_cfg_t(), max_prb=s["nof_prb"])
            self.cells[key] = (cell, chest, P.Pucch(cell))
        return self.cells[key]

    def free(self):
        for _, chest, pucch in self.cells.values():
            pucch.free()
            chest.free()
        self.cells = {}


def device_grid(grid):
    """complex64 host grid -> (tensor kept alive by the caller, device pointer)"""
    t = torch.from_numpy(np.ascontiguousarray(grid, dtype=np.complex64).view(np.float32).copy()).cuda()
    return t, t.data_ptr()


def get_cfg(spec):
    """the configuration as the eNB holds it before srsran_enb_ul_get_pucch"""
    return C.build_cfg(C.full({k: v for k, v in spec.items() if k not in ("fmt", "n_pucch")}))


def direct_cfg(G, i):
    """the configuration of the direct estimate + decode of case i (true format / resource)"""
    cfg = C.build_cfg(C.full(G.cases[i]))
    after = G.z[f"d_cfg_{i}"]
    cfg.uci_cfg.is_scheduling_request_tti = bool(after[4])
    cfg.uci_cfg.cqi.data_enable = bool(after[5])
    return cfg


def get_one(rig, spec, grid):
    """one-entry srsran_pucch_gpu_get_batch: (ret, res, cfg after)"""
    s = C.full(spec)
    _, chest, pucch = rig.get(s)
    cfg, sf = get_cfg(spec), C.build_sf(s)
    t, dptr = device_grid(grid)
    ret, res = pucch.get_batch([(chest.q, sf, cfg, dptr)])
    torch.cuda.synchronize()
    del t
    return ret, res[0], cfg


def get_host_sync(rig, spec, grid):
    """enb_ul.c:156-273 with srsran_chest_ul_estimate_pucch + srsran_pucch_decode per candidate: (res, cfg after)"""
    s = C.full(spec)
    cell, chest, pucch = rig.get(s)
    cfg, sf = get_cfg(spec), C.build_sf(s)
    L = P.lib()
    assert L.srsran_pucch_cfg_isvalid(ctypes.byref(cfg), s["nof_prb"])

    def one_pass():
        total_ack = sum(a[0] for a in s["acks"])
        if not cfg.simul_cqi_ack and total_ack > 0 and cfg.uci_cfg.cqi.data_enable:
            cfg.uci_cfg.cqi.data_enable = False
        cfg.format = L.srsran_pucch_proc_select_format(ctypes.byref(cell), ctypes.byref(cfg), ctypes.byref(cfg.uci_cfg), None)
        npi = (ctypes.c_uint32 * 4)()
        n = L.srsran_pucch_proc_get_resources(ctypes.byref(cell), ctypes.byref(cfg), ctypes.byref(cfg.uci_cfg), None, npi)
        assert 1 <= n <= 4
        best = P.srsran_pucch_res_t()
        for i in range(n):
            r = P.srsran_pucch_res_t()
            cfg.n_pucch = npi[i]
            assert P.estimate(chest, sf, cfg, grid) == 0
            r.snr_db, r.rssi_dbFs, r.ni_dbFs = chest.res.snr_db, chest.res.epre_dBfs, chest.res.noise_estimate_dbFs
            ret, r = pucch.decode(sf, cfg, chest.res, grid, r)
            assert ret == 0
            if total_ack > 0 and cfg.format == P.FORMAT_1B and cfg.ack_nack_feedback_mode == P.MODE_CS and \
                    not cfg.uci_cfg.is_scheduling_request_tti and r.uci_data.ack.valid:
                b = (ctypes.c_uint8 * 2)(r.uci_data.ack.ack_value[0], r.uci_data.ack.ack_value[1])
                L.srsran_pucch_cs_get_ack(ctypes.byref(cfg), ctypes.byref(cfg.uci_cfg), i, b, ctypes.byref(r.uci_data))
            if i == 0 or r.correlation > best.correlation:
                if cfg.meas_ta_en:
                    r.ta_valid = bool(np.isfinite(chest.res.ta_us))
                    r.ta_us = chest.res.ta_us
                best = r
        return best

    res = one_pass()
    if cfg.uci_cfg.is_scheduling_request_tti and s["acks"]:
        cfg.uci_cfg.is_scheduling_request_tti = False
        no_sr = one_pass()
        if no_sr.detected and (not res.detected or no_sr.correlation > res.correlation):
            res = no_sr
        else:
            cfg.uci_cfg.is_scheduling_request_tti = True
    return res, cfg


def same(a, b):
    """bit-identical structures"""
    return bytes(a) == bytes(b)
