"""srsran_chest_ul_estimate_srs (chest_ul.c:298-396, 612-647) restated in float64: the yardstick of the estimator's
tests.  tests/test_srs_host.py holds it against every estimator case the reference recorded."""
import numpy as np

import pusch_cases as PC

F32 = np.float32
# chest_ul.c:644 hands chest_ul_estimate a pilot spacing of 1 although the SRS comb has one pilot every second
# subcarrier: ta_us is twice the delay that produced the phase ramp.  The fixture records this; it is kept.
TA_STRIDE = 1


def comb(row, k0, M_sc):
    """srsran_refsignal_srs_get: the M_sc REs of the last symbol's row from k0, every second one"""
    return np.asarray(row)[k0:k0 + 2 * M_sc:2]


def estimate(rx, r, smooth):
    """rx: the M_sc received comb REs, r: the known sequence, smooth: 3 or 0 (smooth_filter_len) -> dict of the ten
    scalars of srsran_chest_ul_res_t, `ce` (the M_sc values written at symbol L(0, cp) from subcarrier 0) and ta_raw"""
    rx = np.asarray(rx, np.complex128)
    pe = rx * np.conj(np.asarray(r, np.complex128))
    o = {"cfo_hz": np.nan}
    f = -np.angle((pe[1:] * np.conj(pe[:-1])).sum()) / (2 * np.pi)
    o["ta_raw"] = f / TA_STRIDE / 15e3 * 1e6
    o["ta_us"] = float(np.sign(o["ta_raw"]) * np.floor(abs(o["ta_raw"]) * 10 + 0.5) / 10)
    if smooth == 3:
        w = float(F32(0.3333))
        flt = [w, float(F32(1) - F32(2) * F32(0.3333)), w]
        ext = np.concatenate([[3 * pe[1] - 2 * pe[0]], pe, [3 * pe[-1] - 2 * pe[-2]]])
        avg = flt[0] * ext[:-2] + flt[1] * ext[1:-1] + flt[2] * ext[2:]
        a = float(F32(7.419 * w * w + 0.1117 * w - 0.005387))
        o["noise_estimate"] = float((np.abs(avg - pe) ** 2).mean() / (a * 0.8))
    else:
        assert smooth == 0
        avg = pe
        o["noise_estimate"] = 0.0
    o["ce"] = avg
    o["epre"] = float((np.abs(rx) ** 2).mean())
    o["rsrp"] = min(abs(rx.mean()) ** 2, o["epre"])
    o["snr"] = o["epre"] / o["noise_estimate"] if o["noise_estimate"] > 0 else np.nan
    o["epre_dBfs"], o["rsrp_dBfs"], o["snr_db"] = PC.db(o["epre"]), PC.db(o["rsrp"]), PC.db(o["snr"])
    o["noise_estimate_dbFs"] = PC.db(o["noise_estimate"]) + 30
    return o
