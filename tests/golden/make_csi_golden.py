"""Generate tests/golden/cqi_from_snr.json from the reference's own srsran_cqi_from_snr (phch/cqi.c:740-748).

Run where the reference tree exists (REF as in oracle/Makefile, the directory that holds include/ and src/):
    python tests/golden/make_csi_golden.py [REF]
cqi.c is compiled into a shared object in a temporary directory, which is removed afterwards; only the recorded
(snr, cqi) pairs are kept.  The SNRs sit at, one float below and one float above each of the 15 thresholds of the
reference's table, and at -100 and +100 dB; every cqi is the reference's return value.
"""
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# the thresholds are where the recorded function changes its value: found by bisection on the reference itself
LO, HI = -100.0, 100.0


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF")
    if not ref:  # oracle/Makefile's default
        mk = open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "Makefile")).read()
        ref = re.search(r"^REF\s*\?=\s*(\S+)", mk, flags=re.M).group(1)
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libcqi.so")
        # cqi.c includes srsran/srsran.h, which wants the version header a configured build generates: an empty one
        os.makedirs(os.path.join(d, "srsran"))
        open(os.path.join(d, "srsran", "version.h"), "w").write("/* stand-in for the generated header */\n")
        subprocess.run(["gcc", "-std=c99", "-D_GNU_SOURCE", "-O2", "-fPIC", "-shared", "-I", d,
                        "-I", os.path.join(ref, "include"),
                        os.path.join(ref, "src", "phy", "phch", "cqi.c"), "-o", so, "-lm"], check=True)
        L = ctypes.CDLL(so, mode=os.RTLD_LAZY)
        L.srsran_cqi_from_snr.argtypes = [ctypes.c_float]
        L.srsran_cqi_from_snr.restype = ctypes.c_uint8
        f = lambda x: int(L.srsran_cqi_from_snr(float(x)))  # noqa: E731
        assert f(LO) == 0 and f(HI) == 15
        snrs = [np.float32(LO), np.float32(HI)]
        for cqi in range(1, 16):  # the smallest float whose value is >= cqi
            lo, hi = np.float32(LO), np.float32(HI)
            while np.nextafter(lo, np.float32(np.inf)) < hi:
                mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
                if f(mid) >= cqi:
                    hi = mid
                else:
                    lo = mid
            snrs += [lo, hi, np.nextafter(hi, np.float32(np.inf))]
        pairs = [{"snr": float(s), "cqi": f(s)} for s in sorted(set(snrs))]
    with open(os.path.join(HERE, "cqi_from_snr.json"), "w") as out:
        json.dump(pairs, out, indent=0)
        out.write("\n")
    print(f"{len(pairs)} pairs")


if __name__ == "__main__":
    main()
