#!/usr/bin/env python3
"""Registers, scratch and occupancy of the kernels of the single-lane turbo decoders (csrc/tdecs_kernel.hip).

Compiles the four builds (tdec16s, tdec8s, tdec16sw8, tdec8sw8) for gfx950 with the Makefile's flags and
-Rpass-analysis=kernel-resource-usage, device code only, and reports what the compiler states for every kernel:
VGPRs, AGPRs, scratch bytes a lane, waves a SIMD.  The fused 16-step kernel (tdec16s_multi_kernel) must hold
  VGPRs + AGPRs <= 256,  ScratchSize 0,  occupancy 2
(two waves a SIMD without spills); the exit status says whether it does.  Needs no GPU.

The generic class (K <= 400) runs the quad decoder's three NSB = 1 kernels (csrc/tdec_kernel.hip), whose rate
follows the workgroups a CU holds: their rows add the LDS of the K = 400 workgroup (csrc/tdec_gen_geo.h through
tools/tdec_gen_geo_check.cpp) and the workgroups a CU that LDS and the registers allow.  They must hold at least
six (<= 27,306 B, <= 168 VGPRs, no scratch) and are built for eight.

  python tools/tdec_occupancy.py                      # table
  python tools/tdec_occupancy.py --json out.json      # and the same as JSON, merged into out.json's "compiled" key
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tdec_loop_mix import BUILDS, CSRC, demangled_kernel, makefile_var  # noqa: E402

FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
          "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "static_lds_bytes"}


GENERIC = {"_ZN10srsran_amd11tdec_kernelILi1ELb0EEEvNS_8TdecArgsE": "tdec_kernel<1, false>",
           "_ZN10srsran_amd11tdec_kernelILi1ELb1EEEvNS_8TdecArgsE": "tdec_kernel<1, true>",
           "_ZN10srsran_amd17tdec_multi_kernelILi1EEEvPKNS_8TdecArgsEPKji": "tdec_multi_kernel<1>"}


def generic_lds_k400():
    """LDS bytes of the generic decoder's K = 400 workgroup, from the header the launch uses"""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "geo")
        subprocess.run(["g++", "-std=c++17", os.path.join(os.path.dirname(CSRC), "..", "tools", "tdec_gen_geo_check.cpp"),
                        "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    row = [ln for ln in out.splitlines() if ln.startswith("K=400 ")][0]
    return int(dict(x.split("=") for x in row.split())["lds"])


def resources(defines, src="tdecs_kernel.hip"):
    hipcc = os.environ.get("HIPCC", makefile_var("HIPCC"))
    flags = makefile_var("CXXFLAGS").replace("$(ARCH)", os.environ.get("ARCH", makefile_var("ARCH"))).split()
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc] + flags + defines + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                           os.path.join(CSRC, src), "-o", os.path.join(tmp, "k.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(r.stderr)
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(demangled_kernel(m.group(1)), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z][^:]*): (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    a = ap.parse_args()
    res = {}
    for build, (defines, _) in BUILDS.items():
        res.update(resources(defines))
    print("%-28s %6s %6s %8s %6s" % ("kernel", "VGPRs", "AGPRs", "scratch", "waves"))
    for k, v in res.items():
        print("%-28s %6d %6d %8d %6d" % (k, v["vgprs"], v["agprs"], v["scratch_bytes_per_lane"], v["waves_per_simd"]))
    f = res["tdec16s_multi_kernel"]
    ok = f["vgprs"] + f["agprs"] <= 256 and f["scratch_bytes_per_lane"] == 0 and f["waves_per_simd"] == 2
    print("tdec16s_multi_kernel: two waves a SIMD without spills: %s" % ("yes" if ok else "NO"))
    lds = generic_lds_k400()
    gen = {name: v for sym, v in resources([], "tdec_kernel.hip").items() for name in [GENERIC.get(sym)] if name}
    print("%-28s %6s %8s %6s %10s %8s" % ("generic kernel", "VGPRs", "scratch", "waves", "LDS K=400", "WG a CU"))
    for k, v in gen.items():
        v["lds_bytes_k400"] = lds
        v["wg_per_cu"] = min(163840 // lds, 2 * v["waves_per_simd"])  # two waves a workgroup, four SIMDs a CU
        print("%-28s %6d %8d %6d %10d %8d" % (k, v["vgprs"], v["scratch_bytes_per_lane"], v["waves_per_simd"], lds,
                                              v["wg_per_cu"]))
    gen_ok = len(gen) == 3 and all(v["wg_per_cu"] >= 6 and v["scratch_bytes_per_lane"] == 0 for v in gen.values())
    print("generic kernels: six workgroups a CU without spills: %s" % ("yes" if gen_ok else "NO"))
    res.update(gen)
    ok = ok and gen_ok
    if a.json:
        doc = {}
        if os.path.exists(a.json):
            with open(a.json) as fh:
                doc = json.load(fh)
        doc["compiled"] = {"how": "tools/tdec_occupancy.py: hipcc -Rpass-analysis=kernel-resource-usage, gfx950, the Makefile's flags",
                           "kernels": res, "fused_16_step_two_waves_without_spills": ok}
        with open(a.json, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
