#!/usr/bin/env python3
"""Registers, scratch and occupancy of the kernels of the single-lane turbo decoders (csrc/tdecs_kernel.hip).

Compiles the four builds (tdec16s, tdec8s, tdec16sw8, tdec8sw8) for gfx950 with the Makefile's flags and
-Rpass-analysis=kernel-resource-usage, device code only, and reports what the compiler states for every kernel:
VGPRs, AGPRs, scratch bytes a lane, waves a SIMD.  The fused 16-step kernel (tdec16s_multi_kernel) must hold
  VGPRs + AGPRs <= 256,  ScratchSize 0,  occupancy 2
(two waves a SIMD without spills); the exit status says whether it does.  Needs no GPU.

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


def resources(defines):
    hipcc = os.environ.get("HIPCC", makefile_var("HIPCC"))
    flags = makefile_var("CXXFLAGS").replace("$(ARCH)", os.environ.get("ARCH", makefile_var("ARCH"))).split()
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc] + flags + defines + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                           os.path.join(CSRC, "tdecs_kernel.hip"), "-o", os.path.join(tmp, "k.o")]
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
