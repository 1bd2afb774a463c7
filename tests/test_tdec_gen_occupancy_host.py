"""Resources of the generic turbo decoder (the NSB = 1 kernels of csrc/tdec_kernel.hip, K <= 400), no GPU.

The class runs a dependent chain a wave, so what it decodes a second follows the waves a CU holds.  The floor
asserted here is six workgroups a CU at K = 400: at most 163,840 / 6 = 27,306 B of LDS a workgroup and at most
168 VGPRs without scratch (three waves a SIMD).  The kernels are built for eight (20,480 B, 128 VGPRs, four waves
a SIMD); tools/tdec_occupancy.py reports where they stand.

* the registers come from the compiler's resource remarks of tdec_kernel.hip for gfx950;
* the LDS comes from csrc/tdec_gen_geo.h, the header the launch sizes the workgroup from, through
  tools/tdec_gen_geo_check.cpp built under the address and undefined-behaviour sanitizers.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "srsran_4g_amd", "csrc")

GENERIC = {"tdec_kernel<1, false>": "_ZN10srsran_amd11tdec_kernelILi1ELb0EEEvNS_8TdecArgsE",
           "tdec_kernel<1, true>": "_ZN10srsran_amd11tdec_kernelILi1ELb1EEEvNS_8TdecArgsE",
           "tdec_multi_kernel<1>": "_ZN10srsran_amd17tdec_multi_kernelILi1EEEvPKNS_8TdecArgsEPKji"}
MIN_WG_PER_CU = 6
MAX_LDS = 163840 // MIN_WG_PER_CU  # 27,306 B
MAX_VGPRS = 168                    # three waves a SIMD of 512 registers a lane


def find_hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    hipcc = find_hipcc()
    assert hipcc, "hipcc not found"
    obj = str(tmp_path_factory.mktemp("tdec_gen") / "tdec_kernel.o")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "tdec_kernel.hip"),
                        "-o", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", ln)
        if m:
            cur = out[m.group(1)] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def geo(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("tdec_gen_geo") / "tdec_gen_geo_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "tdec_gen_geo_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    rows = {}
    for ln in r.stdout.splitlines():
        f = {k: int(v) for k, v in (x.split("=") for x in ln.split())}
        rows[f["K"]] = f
    return rows


@pytest.mark.parametrize("name", sorted(GENERIC))
def test_generic_kernel_registers(remarks, name):
    res = remarks[GENERIC[name]]
    print(name, res)
    assert res["VGPRs"] <= MAX_VGPRS, res
    assert res["ScratchSize"] == 0 and res["VGPRs Spill"] == 0, res
    assert res["Occupancy"] >= 3, res


def test_generic_lds_at_k400(geo):
    assert sorted(geo) == list(range(40, 401, 8))
    g = geo[400]
    print(g)
    assert g["lds"] <= MAX_LDS, g
    assert g["wg_per_cu"] >= MIN_WG_PER_CU, g
    # the parts: one int16 a slot for 16 blocks, a checkpoint a 16-step window over K + 3 positions and lane,
    # a decision bit a position, two CRC partials a block
    assert g["s"] == 16 * 400 * 2 and g["M"] == 26 and g["ck"] == 26 * 64 * 4
    assert g["lds"] == g["s"] + g["ck"] + g["bits"] + 16 * 2 * 4
    assert g["state"] == 400
    assert all(geo[k]["lds"] <= g["lds"] for k in geo)
