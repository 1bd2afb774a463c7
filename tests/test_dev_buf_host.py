"""Host check of csrc/dev_buf.h (CPU only): dev_buf_check.cpp defines counting hipMalloc / hipFree /
hipHostMalloc / hipHostFree over malloc / free, is built with the host compiler under ASan + UBSan with no
HIP runtime linked, and runs as a child process.  It asserts reserve / floor / failure / move semantics and
that nothing is live at exit."""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "srsran_4g_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_dev_buf_semantics_under_asan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "dev_buf_check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", CSRC,
                        "-isystem", os.path.join(ROCM, "include"), os.path.join(HERE, "dev_buf_check.cpp"),
                        "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "dev_buf OK" in r.stdout and "0 live" in r.stdout, r.stdout
