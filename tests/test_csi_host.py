"""Host side of the channel-state feedback (no GPU): srsran_cqi_from_snr against the reference's recorded values, and
the new declarations as a C99 caller sees them."""
import json
import os
import subprocess
import tempfile

import numpy as np

from srsran_4g_amd import tdec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def test_cqi_from_snr_matches_reference_record():
    """tests/golden/cqi_from_snr.json (tests/golden/make_csi_golden.py: the reference's cqi.c:740-748 at, one float
    below and one float above each of its 15 thresholds, and at -100 / +100 dB)"""
    from srsran_4g_amd import ue_dl as U
    pairs = json.load(open(os.path.join(ROOT, "tests", "golden", "cqi_from_snr.json")))
    assert len(pairs) == 47 and {p["cqi"] for p in pairs} == set(range(16))
    assert pairs[0]["snr"] == -100.0 and pairs[-1]["snr"] == 100.0
    for p in pairs:
        assert float(np.float32(p["snr"])) == p["snr"]  # recorded as floats
        assert U.cqi_from_snr(p["snr"]) == p["cqi"], p


def test_new_entry_points_compile_and_link_as_c99():
    """a C99 translation unit that includes the headers and takes the address of every new entry point; the record
    is 64 bytes with the fields where the Python mirror has them"""
    src = r'''
#include "srsran_ue_dl.h"
#include "srsran_enb_dl.h"
#include <stddef.h>
#include <stdio.h>
typedef void (*fn_t)(void);
int main(void) {
  fn_t f[] = {(fn_t)srsran_precoding_pmi_select, (fn_t)srsran_precoding_cn, (fn_t)srsran_precoding_csi_2x2,
              (fn_t)srsran_pdsch_select_pmi, (fn_t)srsran_pdsch_compute_cn, (fn_t)srsran_ue_dl_select_ri,
              (fn_t)srsran_ue_dl_select_ri_pmi, (fn_t)srsran_ue_dl_gpu_csi_batch, (fn_t)srsran_ue_dl_gpu_last_ce,
              (fn_t)srsran_cqi_from_snr};
  size_t n = 0;
  for (size_t i = 0; i < sizeof(f) / sizeof(f[0]); i++) {
    n += f[i] != NULL;
  }
  srsran_cell_t cell = {0};
  cell.nof_prb = 100;
  printf("%zu %zu %zu %zu %zu %zu %d %d %u\n", n, sizeof(srsran_csi_gpu_t), offsetof(srsran_csi_gpu_t, sinr_2l),
         offsetof(srsran_csi_gpu_t, cn), offsetof(srsran_csi_gpu_t, pmi_1l), offsetof(srsran_csi_gpu_t, cn_count),
         (int)SRSRAN_NOF_RE(cell), SRSRAN_MAX_CODEBOOKS, (unsigned)srsran_cqi_from_snr(10.0f));
  return 0;
}
'''
    from srsran_4g_amd import ue_dl as U
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "csi.c"), os.path.join(d, "csi")
        open(c, "w").write(src)
        libdir = os.path.dirname(tdec.LIB_PATH)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, c, "-L", libdir, "-lsrsran_4g_amd",
                            "-Wl,-rpath," + libdir, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    T = U.srsran_csi_gpu_t
    assert [int(x) for x in out] == [10, 64, T.sinr_2l.offset, T.cn.offset, T.pmi_1l.offset, T.cn_count.offset, 16800,
                                     4, 5]
    assert (T.sinr_2l.offset, T.cn.offset, T.pmi_1l.offset, T.cn_count.offset) == (16, 24, 32, 52)
    assert U.CSI_DTYPE.itemsize == 64 and [U.CSI_DTYPE.fields[k][1] for k in ("sinr_2l", "cn", "pmi_1l", "cn_count")] == [
        16, 24, 32, 52]
