"""PBCH / MIB decoder, host side (CPU only, no kernel launches): the fixture, the RE table of srsran_pbch_cp, MIB
packing and unpacking, the hypothesis count, and the header as C99."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import chest_cases
import pbch_cases as C
from srsran_4g_amd import enb_dl as E
from srsran_4g_amd import pbch as B
from srsran_4g_amd import tdec
from srsran_4g_amd import ue_dl as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", C.FIXTURE)


@pytest.fixture(scope="module")
def golden():
    z = np.load(FIXTURE)
    return z, json.loads(bytes(z["meta"]).decode())


def test_fixture_size_and_measured_copy(golden):
    z, meta = golden
    assert os.path.getsize(FIXTURE) <= chest_cases.MAX_FIXTURE_BYTES
    assert C.MEASURED == meta["measured"]
    assert C.LLR_TOL == max(4 * meta["measured"], 1e-6)
    assert [m["name"] for m in meta["cases"]] == [c["name"] for c in C.CASES]
    for m, c in zip(meta["cases"], C.CASES):
        assert all(m[k] == c[k] for k in c), c["name"]
        assert [k["ret"] for k in m["calls"]] == c["expect"], c["name"]
        assert max(m["dev1"], m["dev2"]) <= meta["measured"]
    assert meta["invalid"] == [B.ERROR_INVALID_INPUTS, B.ERROR_INVALID_INPUTS]


def pbch_re_36211(nof_prb, cell_id, cp):
    """36.211 6.6.4, written out: the PBCH is mapped to k = N_RB N_sc / 2 - 36 + k', k' = 0..71, l = 0..3 of slot 1,
    in increasing order of k, then l, excluding the REs reserved for reference signals of antenna ports 0-3
    irrespective of the actual configuration.  CRS (6.10.1.2): ports 0 / 1 in l = 0 and l = N_symb - 3, ports 2 / 3 in
    l = 1, on k = 6 m + (v + v_shift) mod 6 with v in {0, 3} (+3 for the other port of the pair): together every k
    with k mod 3 = N_ID mod 3.  N_symb - 3 is l = 4 with the normal CP (outside the PBCH) and l = 3 with the extended
    one."""
    nsymb, nsc = (6 if cp else 7), 12 * nof_prb
    crs_symbols = {0, 1, nsymb - 3}
    out = []
    for l in range(4):
        for kp in range(72):
            k = nsc // 2 - 36 + kp
            if l in crs_symbols and k % 3 == cell_id % 3:
                continue
            out.append((nsymb + l) * nsc + k)
    return np.array(out, np.uint32)


def lib_re_table(c):
    """srsran_pbch_get over slot 1 of a grid that holds its own indices"""
    cell = U.cell(c["nof_prb"], c["ports"], c["cell_id"], cp=c["cp"])
    nsymb, nre = (6 if c["cp"] else 7), 12 * c["nof_prb"]
    grid = np.arange(2 * nsymb * nre).astype(np.complex64)
    out = np.zeros(240, np.complex64)
    n = B.lib().srsran_pbch_get(grid[nsymb * nre:].ctypes.data, out.ctypes.data, cell)
    return out[:n].real.astype(np.uint32)


@pytest.mark.parametrize("c", C.CASES, ids=lambda c: c["name"])
def test_re_table(golden, c):
    z, _ = golden
    want = pbch_re_36211(c["nof_prb"], c["cell_id"], c["cp"])
    assert want.size == C.nof_symbols(c)
    assert np.array_equal(z[c["name"] + "/re"], want)  # the reference's srsran_pbch_cp
    assert np.array_equal(lib_re_table(c), want)       # the library's
    assert np.array_equal(np.array(C.re_table(c["nof_prb"], c["cell_id"], c["cp"]), np.uint32), want)


def test_re_table_put_is_get_inverse():
    cell = U.cell(15, 2, 5)  # odd nof_prb: the PBCH starts in the middle of a PRB; id mod 3 = 2
    L = B.lib()
    sym = (np.arange(240) + 1).astype(np.complex64)
    slot = np.zeros(7 * 180, np.complex64)
    assert L.srsran_pbch_put(sym.ctypes.data, slot.ctypes.data, cell) == 240
    assert np.count_nonzero(slot) == 240 and not slot[4 * 180:].any()
    k = np.nonzero(slot[:180])[0]
    assert k.min() == 90 - 36 and k.max() <= 90 + 35 and not (k % 3 == 2).any()
    back = np.zeros(240, np.complex64)
    assert L.srsran_pbch_get(slot.ctypes.data, back.ctypes.data, cell) == 240
    assert np.array_equal(back, sym)


def test_mib_pack_unpack_roundtrip():
    for nof_prb in (6, 15, 25, 50, 75, 100):
        for phich_len in (0, 1):
            for phich_res in range(4):
                cell = U.cell(nof_prb, 1, 0, phich_res=phich_res, phich_len=phich_len)
                for sfn in list(range(0, 1024, 37)) + [1, 2, 3, 1020, 1021, 1022, 1023]:
                    got = B.mib_unpack(E.mib_pack(cell, sfn))
                    assert got == (nof_prb, phich_len, phich_res, sfn & ~3), (nof_prb, phich_len, phich_res, sfn)


def test_zero_mib_is_the_6prb_default():
    """the MIB the decoder must refuse (pbch.c:374-393) is a real one: 6 PRB, normal PHICH, Ng = 1/6, SFN 0..3"""
    for sfn in range(4):
        assert not E.mib_pack(U.cell(6, 1, 0, phich_res=0), sfn).any()
    assert E.mib_pack(U.cell(6, 1, 0, phich_res=0), 4).any()


def test_hypothesis_count():
    L = B.lib()
    assert [L.srsran_pbch_nof_hypotheses(f) for f in range(5)] == [0, 4, 11, 20, 30]
    for f in range(1, 5):  # the reference's loops (pbch.c:517-519)
        want = [(nb, dst, src) for nb in range(f) for dst in range(4 - nb) for src in range(f - nb)]
        assert [h for _, h in B.hyp_list(f)] == want
    assert B.NOF_HYP == 3 * 30


def test_pbch_exists():
    L = B.lib()
    # pbch.c:47-50: slot 1 of the frames whose number is a multiple of 5
    assert L.srsran_pbch_exists(0, 1) is True and L.srsran_pbch_exists(5, 1) is True
    assert L.srsran_pbch_exists(10, 1) is True
    assert L.srsran_pbch_exists(0, 0) is False and L.srsran_pbch_exists(3, 1) is False
    assert L.srsran_pbch_exists(5, 0) is False and L.srsran_pbch_exists(5, 11) is False


def test_struct_layout_and_c99_header():
    src = r'''
#include "srsran_pbch.h"
#include "srsran_enb_dl.h"
#include <stdio.h>
int main(void) {
  srsran_cell_t cell = {25, 2, 1, SRSRAN_CP_NORM, SRSRAN_PHICH_NORM, SRSRAN_PHICH_R_1, SRSRAN_FDD}, back;
  uint8_t mib[SRSRAN_BCH_PAYLOAD_LEN];
  uint32_t sfn = 0;
  printf("%zu %zu %zu %zu %zu\n", sizeof(srsran_pbch_t), sizeof(srsran_ue_mib_t), sizeof(srsran_pbch_gpu_entry_t),
         sizeof(srsran_pbch_gpu_res_t), sizeof(srsran_ue_mib_gpu_entry_t));
  srsran_pbch_mib_pack(&cell, 517, mib);
  srsran_pbch_mib_unpack(mib, &back, &sfn);
  if (back.nof_prb != 25 || back.phich_resources != SRSRAN_PHICH_R_1 || sfn != 516) return 1;
  if (SRSRAN_BCH_PAYLOADCRC_LEN != 40 || SRSRAN_BCH_ENCODED_LEN != 120 || SRSRAN_UE_MIB_NOF_PRB != 6) return 2;
  if (!srsran_pbch_exists(10, 1) || srsran_pbch_nof_hypotheses(4) != 30) return 3;
  if (0) { srsran_pbch_t q; srsran_ue_mib_t m; int off; uint32_t np;
           srsran_pbch_init(&q); srsran_pbch_set_cell(&q, cell); srsran_pbch_decode(&q, 0, 0, mib, &np, &off);
           srsran_pbch_decode_reset(&q); srsran_pbch_gpu_decode_batch(0, 0, 0, 0); srsran_pbch_gpu_last_llr(&q, 0, 0, 0);
           srsran_pbch_free(&q); srsran_ue_mib_init(&m, 0, 6); srsran_ue_mib_set_cell(&m, cell);
           srsran_ue_mib_decode(&m, mib, &np, &off); srsran_ue_mib_reset(&m); srsran_ue_mib_gpu_decode_batch(0, 0, 0, 0);
           srsran_ue_mib_gpu_sync(&m); srsran_ue_mib_free(&m); }
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "caller.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "caller")
        libdir = os.path.dirname(tdec.LIB_PATH)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-L", libdir,
                        "-lsrsran_4g_amd", "-Wl,-rpath," + libdir, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert [int(x) for x in out.split()] == [ctypes.sizeof(t) for t in (
        B.srsran_pbch_t, B.srsran_ue_mib_t, B.srsran_pbch_gpu_entry_t, B.srsran_pbch_gpu_res_t,
        B.srsran_ue_mib_gpu_entry_t)]
    assert B.RES_DTYPE.itemsize == ctypes.sizeof(B.srsran_pbch_gpu_res_t)
    assert B.HYP_DTYPE.itemsize == 28


@pytest.mark.skipif(tdec.gpu_available(), reason="a HIP device is present")
def test_fails_loudly_without_gpu():
    with pytest.raises(RuntimeError):
        B.Pbch(U.cell(6, 1, 0))
    with pytest.raises(RuntimeError):
        B.UeMib(U.cell(6, 0, 0))
