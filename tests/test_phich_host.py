"""PHICH, host side (no GPU): the PHICH RE table of srsran_regs_t and srsran_phich_calc against the fixture recorded
from the compiled reference (tests/golden/make_phich_golden.py), the ctypes layout of the new structs against the C
compiler's, and a C99 caller of srsran_enb_dl_put_phich / srsran_ue_dl_decode_phich that compiles and links."""
import ctypes
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from srsran_4g_amd import enb_dl, pdcch, phich, tdec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "phich_golden.npz"))
META = json.loads(bytes(GOLD["meta"]).decode())
CASES = META["cases"]


def make_cell(c):
    cl = pdcch.cell(c["nof_prb"], c["ports"], c["cell_id"], c["phich_len"], c["phich_res"], c["cp"])
    cl.frame_type = c["frame"]
    return cl


def make_regs(c):
    return pdcch.Regs(make_cell(c), c["mi"], c["sf1_6"])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_phich_re_table_equals_reference(c):
    regs = make_regs(c)
    try:
        want = GOLD[c["name"] + "/re"]
        units = c["ngroups"] // 2 if c["cp"] else c["ngroups"]
        assert regs.q.ngroups_phich == units == want.shape[0]  # mapping units; the reference's count is c["ngroups"]
        if c["mi"]:  # with m_i = 0 the reference leaves ngroups_phich_m1 unset (regs.c:762); this library keeps it
            assert regs.q.ngroups_phich_m1 == c["ngroups_m1"]
        assert np.array_equal(regs.phich_re(), want)
        # the units' REs are no PCFICH or PDCCH RE of any CFI
        used = set(want.ravel().tolist())
        assert len(used) == want.size
        assert not used & set(regs.pcfich_re().tolist())
        for cfi in (1, 2, 3):
            assert not used & set(regs.pdcch_re(cfi).tolist())
    finally:
        regs.free()


@pytest.mark.parametrize("name", sorted(META["calc"]))
def test_phich_calc_equals_reference(name):
    c = next(x for x in CASES if x["name"] == name)
    regs = make_regs(c)
    try:
        want = GOLD[name + "/calc"]
        got = np.array([[phich.calc(regs, make_cell(c), n, dm, META["calc"][name]) for dm in range(8)]
                        for n in range(c["nof_prb"])], np.uint32)
        assert np.array_equal(got, want)
    finally:
        regs.free()


def test_ack_encode_decode_rule():
    bits = (ctypes.c_uint8 * 3)()
    phich.lib().srsran_phich_ack_encode(1, bits)
    assert list(bits) == [1, 1, 1]
    for llr, ack, dist in (((0.5, 1.0, 0.0), 1, 0.5), ((-0.5, -1.0, 0.0), 0, 0.5), ((0.0, 0.0, 0.0), 0, 0.0)):
        d = ctypes.c_float()
        assert phich.lib().srsran_phich_ack_decode((ctypes.c_float * 3)(*llr), ctypes.byref(d)) == ack
        assert d.value == pytest.approx(dist, abs=1e-7)  # ACK only if strictly larger


NEW_STRUCTS = {
    "srsran_phich_t": phich.srsran_phich_t, "srsran_phich_resource_t": phich.srsran_phich_resource_t,
    "srsran_phich_grant_t": phich.srsran_phich_grant_t, "srsran_phich_res_t": phich.srsran_phich_res_t,
    "srsran_phich_gpu_item_t": phich.srsran_phich_gpu_item_t, "srsran_phich_gpu_res_t": phich.srsran_phich_gpu_res_t,
    "srsran_enb_dl_gpu_phich_t": enb_dl.srsran_enb_dl_gpu_phich_t,
    "srsran_enb_dl_gpu_ctrl_t": enb_dl.srsran_enb_dl_gpu_ctrl_t, "srsran_regs_t": pdcch.srsran_regs_t,
}

CALLER = r'''
static int caller(void)
{
  if (0) { /* linked, not run */
    srsran_enb_dl_t      enb;
    srsran_ue_dl_t       ue;
    srsran_dl_sf_cfg_t   sf;
    srsran_ue_dl_cfg_t   cfg;
    srsran_phich_grant_t grant = {0, 0, 0};
    srsran_phich_res_t   res;
    srsran_enb_dl_put_phich(&enb, &grant, true);
    return srsran_ue_dl_decode_phich(&ue, &sf, &cfg, &grant, &res);
  }
  return 0;
}
'''


def test_new_structs_layout_and_c99_caller_links():
    headers = sorted(h for h in os.listdir(INCLUDE) if h.endswith(".h"))
    assert "srsran_phich.h" in headers
    body = []
    for n, cls in sorted(NEW_STRUCTS.items()):
        body.append(f'  printf("S {n} %zu\\n", sizeof({n}));')
        for f in cls._fields_:
            body.append(f'  printf("F {n} {f[0]} %zu\\n", offsetof({n}, {f[0]}));')
    src = "#define _GNU_SOURCE\n" + "".join(f'#include "{h}"\n' for h in headers) + \
        "#include <stddef.h>\n#include <stdio.h>\n#include <string.h>\n" + CALLER + \
        "int main(void) {\n" + "\n".join(body) + '\n  printf("C %d\\n", caller());\n  return 0;\n}\n'
    libdir = os.path.dirname(tdec.LIB_PATH)
    with tempfile.TemporaryDirectory() as d:
        cfile, exe = os.path.join(d, "phich_abi.c"), os.path.join(d, "phich_abi")
        open(cfile, "w").write(src)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-unused-variable", "-I", INCLUDE, cfile, "-o",
                            exe, "-L", libdir, "-lsrsran_4g_amd", "-Wl,-rpath," + libdir, "-lm"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes, offs = {}, {}
    for ln in out.splitlines():
        p = ln.split()
        if p[0] == "S":
            sizes[p[1]] = int(p[2])
        elif p[0] == "F":
            offs[(p[1], p[2])] = int(p[3])
    bad = []
    for n, cls in NEW_STRUCTS.items():
        if ctypes.sizeof(cls) != sizes[n]:
            bad.append(f"sizeof({n}): C {sizes[n]} ctypes {ctypes.sizeof(cls)}")
        for f in cls._fields_:
            if getattr(cls, f[0]).offset != offs[(n, f[0])]:
                bad.append(f"offsetof({n}, {f[0]}): C {offs[(n, f[0])]} ctypes {getattr(cls, f[0]).offset}")
    assert not bad, bad
    # phich_re is the last member of srsran_regs_t: the reference-ordered part of the struct did not move
    assert pdcch.srsran_regs_t._fields_[-1][0] == "phich_re"
    assert offs[("srsran_regs_t", "phich_re")] + ctypes.sizeof(ctypes.c_void_p) == sizes["srsran_regs_t"]
