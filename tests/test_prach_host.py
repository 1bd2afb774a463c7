"""PRACH host side (no GPU): the FDD occasion helpers against 36.211 Table 5.7.1-2 written out here, the
root-sequence table's structure, and the ctypes mirrors against the C layout."""
import ctypes
import math
import os
import subprocess
import tempfile

import prach_np as R
from srsran_4g_amd import prach as P
from srsran_4g_amd import tdec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 36.211 Table 5.7.1-2, frame structure type 1: PRACH configuration index % 16 -> (system frame number, subframes)
EVEN, ANY = 0, 1
TABLE = {0: (EVEN, [1]), 1: (EVEN, [4]), 2: (EVEN, [7]), 3: (ANY, [1]), 4: (ANY, [4]), 5: (ANY, [7]),
         6: (ANY, [1, 6]), 7: (ANY, [2, 7]), 8: (ANY, [3, 8]), 9: (ANY, [1, 4, 7]), 10: (ANY, [2, 5, 8]),
         11: (ANY, [3, 6, 9]), 12: (ANY, [0, 2, 4, 6, 8]), 13: (ANY, [1, 3, 5, 7, 9]),
         14: (ANY, list(range(10))), 15: (EVEN, [9])}
# Table 5.7.1-1: T_CP + T_SEQ in T_s
T_TOT = {0: 3168 + 24576, 1: 21024 + 24576, 2: 6240 + 2 * 24576, 3: 21024 + 2 * 24576}  # format = config_idx // 16


def want_opportunity(config_idx, tti):
    sfn, sfs = TABLE[config_idx % 16]
    if config_idx == 14:  # the reference special-cases index 14 itself, not 14 mod 16 (prach.c:154)
        return True
    if config_idx % 16 == 14:
        return False  # nof_sf = -1 in the reference's table: no subframe matches
    return (sfn == ANY or (tti // 10) % 2 == 0) and tti % 10 in sfs


def test_format_and_sfn():
    L = P.lib()
    for c in range(64):
        assert L.srsran_prach_get_preamble_format(c) == c // 16
        assert L.srsran_prach_get_sfn(c) == TABLE[c % 16][0]


def test_tti_opportunity_matches_table():
    L = P.lib()
    for c in range(64):
        for tti in range(40):
            assert L.srsran_prach_tti_opportunity_config_fdd(c, tti, -1) == want_opportunity(c, tti), (c, tti)
    # the cases the table is known by
    assert [t for t in range(40) if L.srsran_prach_tti_opportunity_config_fdd(0, t, -1)] == [1, 21]
    assert [t for t in range(40) if L.srsran_prach_tti_opportunity_config_fdd(3, t, -1)] == [1, 11, 21, 31]
    assert [t for t in range(10) if L.srsran_prach_tti_opportunity_config_fdd(12, t, -1)] == [0, 2, 4, 6, 8]
    assert all(L.srsran_prach_tti_opportunity_config_fdd(14, t, -1) for t in range(40))
    assert [t for t in range(40) if L.srsran_prach_tti_opportunity_config_fdd(15, t, -1)] == [9, 29]
    # allowed_subframe restricts to one subframe
    assert L.srsran_prach_tti_opportunity_config_fdd(12, 4, 4)
    assert not L.srsran_prach_tti_opportunity_config_fdd(12, 4, 6)


def test_sf_config():
    for c in range(64):
        n, sf = P.sf_config(c)
        if c % 16 == 14:
            assert n == -1
        else:
            assert n == len(TABLE[c % 16][1]) and sf[:n] == TABLE[c % 16][1]


def test_in_window_spans_the_preamble():
    L = P.lib()
    for c in (0, 3, 6, 12, 15, 16, 19, 28, 32, 35, 47, 51, 63):
        dur = math.ceil(T_TOT[c // 16] / (15000 * 2048) * 1000)
        assert dur == {0: 1, 1: 2, 2: 2, 3: 3}[c // 16]
        for tti in range(10, 50):
            want = any(want_opportunity(c, tti - i) for i in range(dur))
            assert L.srsran_prach_in_window_config_fdd(c, tti, -1) == want, (c, tti)


def test_object_opportunity_is_fdd_only():
    q = P.srsran_prach_t()
    q.config_idx = 3
    L = P.lib()
    assert L.srsran_prach_tti_opportunity(ctypes.byref(q), 11, -1)
    assert not L.srsran_prach_tti_opportunity(ctypes.byref(q), 12, -1)
    q.tdd_config.configured = True
    assert not L.srsran_prach_tti_opportunity(ctypes.byref(q), 11, -1)
    assert not L.srsran_prach_tti_opportunity(None, 11, -1)


def test_root_table_structure():
    roots = R.tables()["kPrachRoots"]
    assert len(roots) == 838 and sorted(roots) == list(range(1, 839))
    assert all(roots[i] + roots[i + 1] == 839 for i in range(0, 838, 2))
    assert roots[:4] == [129, 710, 140, 699]
    # 36.211 Table 5.7.2-4, spot values: the rows of logical numbers 0-23 (its end), 24-29 (its start) and 820-837
    for logical, u in ((20, 2), (21, 837), (22, 1), (23, 838), (24, 56), (25, 783), (836, 229), (837, 610)):
        assert roots[logical] == u, (logical, u)
    assert R.tables()["kPrachNcs"] == [0, 13, 15, 18, 22, 26, 32, 38, 46, 59, 76, 93, 119, 167, 279, 419]
    assert R.tables()["kPrachTcp"] == [3168, 21024, 6240, 21024]
    assert R.tables()["kPrachTseq"] == [24576, 24576, 49152, 49152]


def test_ctypes_mirrors_match_the_header():
    """sizeof / offsetof of the PRACH structs as a C99 compiler lays them out"""
    types = [P.srsran_prach_t, P.srsran_prach_cfg_t, P.srsran_prach_sf_config_t, P.srsran_prach_gpu_occ_t,
             P.srsran_prach_gpu_res_t]
    body = []
    for t in types:
        body.append(f'  printf("{t.__name__} %zu\\n", sizeof({t.__name__}));')
        for f in t._fields_:
            body.append(f'  printf("{t.__name__}.{f[0]} %zu\\n", offsetof({t.__name__}, {f[0]}));')
    src = '#include "srsran_prach.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + \
        "\n".join(body) + "\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(c, "w").write(src)
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), c, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict((ln.split()[0], int(ln.split()[1])) for ln in out.splitlines())
    for t in types:
        assert got[t.__name__] == ctypes.sizeof(t), t.__name__
        for f in t._fields_:
            assert got[f"{t.__name__}.{f[0]}"] == getattr(t, f[0]).offset, (t.__name__, f[0])


def test_symbols_exported():
    L = tdec.load_library()
    for n in ("srsran_prach_init", "srsran_prach_set_cfg", "srsran_prach_gen", "srsran_prach_detect",
              "srsran_prach_detect_offset", "srsran_prach_set_detect_factor", "srsran_prach_free",
              "srsran_prach_gpu_detect_batch", "srsran_prach_gpu_gen", "srsran_prach_gpu_get_metrics",
              "srsran_prach_gpu_detect_time"):
        assert hasattr(L, n), n
