"""The launch plan of srsran_tdec_gpu_run_multi (csrc/tdec_plan.h: tdec_multi_plan), no GPU: tools/tdec_plan_check.cpp,
built from the planner's header alone under the address and undefined-behaviour sanitizers, prints the launches of
seven cases; here they are compared with what the decoder has issued for those shapes since the class launches were
cut by residency and gated.  The residency stub is that section's: three workgroups a CU for
K >= 4864, four below.

Two cases follow the code that the plan was taken from where the request for this test read it differently: with the
mid cut at 0 (G) the sizes above the 8-step cut are still cut by residency, so they are two launches, and with every
single-lane threshold at 0 on the natural layout (E) the generic class, which has no other layout, runs its
single-lane build."""
import os
import shutil
import subprocess

import pytest

from oracle import CB_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

S12 = (40, 400, 408, 800, 816, 1536, 1568, 2048, 2112, 4800, 4864, 6144)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("tdec_plan") / "tdec_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "tdec_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "case":
            cur = out[w[1]] = {"launches": [], "large_done": None, "reserved": None}
        elif w[0] == "large_done":
            cur["large_done"] = len(cur["launches"])
        elif w[0] == "reserved":
            cur["reserved"] = int(w[1])
        else:
            assert w[0] == "launch", ln
            f = dict(x.split("=") for x in w[2:])
            cur["launches"].append({
                "build": w[1], "fused": f["fused"] == "1", "scratch": f["scratch"] == "1", "slot": int(f["slot"]),
                "stream": int(f["stream"]), "gated": f["gated"] == "1", "wg": int(f["wg"]),
                "K": [int(k) for k in f["K"].split(",")],
                "ck": [tuple(int(v) for v in p.split("+")) for p in f["ck"].split(",") if p]})
    assert list(out) == list("ABCDEFG")
    return out


def rows(case):
    """(build, scratch, sizes, stream, gated) of every launch"""
    return [(x["build"], x["scratch"], x["K"], x["stream"], x["gated"]) for x in case["launches"]]


SMALL = [("tdecs16w8", False, [1536, 816], 1, True),
         ("tdecs8w8", False, [800, 408], 2, True),
         ("quad<1>", False, [400, 40], 3, True)]


def test_a_every_entry(cases):
    a = cases["A"]
    assert rows(a) == [("tdecs16", True, [6144, 4864], 0, False),
                       ("tdecs16", True, [4800, 2112], 0, False),
                       ("tdecs16", True, [2048, 1568], 0, False)] + SMALL
    assert a["large_done"] == 2
    assert all(x["fused"] for x in a["launches"]) and [x["slot"] for x in a["launches"]] == [0, 1, 2, 3, 4, 5]


def test_b_defaults_on_few_blocks(cases):
    b = cases["B"]
    assert rows(b) == [("quad<16>", False, [6144, 4864, 4800, 2112, 2048, 1568, 1536, 816], 0, False),
                       ("quad<8>", False, [800, 408], 2, False),
                       ("quad<1>", False, [400, 40], 3, False)]
    assert all(x["fused"] for x in b["launches"]) and b["reserved"] == 0


def test_c_the_benchmark_shape(cases):
    c = cases["C"]
    got = [(x["build"], x["scratch"], len(x["K"]), min(x["K"]), max(x["K"])) for x in c["launches"]]
    assert got == [("tdecs16", True, 21, 4864, 6144),
                   ("tdecs16", True, 43, 2112, 4800),
                   ("tdecs16", True, 16, 1568, 2048),
                   ("tdecs16w8", False, 30, 816, 1536),
                   ("tdecs8w8", False, 32, 408, 800),
                   ("quad<1>", False, 46, 40, 400)]
    assert [x["gated"] for x in c["launches"]] == [False, False, False, True, True, True]
    assert [x["stream"] for x in c["launches"]] == [0, 0, 0, 1, 2, 3]
    assert [x["slot"] for x in c["launches"]] == [0, 1, 2, 3, 4, 5] and all(x["fused"] for x in c["launches"])
    assert c["large_done"] == 2
    assert [x["wg"] for x in c["launches"][:2]] == [5376, 11008]
    assert sorted(k for x in c["launches"] for k in x["K"]) == sorted(CB_SIZES)
    assert all(x["K"] == sorted(x["K"], reverse=True) for x in c["launches"])  # longest first


def test_d_one_size_a_class(cases):
    d = cases["D"]
    assert rows(d) == [("tdecs16", False, [6144], 0, False), ("quad<1>", False, [40], 3, False)]
    assert not any(x["fused"] for x in d["launches"]) and d["reserved"] == 0


def test_e_natural_layout(cases):
    e = cases["E"]
    assert rows(e) == [("quad<16>", False, [6144, 4864, 4800, 2112, 2048, 1568, 1536, 816], 0, False),
                       ("quad<8>", False, [800, 408], 2, False),
                       ("tdecs1", False, [400, 40], 3, False)]


def test_f_failed_residency_query(cases):
    f = cases["F"]
    assert rows(f) == [("tdecs16", True, [6144, 4864, 4800, 2112], 0, False),
                       ("tdecs16", True, [2048, 1568], 0, False)] + SMALL
    assert [x["slot"] for x in f["launches"]] == [0, 2, 3, 4, 5] and f["large_done"] == 1


def test_g_no_mid_cut(cases):
    g = cases["G"]
    assert rows(g) == [("tdecs16", True, [6144, 4864], 0, False),
                       ("tdecs16", True, [4800, 2112, 2048, 1568], 0, False)] + [r[:4] + (False,) for r in SMALL]
    assert g["large_done"] == 2


@pytest.mark.parametrize("name", ["A", "C", "G"])
def test_scratch_parts_are_disjoint_and_fill_the_reservation(cases, name):
    case = cases[name]
    parts = [p for x in case["launches"] for p in x["ck"]]
    assert len(parts) == sum(len(x["K"]) for x in case["launches"] if x["scratch"]) > 0
    assert all(not x["ck"] for x in case["launches"] if not x["scratch"])
    end = 0
    for off, size in sorted(parts):
        assert off >= end and size > 0, (off, end)
        end = off + size
    assert sum(size for _, size in parts) == end == case["reserved"]
    # every workgroup's region: [ceil(L / 16) windows][64 lanes][16 B], four blocks a workgroup (tdecs_ck_geo.h)
    want = [(-(-(k // 16) // 16)) * 1024 * -(-n // 4) for x in case["launches"] if x["scratch"]
            for k, n in zip(x["K"], [1024 if name == "C" else 5] * len(x["K"]))]
    assert [size for _, size in parts] == want
