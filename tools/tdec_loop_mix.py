#!/usr/bin/env python3
"""Instruction mix of the window loops of the single-lane turbo decoders (csrc/tdecs_kernel.hip).

Compiles the four builds (tdec16s, tdec8s, tdec16sw8, tdec8sw8) to gfx950 assembly in a temporary directory
with the Makefile's flags, finds the innermost loops of every kernel and prints, for each loop that carries a
window of trellis steps, one iteration's instructions by class.  The classes go by mnemonic prefix only:

  trellis   v_pk_add_i16 / v_pk_sub_i16 / v_pk_max_i16 / v_perm_b32
  buf_load  buffer_load_*
  lds       ds_*
  waitcnt   s_waitcnt*
  copies    v_mov_b32 / v_accvgpr_*
  scalar    every other s_*
  valu      every other v_*
  other     the rest (global / flat memory, ...)

The counts are static: both arms of a conditional inside a loop are included.  A loop iteration holds as many
windows as it issues sets of 2 W buffer loads (DEC2 runs its windows in pairs); the counts are per window.  A window
loop is a loop with at least 8 trellis instructions per window position; it is a phase-2 loop (recomputation + step
+ LLR) from 30 a position, else a phase-1 loop.  Needs no GPU.

  python tools/tdec_loop_mix.py                      # table
  python tools/tdec_loop_mix.py --json out.json      # and the same as JSON
  python tools/tdec_loop_mix.py --resources          # also registers / spills / scratch per kernel
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "srsran_4g_amd", "csrc")
BUILDS = {  # product -> (defines, window)
    "tdec16s": (["-DTDECS_NSB=16"], 16),
    "tdec8s": (["-DTDECS_NSB=8"], 16),
    "tdec16sw8": (["-DTDECS_NSB=16", "-DTDECS_W=8"], 8),
    "tdec8sw8": (["-DTDECS_NSB=8", "-DTDECS_W=8"], 8),
}
CLASSES = ["trellis", "buf_load", "lds", "waitcnt", "copies", "scalar", "valu", "other"]
TRELLIS = ("v_pk_add_i16", "v_pk_sub_i16", "v_pk_max_i16", "v_perm_b32")


def makefile_var(name):
    with open(os.path.join(CSRC, "Makefile")) as f:
        for line in f:
            m = re.match(r"%s\s*[:?]?=\s*(.*)" % name, line)
            if m:
                return m.group(1).strip()
    raise SystemExit("tdec_loop_mix: no %s in the Makefile" % name)


def classify(mn):
    if mn.startswith(TRELLIS):
        return "trellis"
    if mn.startswith("buffer_load"):
        return "buf_load"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith("s_waitcnt"):
        return "waitcnt"
    if mn.startswith("v_mov_b32") or mn.startswith("v_accvgpr_"):
        return "copies"
    if mn.startswith("s_"):
        return "scalar"
    if mn.startswith("v_"):
        return "valu"
    return "other"


def demangled_kernel(sym):
    m = re.search(r"\d+(tdec\d+s(?:w8)?_(?:multi_)?kernel)(ILb([01])E)?", sym)
    if not m:
        return sym
    return m.group(1) + ("<%s>" % ("true" if m.group(3) == "1" else "false") if m.group(2) else "")


def kernels_of(asm):
    """{kernel symbol: [lines]} of an assembly file."""
    out, cur, name = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                cur = None
            else:
                cur.append(line)
    return out


def loops_of(lines):
    """Innermost loops of a kernel: (label, [mnemonics]) for every back-edge with no back-edge inside it."""
    labels, insts = {}, []
    for line in lines:
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        m = re.match(r"^\s+([a-z]\w*)\s*(.*)", line)
        if m and not line.lstrip().startswith((".", ";")):
            insts.append((m.group(1), m.group(2)))
    spans = []
    for i, (mn, ops) in enumerate(insts):
        if mn.startswith("s_cbranch") or mn == "s_branch":
            tgt = ops.split()[0] if ops else ""
            if tgt in labels and labels[tgt] <= i:
                spans.append((labels[tgt], i, tgt))
    inner = [s for s in spans if not any(o is not s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    return [(lab, [mn for mn, _ in insts[a:b + 1]]) for a, b, lab in inner]


def mix(mns):
    c = dict.fromkeys(CLASSES, 0)
    for mn in mns:
        c[classify(mn)] += 1
    c["total"] = len(mns)
    return c


def compile_build(product, tmp, resources):
    defs, _ = BUILDS[product]
    hipcc = os.environ.get("HIPCC", makefile_var("HIPCC"))
    flags = makefile_var("CXXFLAGS").replace("$(ARCH)", os.environ.get("ARCH", makefile_var("ARCH"))).split()
    out = os.path.join(tmp, product + ".s")
    cmd = [hipcc] + flags + defs + ["--offload-device-only", "-S", os.path.join(CSRC, "tdecs_kernel.hip"), "-o", out]
    if resources:
        cmd.append("-Rpass-analysis=kernel-resource-usage")
    r = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit("tdec_loop_mix: %s did not compile" % product)
    res = {}
    if resources:
        name = None
        for line in r.stderr.splitlines():
            m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
            if not m:
                continue
            k, _, v = m.group(1).partition(": ")
            k = k.strip()
            if k == "Function Name":
                name = demangled_kernel(v)
                res[name] = {}
            elif name and k in ("VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]",
                                "Occupancy [waves/SIMD]"):
                res[name][k] = int(v)
    with open(out) as f:
        return f.read(), res


def analyse(resources=False):
    result = {}
    with tempfile.TemporaryDirectory(prefix="tdec_loop_mix_") as tmp:
        for product, (_, w) in BUILDS.items():
            asm, res = compile_build(product, tmp, resources)
            ks = {}
            for sym, lines in kernels_of(asm).items():
                name = demangled_kernel(sym)
                loops = []
                for lab, mns in loops_of(lines):
                    c = mix(mns)
                    nwin = max(1, round(c["buf_load"] / (2 * w)))
                    if c["trellis"] < 8 * w * nwin:
                        continue
                    c = {k: v / nwin if v % nwin else v // nwin for k, v in c.items()}
                    c["windows"] = nwin
                    c["phase"] = 2 if c["trellis"] >= 30 * w else 1
                    c["label"] = lab
                    loops.append(c)
                ks[name] = {"window": w, "loops": loops}
                if name in res:
                    ks[name]["resources"] = res[name]
            result[product] = ks
    return result


def summary(result):
    """Per kernel and phase the largest loop (the steady-state figure the budget is set on)."""
    s = {}
    for product, ks in result.items():
        for name, k in ks.items():
            for ph in (1, 2):
                ls = [lp["total"] for lp in k["loops"] if lp["phase"] == ph]
                if ls:
                    s["%s phase %d" % (name, ph)] = {"max": max(ls), "min": min(ls), "loops": len(ls)}
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--json", help="write the result to this file as well")
    ap.add_argument("--label", default="tree", help="key of this result in the JSON file (merged into an existing file)")
    ap.add_argument("--resources", action="store_true", help="also report registers, spills and scratch per kernel")
    ap.add_argument("--brief", action="store_true", help="print the per-kernel summary only")
    a = ap.parse_args()
    result = analyse(a.resources)
    hdr = "%-28s %-10s %2s %3s %6s " % ("kernel", "loop", "ph", "win", "total") + " ".join("%8s" % c for c in CLASSES)
    if a.brief:
        for k, v in summary(result).items():
            print("%-36s %d loops, %g .. %g instructions a window" % (k, v["loops"], v["min"], v["max"]))
    else:
        print(hdr)
    for product, ks in result.items() if not a.brief else ():
        for name, k in ks.items():
            for lp in k["loops"]:
                print("%-28s %-10s %2d %3d %6g " % (name, lp["label"], lp["phase"], lp["windows"], lp["total"])
                      + " ".join("%8g" % lp[c] for c in CLASSES))
            if "resources" in k:
                print("%-28s %s" % (name, ", ".join("%s %d" % kv for kv in k["resources"].items())))
    if a.json:
        doc = {}
        if os.path.exists(a.json):
            with open(a.json) as f:
                doc = json.load(f)
        doc[a.label] = {"kernels": result, "summary": summary(result)}
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
