"""Host checks of the NR SCH transmit side (CPU only).

* nr_rm_tx_pos_check.cpp, a stand-alone program, is built with the host compiler under ASan + UBSan and run as a
  child process: the closed forms of csrc/nr_rm_tx_pos.h (k0 / Ncb, non-filler rank -> position, interleaver
  index, E per code block and its prefix offset) against the reference's sequential definitions written out as
  loops, over both base graphs, Z in {2, 7, 20, 384}, rv 0-3, four N_ref, three filler counts, every modulation
  order and E below, at and above one lap of the circular buffer.
* the new structs' sizeof / offsetof as a C99 compiler lays them out against the ctypes mirrors, the new names in
  the library, and a C99 caller of every new entry point compiled with -std=c99 -Wall -Werror.
"""
import ctypes
import os
import subprocess
import tempfile

from srsran_4g_amd import ldpc, sch, sch_nr, tdec

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "srsran_4g_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

NEW_NAMES = ["srsran_ldpc_encoder_init", "srsran_ldpc_encoder_free", "srsran_ldpc_encoder_encode",
             "srsran_ldpc_encoder_encode_rm", "srsran_ldpc_encoder_gpu_encode_batch", "srsran_ldpc_rm_tx_init",
             "srsran_ldpc_rm_tx", "srsran_ldpc_rm_tx_free", "srsran_softbuffer_tx_init",
             "srsran_softbuffer_tx_init_guru", "srsran_softbuffer_tx_free", "srsran_softbuffer_tx_reset",
             "srsran_sch_nr_init_tx", "srsran_dlsch_nr_encode", "srsran_ulsch_nr_encode",
             "srsran_sch_nr_gpu_encode_batch"]

NEW_STRUCTS = {"srsran_ldpc_encoder_t": ldpc.srsran_ldpc_encoder_t, "srsran_ldpc_rm_t": ldpc.srsran_ldpc_rm_t,
               "srsran_softbuffer_tx_t": sch.srsran_softbuffer_tx_t,
               "srsran_sch_nr_gpu_enc_t": sch_nr.srsran_sch_nr_gpu_enc_t, "srsran_sch_tb_t": sch_nr.srsran_sch_tb_t}

CALLER = r'''
/* a gNB / UE transmitter's calls; without a HIP device every *_init refuses, which main() reports */
static int caller(void)
{
  srsran_ldpc_encoder_t  enc;
  srsran_ldpc_rm_t       rm;
  srsran_softbuffer_tx_t sb;
  srsran_sch_nr_t        q;
  srsran_sch_nr_args_t   args;
  srsran_sch_cfg_t       cfg;
  srsran_sch_tb_t        tb;
  srsran_carrier_nr_t    carrier;
  static uint8_t         msg[44], cw[132], data[3], e[48];
  int                    n = 0;
  memset(&args, 0, sizeof(args));
  memset(&cfg, 0, sizeof(cfg));
  memset(&tb, 0, sizeof(tb));
  memset(&carrier, 0, sizeof(carrier));
  if (srsran_softbuffer_tx_init_guru(&sb, SRSRAN_SCH_NR_MAX_NOF_CB_LDPC, SRSRAN_LDPC_MAX_LEN_ENCODED_CB) != SRSRAN_SUCCESS ||
      sb.max_cb != SRSRAN_SCH_NR_MAX_NOF_CB_LDPC || sb.buffer_b == NULL || sb.buffer_b[0] == NULL) {
    return -1;
  }
  srsran_softbuffer_tx_reset(&sb);
  if (srsran_ldpc_encoder_init(&enc, SRSRAN_LDPC_ENCODER_AVX2, BG1, 2) == 0) {
    n += srsran_ldpc_encoder_encode(&enc, msg, cw, enc.liftK) == 0;
    n += srsran_ldpc_encoder_encode_rm(&enc, msg, cw, enc.liftK, 60) == 0;
    n += srsran_ldpc_encoder_gpu_encode_batch(&enc, NULL, 0, 0, 0, NULL, 0, NULL) != 0;
    srsran_ldpc_encoder_free(&enc);
  }
  if (srsran_ldpc_rm_tx_init(&rm) == 0) {
    n += srsran_ldpc_rm_tx(&rm, cw, e, 48, BG1, 2, 0, SRSRAN_MOD_QPSK, 132) == 0;
    srsran_ldpc_rm_tx_free(&rm);
  }
  if (srsran_sch_nr_init_tx(&q, &args) == SRSRAN_SUCCESS) {
    carrier.nof_prb = 25;
    srsran_sch_nr_set_carrier(&q, &carrier);
    tb.mod = SRSRAN_MOD_QPSK; tb.N_L = 1; tb.tbs = 24; tb.R = 0.5; tb.nof_bits = 48;
    tb.softbuffer.tx = &sb;
    n += srsran_dlsch_nr_encode(&q, &cfg, &tb, data, e) == SRSRAN_SUCCESS;
    n += srsran_ulsch_nr_encode(&q, &cfg, &tb, data, e) == SRSRAN_SUCCESS;
    n += srsran_sch_nr_gpu_encode_batch(&q, 0, NULL, NULL) == SRSRAN_SUCCESS;
    srsran_sch_nr_free(&q);
  }
  srsran_softbuffer_tx_free(&sb);
  return n;
}
'''


def test_rm_tx_positions_under_asan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "nr_rm_tx_pos_check")
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-O1", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(HERE, "nr_rm_tx_pos_check.cpp"),
                        "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "nr_rm_tx_pos OK" in r.stdout, r.stdout


def test_new_names_resolve():
    L = tdec.load_library()
    missing = [n for n in NEW_NAMES if not hasattr(L, n)]
    assert not missing, missing


def test_c99_caller_and_struct_layouts():
    body = []
    for n, c in sorted(NEW_STRUCTS.items()):
        body.append(f'  printf("S {n} %zu\\n", sizeof({n}));')
        for f in c._fields_:
            body.append(f'  printf("F {n} {f[0]} %zu\\n", offsetof({n}, {f[0]}));')
    src = '#include "srsran_ldpc.h"\n#include "srsran_sch.h"\n#include "srsran_sch_nr.h"\n' \
          "#include <stddef.h>\n#include <stdio.h>\n#include <string.h>\n" + CALLER + \
          "int main(void) {\n" + "\n".join(body) + '\n  printf("C %d\\n", caller());\n  return 0;\n}\n'
    libdir = os.path.dirname(tdec.LIB_PATH)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "tx_abi.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(d, "tx_abi")
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, c, "-o", exe, "-L", libdir,
                            "-lsrsran_4g_amd", "-Wl,-rpath," + libdir, "-lm"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes, offs, ran = {}, {}, None
    for ln in out.splitlines():
        p = ln.split()
        if p[0] == "S":
            sizes[p[1]] = int(p[2])
        elif p[0] == "F":
            offs[(p[1], p[2])] = int(p[3])
        elif p[0] == "C":
            ran = int(p[1])
    bad = []
    for n, c in NEW_STRUCTS.items():
        if ctypes.sizeof(c) != sizes[n]:
            bad.append(f"sizeof({n}): C {sizes[n]} ctypes {ctypes.sizeof(c)}")
        for f in c._fields_:
            if getattr(c, f[0]).offset != offs[(n, f[0])]:
                bad.append(f"offsetof({n}, {f[0]}): C {offs[(n, f[0])]} ctypes {getattr(c, f[0]).offset}")
    assert not bad, bad
    # without a HIP device every GPU object refuses to initialise (no CPU fallback) and only the capacity-only
    # soft buffer works; with one, all seven calls succeed
    assert ran == (7 if tdec.gpu_available() else 0), out
