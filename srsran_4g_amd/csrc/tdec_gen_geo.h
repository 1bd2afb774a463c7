// srsran_4g_amd/csrc/tdec_gen_geo.h -- LDS geometry of the generic (K <= 400) quad decoder of
// tdec_kernel.hip: the kernel, its launch and the host-side checks size the workgroup from here.
// Plain C++ (no HIP types), so a stand-alone host program can include it.
#ifndef SRSRAN_AMD_TDEC_GEN_GEO_H
#define SRSRAN_AMD_TDEC_GEN_GEO_H
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TDEC_GEN_HD __host__ __device__
#else
#define TDEC_GEN_HD
#endif

namespace srsran_amd {

static constexpr int TDEC_GEN_W    = 16;   // steps between checkpoints (the recompute window)
static constexpr int TDEC_GEN_CPW  = 16;   // code blocks a workgroup (a quad of lanes each, per wave)
static constexpr int TDEC_GEN_KMAX = 400;  // largest K the AUTO decoder gives to the generic class
static constexpr uint32_t TDEC_LDS_PER_CU = 160 * 1024;  // gfx950

// LDS of one workgroup (dwords): S [16][K int16] | CK [M][64 lanes] | BITS [16][K/8 B] | RED [16][2]
struct TdecGenGeo {
  uint32_t s_dw, ck_dw, bits_dw, total_dw;  // bits_dw: one block's bitmap
};

// int16 slots a block (TdecArgs::xyw) and checkpoints (TdecArgs::M) of size K: beta runs over K + 3 positions
// (the tail steps are part of the backward pass, turbodecoder_gen.c:78-110)
TDEC_GEN_HD inline uint32_t tdec_gen_xyw(uint32_t K) { return K; }
TDEC_GEN_HD inline uint32_t tdec_gen_M(uint32_t K) { return (K + 3 + TDEC_GEN_W - 1) / TDEC_GEN_W; }

TDEC_GEN_HD inline TdecGenGeo tdec_gen_geo(uint32_t K, uint32_t M)
{
  TdecGenGeo g;
  g.s_dw     = TDEC_GEN_CPW * K / 2;  // K is a multiple of 8
  g.ck_dw    = M * 64;
  g.bits_dw  = (K / 8 + 3) / 4;
  g.total_dw = g.s_dw + g.ck_dw + TDEC_GEN_CPW * g.bits_dw + TDEC_GEN_CPW * 2;
  return g;
}

TDEC_GEN_HD inline size_t tdec_gen_lds_bytes(uint32_t K) { return (size_t)tdec_gen_geo(K, tdec_gen_M(K)).total_dw * 4; }

// int16 values a block keeps between srsran_tdec_iteration calls: the S array
TDEC_GEN_HD inline size_t tdec_gen_state_len(uint32_t K) { return tdec_gen_xyw(K); }

}  // namespace srsran_amd
#endif
