// srsran_4g_amd/csrc/ctrl_dev.h -- device helpers shared by the convolutionally coded control channels: the PDCCH
// candidates (pdcch_kernel.hip) and the PBCH hypotheses (pbch_kernel.hip).
//
//   cpx / ldc / cmulf / conjf   complex arithmetic in the operation order of the reference's predecoders
//   kPerm / kPermInv, rm_geom,  the tail-biting rate matcher's sub-block interleaver (rm_conv.c:120-175): geometry of
//   cb_rank / cb_pos            a code of clen bits, rank of a soft-buffer position among the non-dummy positions of
//                               the circular buffer and its inverse
//   rm_conv_rx_gather           srsran_rm_conv_rx for one 64-lane workgroup: every output gathers its inputs in
//                               increasing input order, SRSRAN_RX_NULL inputs skipped (no atomics)
//   vit_quantise                srsran_viterbi_decode_f's float -> uint16 conversion in the AVX2 16-bit build
//                               (viterbi.c:546-585): gain 500 / max|x|, one fused multiply-add, truncation
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srsran_amd {

static constexpr float CTRL_RX_NULL = 10000.0f;  // SRSRAN_RX_NULL
static constexpr int   CTRL_NCOLS   = 32;
static __constant__ uint8_t kPerm[CTRL_NCOLS] = {1, 17, 9, 25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31,
                                                 0, 16, 8, 24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};
static __constant__ uint8_t kPermInv[CTRL_NCOLS] = {16, 0, 24, 8, 20, 4, 28, 12, 18, 2, 26, 10, 22, 6, 30, 14,
                                                    17, 1, 25, 9, 21, 5, 29, 13, 19, 3, 27, 11, 23, 7, 31, 15};

struct cpx {
  float r, i;
};
__device__ __forceinline__ cpx ldc(const float2* p, uint32_t k)
{
  const float2 v = p[k];
  return {v.x, v.y};
}
__device__ __forceinline__ cpx cmulf(cpx a, cpx b)
{
#pragma clang fp contract(off)
  return {a.r * b.r - a.i * b.i, a.i * b.r + a.r * b.i};
}
__device__ __forceinline__ cpx conjf(cpx a) { return {a.r, -a.i}; }

struct RmGeom {
  int nrows, Kp, nd, nv;  // interleaver rows, padded stream length, dummies per stream, non-dummy positions
};
__device__ __forceinline__ RmGeom rm_geom(uint32_t clen)
{
  RmGeom g;
  g.nrows = (int)((clen / 3 - 1) / CTRL_NCOLS + 1);
  g.Kp    = g.nrows * CTRL_NCOLS;
  g.nd    = max(0, g.Kp - (int)(clen / 3));
  g.nv    = 3 * (g.Kp - g.nd);
  return g;
}

// Rank of soft-buffer position p (stream s, column col, row r) among the non-dummy positions of
// the circular buffer (rm_conv.c bit collection order); -1 for a dummy position.  Only row 0 of a
// column whose permuted index is below ndummy (< 32) is a dummy.
__device__ __forceinline__ int cb_rank(int p, int nrows, int Kp, int ndummy, const uint8_t* dcols_before)
{
  const int s = p / Kp, q = p - s * Kp, col = q / nrows, r = q - col * nrows;
  const bool dcol = kPerm[col] < ndummy;
  if (r == 0 && dcol) {
    return -1;
  }
  return s * (Kp - ndummy) + col * nrows - dcols_before[col] + r - (dcol ? 1 : 0);
}

// Soft-buffer position of rank k (inverse of cb_rank).
__device__ __forceinline__ int cb_pos(int k, int nrows, int Kp, int ndummy)
{
  const int nv = Kp - ndummy, s = k / nv;
  int       r  = k - s * nv;
  for (int col = 0; col < CTRL_NCOLS; col++) {
    const int cnt = nrows - (kPerm[col] < ndummy ? 1 : 0);
    if (r < cnt) {
      return s * Kp + col * nrows + r + (kPerm[col] < ndummy ? 1 : 0);
    }
    r -= cnt;
  }
  return -1;
}

// srsran_rm_conv_rx (rm_conv.c:120-175) from E inputs e(0 .. E - 1) to clen outputs in rm (LDS); an output none of
// whose inputs is set becomes 0.  dcb: 32 bytes of LDS.  All 64 lanes call it (it synchronises).
template <typename Load>
__device__ __forceinline__ void rm_conv_rx_gather(uint32_t clen, uint32_t E, Load e, float* rm, uint8_t* dcb, int lane)
{
#pragma clang fp contract(off)
  const RmGeom g = rm_geom(clen);
  if (lane == 0) {
    int acc = 0;
    for (int col = 0; col < CTRL_NCOLS; col++) {
      dcb[col] = (uint8_t)acc;
      acc += kPerm[col] < g.nd ? 1 : 0;
    }
  }
  __syncthreads();
  for (uint32_t oi = lane; oi < clen; oi += 64) {
    const int i = (int)(oi / 3), j = (int)(oi - 3 * (oi / 3));
    const int di = (i + g.nd) / CTRL_NCOLS, dj = (i + g.nd) % CTRL_NCOLS;
    const int p  = g.Kp * j + kPermInv[dj] * g.nrows + di;
    const int rk = cb_rank(p, g.nrows, g.Kp, g.nd, dcb);
    float     t  = CTRL_RX_NULL;
    if (rk >= 0) {
      for (int k = rk; k < (int)E; k += g.nv) {
        const float v = e(k);
        if (t == CTRL_RX_NULL) {
          t = v;
        } else if (v != CTRL_RX_NULL) {
          t = t + v;
        }
      }
    }
    rm[oi] = t != CTRL_RX_NULL ? t : 0.0f;
  }
  __syncthreads();
}

// rm: clen floats in LDS -> sym: clen quantised soft bits.  All 64 lanes call it (it synchronises).
__device__ __forceinline__ void vit_quantise(const float* rm, uint32_t clen, uint16_t* sym, int lane)
{
  float mx = 0.0f;
  for (uint32_t i = lane; i < clen; i += 64) {
    mx = fmaxf(mx, fabsf(rm[i]));
  }
  for (int off = 32; off > 0; off >>= 1) {
    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  }
  const float mxv  = (mx > 0.0f && __builtin_isnormal(mx)) ? mx : 1e-9f;
  const float gain = __fdiv_rn(500.0f, mxv);
  for (uint32_t i = lane; i < clen; i += 64) {
    int v  = __float2int_rz(__builtin_fmaf(gain, rm[i], 32767.5f));
    sym[i] = (uint16_t)min(max(v, 0), 65535);
  }
  __syncthreads();
}

}  // namespace srsran_amd
