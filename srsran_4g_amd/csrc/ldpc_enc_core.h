// srsran_4g_amd/csrc/ldpc_enc_core.h -- NR LDPC encoder of one code block in LDS (device code, gfx950).
//
// Arithmetic of ldpc_enc_c.c:38-230 on packed bits.  A chunk is the Z bits of one base-graph column,
// bit i in word i / 32 at bit i % 32.  The bgK message chunks and the four core parity chunks are kept
// DOUBLED: the Z bits twice back to back, so the chunk rotated by s -- bit i = chunk[(i + s) mod Z] --
// is a plain unaligned 32-bit field read at bit offset s + 32 w (two dwords and a funnel shift), for any
// Z, with a mask on the last word only.  A work item is (row m, word w):
//   rows 0..3   aux[m] = XOR over the row's message edges of the rotated chunk (preprocess_systematic_bits)
//   core        the four high-rate solutions (encode_high_rate_case1..4) on aux[0..3], word-wise
//   rows >= 4   aux[m] XOR the rotated core parity chunks (encode_ext_region): every edge of the row
//               left of the identity part, in one pass
// Base-graph topology is compile time (ldpc_bg_tables.inc); the shifts V mod Z come from the caller's
// table in edge order.  Both users -- the plain encoder (ldpc_enc_kernel.hip) and the NR SCH transmit
// kernel (nr_sch_tx_kernel.hip) -- fill LdpcEncLds::msg, call ldpc_enc_core and read the code block
// back through ldpc_enc_bit.
#ifndef SRSRAN_AMD_LDPC_ENC_CORE_H
#define SRSRAN_AMD_LDPC_ENC_CORE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldpc_enc_kernel.h"
#include "ldpc_kernel.h"

// row starts and columns are indexed by a per-lane row: device-resident constant tables
#define LDPC_TBL static __constant__ const
#include "ldpc_bg_tables.inc"

namespace srsran_amd {

constexpr int LDPC_ENC_MAXW = 12;                     // words per chunk at Z = 384
constexpr int LDPC_ENC_MAXD = 2 * LDPC_ENC_MAXW + 1;  // words per doubled chunk (+1: the funnel's high dword)

struct LdpcEncLds {
  uint32_t sh[LDPC_MAX_EDGES];                       // V mod Z per edge
  uint32_t msg[8448 / 32 + 2];                       // the liftK message bits, fillers as 0 (+ funnel pad)
  uint32_t dbl[(22 + 4) * LDPC_ENC_MAXD];            // doubled chunks: message 0 .. bgK - 1, core parity bgK .. bgK + 3
  uint32_t ext[42 * LDPC_ENC_MAXW];                  // parity chunks of rows >= 4, packed
  uint32_t aux[5 * LDPC_ENC_MAXW + 2];               // aux[0..3], then the packed core parity (+ what the funnel reads behind it)
  uint32_t sum[LDPC_ENC_MAXD];                       // aux[0] ^ aux[1] ^ aux[2] ^ aux[3], doubled
};

template <int BG>
struct LdpcEncTopo;
template <>
struct LdpcEncTopo<0> {
  static constexpr int M = 46, K = 22, NE = LDPC_BG1_NEDGES;
  static __device__ __forceinline__ int rs(int m) { return LDPC_BG1_ROW_START[m]; }
  static __device__ __forceinline__ int col(int e) { return LDPC_BG1_COL[e]; }
};
template <>
struct LdpcEncTopo<1> {
  static constexpr int M = 42, K = 10, NE = LDPC_BG2_NEDGES;
  static __device__ __forceinline__ int rs(int m) { return LDPC_BG2_ROW_START[m]; }
  static __device__ __forceinline__ int col(int e) { return LDPC_BG2_COL[e]; }
};

// 32 bits of a packed bit array from bit offset `off` (the array has one pad word behind its last bit)
__device__ __forceinline__ uint32_t ldpc_enc_get32(const uint32_t* a, uint32_t off)
{
  const uint32_t w = off >> 5;
  return (uint32_t)((((uint64_t)a[w + 1] << 32) | a[w]) >> (off & 31u));
}

__device__ __forceinline__ uint32_t ldpc_enc_lowmask(int n) { return n >= 32 ? 0xFFFFFFFFu : (1u << n) - 1u; }

// word j of the doubled form of the Z bits that start at bit `base` of `src`
__device__ __forceinline__ uint32_t ldpc_enc_dbl_word(const uint32_t* src, uint32_t base, int Z, int j)
{
  const int p0 = 32 * j;
  uint32_t  v  = 0;
  if (p0 < Z) {
    v = ldpc_enc_get32(src, base + p0) & ldpc_enc_lowmask(Z - p0);
    if (Z - p0 < 32) {
      v |= ldpc_enc_get32(src, base) << (Z - p0);
    }
  } else {
    v = ldpc_enc_get32(src, base + p0 - Z);
  }
  return v;
}

// Encodes the message in s.msg (bits >= liftK zero, filler bits zero); s.sh holds the shifts.  The caller
// has synchronised after writing both.  n_rows = base-graph rows computed (4 .. M).  On return (synchronised)
// s.dbl holds the doubled message and core parity chunks and s.ext the parity of rows 4 .. n_rows - 1.
template <int BG>
__device__ __forceinline__ void ldpc_enc_core(LdpcEncLds& s, int Z, int hr_case, int n_rows)
{
  using T       = LdpcEncTopo<BG>;
  const int W   = (Z + 31) >> 5;
  const int SD  = 2 * W + 1;
  const int tid = threadIdx.x, nt = blockDim.x;
  const uint32_t last = ldpc_enc_lowmask(Z - 32 * (W - 1));

  for (int it = tid; it < T::K * SD; it += nt) {
    const int k = it / SD, j = it - k * SD;
    s.dbl[it]   = ldpc_enc_dbl_word(s.msg, (uint32_t)(k * Z), Z, j);
  }
  __syncthreads();
  // rows 0..3 over the message columns
  for (int it = tid; it < 4 * W; it += nt) {
    const int m = it / W, w = it - m * W;
    uint32_t  x = 0;
    for (int e = T::rs(m); e < T::rs(m + 1); ++e) {
      const int c = T::col(e);
      if (c < T::K) {
        x ^= ldpc_enc_get32(s.dbl + c * SD, s.sh[e] + 32u * w);
      }
    }
    s.aux[it] = w == W - 1 ? x & last : x;
  }
  __syncthreads();
  uint32_t a[4] = {0, 0, 0, 0};
  if (tid < W) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      a[m] = s.aux[m * W + tid];
    }
  }
  __syncthreads();  // aux[] is rewritten below
  if (tid < W) {
    s.aux[tid] = a[0] ^ a[1] ^ a[2] ^ a[3];
  }
  if (tid == 0) {
    s.aux[W] = 0;  // funnel pad
  }
  __syncthreads();
  for (int j = tid; j < SD; j += nt) {
    s.sum[j] = ldpc_enc_dbl_word(s.aux, 0, Z, j);
  }
  __syncthreads();
  if (tid < W) {
    // p0 = sum rotated by r0; q = what the second and fourth chunk add (ldpc_enc_c.c:110-224)
    const int r0 = hr_case == 2 ? (Z - 105 % Z) % Z : (hr_case == 3 ? Z - 1 : 0);
    const int r1 = (hr_case == 1 || hr_case == 4) ? 1 % Z : r0;
    const uint32_t m  = tid == W - 1 ? last : 0xFFFFFFFFu;
    const uint32_t p0 = ldpc_enc_get32(s.sum, (uint32_t)r0 + 32u * tid) & m;
    const uint32_t q  = ldpc_enc_get32(s.sum, (uint32_t)r1 + 32u * tid) & m;
    const uint32_t p1 = a[0] ^ q;
    uint32_t       p2, p3 = a[3] ^ q;
    if (hr_case <= 2) {
      p2 = a[2] ^ p3;
    } else {
      p2 = a[1] ^ p1;
    }
    s.aux[0 * W + tid] = p0;
    s.aux[1 * W + tid] = p1;
    s.aux[2 * W + tid] = p2;
    s.aux[3 * W + tid] = p3;
  }
  if (tid == 0) {
    s.aux[4 * W] = 0;
  }
  __syncthreads();
  for (int it = tid; it < 4 * SD; it += nt) {
    const int k = it / SD, j = it - k * SD;
    s.dbl[(T::K + k) * SD + j] = ldpc_enc_dbl_word(s.aux, 32u * (uint32_t)(k * W), Z, j);
  }
  __syncthreads();
  // rows >= 4: message and core parity edges (the row's last edge is its own identity column)
  for (int it = tid; it < (n_rows - 4) * W; it += nt) {
    const int m = 4 + it / W, w = it - (m - 4) * W;
    uint32_t  x = 0;
    for (int e = T::rs(m); e < T::rs(m + 1); ++e) {
      const int c = T::col(e);
      if (c < T::K + 4) {
        x ^= ldpc_enc_get32(s.dbl + c * SD, s.sh[e] + 32u * w);
      }
    }
    s.ext[it] = w == W - 1 ? x & last : x;
  }
  __syncthreads();
}

// bit p of the stored codeword (the first 2Z bits punctured), p < (n_rows + bgK - 2) Z;
// magic = ceil(2^32 / Z): p / Z = umulhi(p, magic) for p < 2^16
template <int BG>
__device__ __forceinline__ uint32_t ldpc_enc_bit(const LdpcEncLds& s, int Z, uint32_t magic, uint32_t p)
{
  using T          = LdpcEncTopo<BG>;
  const int      W = (Z + 31) >> 5;
  const uint32_t c = __umulhi(p, magic) + 2u;
  const uint32_t i = p - (c - 2u) * (uint32_t)Z;
  const uint32_t w = c < (uint32_t)(T::K + 4) ? s.dbl[c * (2 * W + 1) + (i >> 5)]
                                              : s.ext[(c - (T::K + 4)) * W + (i >> 5)];
  return (w >> (i & 31u)) & 1u;
}

}  // namespace srsran_amd
#endif
