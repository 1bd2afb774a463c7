// srsran_4g_amd/csrc/seq_mod_dev.h -- device helpers shared by the kernels that scramble and map bits
// (llr_kernel.hip: PDSCH / control transmit and the LLR stages; pusch_tx_kernel.hip: PUSCH transmit): the Gold
// sequence LFSR steps (36.211 7.2, common/sequence.c), the GF(2) jump-table layout gold_tables_init() builds, and the
// constellations of modem/lte_tables.c:45-160.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srsran_amd {

static constexpr int GOLD_NC   = 1600;  // sequence.c:39
static constexpr int JUMP_BITS = 24;    // offsets below 2^24 bits
static constexpr int JUMP_LVLS = 3;     // offset = b0 + 256 b1 + 65536 b2

struct GoldTables {
  uint32_t        x1_nc;      // x1 after Nc steps from x1 = 1
  uint32_t        x2_nc[31];  // x2 after Nc steps from the unit seed 1 << i
  const uint32_t* jump;       // [lvl][b][lfsr][32]: columns of A_lfsr^(b * 256^lvl) (device memory)
  const uint32_t* stride;     // [MOD][lane][lfsr][32]: columns of A_lfsr^(lane * GOLD_LANE_SYMBOLS * Qm) (device)
};
// the current device's tables (built by gold_tables_init() on first use), for a kernel file's own __constant__ copy
hipError_t gold_tables_get(GoldTables* out);

__host__ __device__ inline uint32_t step_x1(uint32_t s) { return (s >> 1) ^ (((s ^ (s >> 3)) & 1u) << 30); }
__host__ __device__ inline uint32_t step_x2(uint32_t s)
{
  return (s >> 1) ^ (((s ^ (s >> 1) ^ (s >> 2) ^ (s >> 3)) & 1u) << 30);
}
__host__ __device__ inline uint32_t apply(const uint32_t* cols, uint32_t v)
{
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 31; i++) {
    r ^= ((v >> i) & 1u) ? cols[i] : 0u;
  }
  return r;
}

// columns (32 dwords, 16-byte aligned) applied to v
__device__ __forceinline__ uint32_t apply_cols(const uint32_t* __restrict__ cols, uint32_t v)
{
  const uint4* c4 = reinterpret_cast<const uint4*>(cols);
  uint32_t     r  = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const uint4 c = c4[q];
    r ^= ((v >> (4 * q)) & 1u) ? c.x : 0u;
    r ^= ((v >> (4 * q + 1)) & 1u) ? c.y : 0u;
    r ^= ((v >> (4 * q + 2)) & 1u) ? c.z : 0u;
    if (q < 7) {
      r ^= ((v >> (4 * q + 3)) & 1u) ? c.w : 0u;
    }
  }
  return r;
}

// advance both LFSRs by 16 bits and return c(n..n+15) (bit k = c(n+k)): the recurrences
// x1(m+31) = x1(m+3) ^ x1(m) and x2(m+31) = x2(m+3) ^ x2(m+2) ^ x2(m+1) ^ x2(m) give 28 new bits
// per shift-xor, 16 of which are used
__device__ __forceinline__ uint32_t gold16(uint32_t& x1, uint32_t& x2)
{
  const uint32_t c  = (x1 ^ x2) & 0xFFFFu;
  const uint32_t n1 = ((x1 >> 3) ^ x1) & 0xFFFFu;
  const uint32_t n2 = ((x2 >> 3) ^ (x2 >> 2) ^ (x2 >> 1) ^ x2) & 0xFFFFu;
  x1                = (x1 >> 16) | (n1 << 15);
  x2                = (x2 >> 16) | (n2 << 15);
  return c;
}

// modulation tables of lte_tables.c:45-160, as the same float expressions
__device__ __forceinline__ float qam64_level(uint32_t hi, uint32_t lo)  // (b2, b4) -> 3, 1, 5, 7 / sqrt(42)
{
  const uint32_t m = hi * 2 + lo;
  return m == 0 ? 3.0f / sqrtf(42.0f) : m == 1 ? 1.0f / sqrtf(42.0f) : m == 2 ? 5.0f / sqrtf(42.0f) : 7.0f / sqrtf(42.0f);
}

// symbol of modulation `mod` (1 QPSK, 2 16QAM, 3 64QAM, 4 256QAM) from its Qm bits, b0 first (MSB)
__device__ __forceinline__ float2 modulate(int mod, uint32_t i)
{
  if (mod == 1) {
    const float l = (float)0.70710678118654752440;  // M_SQRT1_2
    return make_float2((i & 2u) ? -l : l, (i & 1u) ? -l : l);
  }
  if (mod == 2) {
    const float l1 = 1.0f / sqrtf(10.0f), l2 = 3.0f / sqrtf(10.0f);
    const float re = (i & 2u) ? l2 : l1, im = (i & 1u) ? l2 : l1;
    return make_float2((i & 8u) ? -re : re, (i & 4u) ? -im : im);
  }
  if (mod == 3) {
    const float re = qam64_level((i >> 3) & 1u, (i >> 1) & 1u), im = qam64_level((i >> 2) & 1u, i & 1u);
    return make_float2((i & 32u) ? -re : re, (i & 16u) ? -im : im);
  }
  float offset = -1, re = 0, im = 0;  // set_256QAMtable's loop
  for (uint32_t j = 0; j < 4; j++) {
    re += offset;
    im += offset;
    offset *= 2;
    re *= (i & (1u << (2 * j + 1))) ? +1 : -1;
    im *= (i & (1u << (2 * j + 0))) ? +1 : -1;
  }
  return make_float2(re / sqrtf(170), im / sqrtf(170));
}

}  // namespace srsran_amd
