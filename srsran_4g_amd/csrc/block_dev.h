// srsran_4g_amd/csrc/block_dev.h -- device (32, O) block-code ML decoder shared by the UCI-on-PUSCH
// kernels (uci_kernel.hip) and PUCCH format 3 (pucch_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srsran_amd {
namespace {

// (32, O) basis sequences, 36.212 Table 5.2.2.6.4-1; bit n of word i is M_{i,n} (block.c:37-43)
__constant__ uint16_t kBlockBasis[32] = {0x403, 0x607, 0x749, 0x50D, 0x48F, 0x5D3, 0x755, 0x599, 0x69B, 0x65D, 0x6E5,
                                         0x567, 0x7A9, 0x6AB, 0x4B1, 0x6F3, 0x277, 0x139, 0x0FB, 0x061, 0x445, 0x60B,
                                         0x591, 0x717, 0x3DF, 0x4E3, 0x32D, 0x3AF, 0x175, 0x1FD, 0x7FF, 0x001};

// srsran_block_decode over 32 accumulated soft bits (block.c:196-232) by one wave: returns the
// correlation, writes min(nbits, 11) bits.  The 2^O hypotheses run across the lanes; the reference's
// strict ">" from a zero start keeps the first maximum.
__device__ int32_t block_ml(const int16_t* llr32, uint32_t nbits, uint8_t* data, int lane)
{
  nbits               = min(nbits, 11u);
  const uint32_t ng   = 1u << nbits;
  int32_t        best = INT32_MIN;
  uint32_t       bw   = 0;
  for (uint32_t w = (uint32_t)lane; w < ng; w += 64) {
    int32_t corr = 0;
    for (int i = 0; i < 32; i++) {
      const int32_t e = (int32_t)(__builtin_popcount(w & kBlockBasis[i]) & 1) * 2 - 1;
      corr += (int32_t)llr32[i] * e;
    }
    if (corr > best) {  // ascending w: the first maximum of the lane
      best = corr;
      bw   = w;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const int32_t  ob = __shfl_xor(best, off, 64);
    const uint32_t ow = (uint32_t)__shfl_xor((int)bw, off, 64);
    if (ob > best || (ob == best && ow < bw)) {
      best = ob;
      bw   = ow;
    }
  }
  if (best <= 0) {  // max_corr starts at 0 with word 0 and only a strictly larger one replaces it
    best = 0;
    bw   = 0;
  }
  if (lane == 0) {
    for (uint32_t i = 0; i < nbits; i++) {
      data[i] = (uint8_t)((bw >> i) & 1u);
    }
  }
  return best;
}

}  // namespace
}  // namespace srsran_amd
