// srsran_4g_amd/csrc/nr_tb_crc.h -- slice / shift-factor scheme of the NR TB CRC, shared by the receive
// (nr_tb_kernel) and transmit (nr_tb_crc_kernel) sides: a TB's payload is cut, counted from its end,
// into slices of NR_TB_SLICE bytes and those into 16-byte chunks, one per thread; a chunk's CRC (from
// zero) is moved to its place with x^(8 bytes after) mod P from the tables below, and the parts XOR.
#ifndef SRSRAN_AMD_NR_TB_CRC_H
#define SRSRAN_AMD_NR_TB_CRC_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srsran_amd {

// TB slices: each workgroup handles NR_TB_SLICE payload bytes of one TB
constexpr uint32_t NR_TB_THREADS = 256;
constexpr uint32_t NR_TB_BYTES   = 16;  // contiguous bytes per thread
constexpr uint32_t NR_TB_SLICE   = NR_TB_THREADS * NR_TB_BYTES;
constexpr uint32_t NR_TB_MAX_SLICES = 16;  // shift factors kept: payloads up to 64 KiB

// a * b mod P, P of degree `order` <= 24 given with its x^order bit, a, b < 2^order (Horner over
// the 24 low bits of b: leading zero bits leave r = 0)
__host__ __device__ constexpr uint32_t mulmod(uint32_t a, uint32_t b, uint32_t poly, int order)
{
  uint32_t r = 0;
#pragma unroll
  for (int i = 23; i >= 0; i--) {
    r = (r << 1) ^ (((b >> i) & 1u) ? a : 0u);
    r ^= ((r >> order) & 1u) ? poly : 0u;
  }
  return r;
}

// Shift factors of the TB CRCs ([0] CRC24A, [1] CRC16, phy_common.h:72-74): thread[t] = x^(8 16 t)
// and slice[s] = x^(8 NR_TB_SLICE s) mod P -- the bytes after a thread's chunk inside its slice and
// after the slice
struct TbCrcShift {
  uint32_t thread[2][NR_TB_THREADS];
  uint32_t slice[2][NR_TB_MAX_SLICES];
  constexpr TbCrcShift() : thread(), slice()
  {
    const uint32_t polys[2] = {0x1864CFBu, 0x11021u};
    const int      ords[2]  = {24, 16};
    for (int t = 0; t < 2; t++) {
      uint32_t x128 = 1u << 8;  // x^8 -> x^128
      for (int k = 0; k < 4; k++) {
        x128 = mulmod(x128, x128, polys[t], ords[t]);
      }
      thread[t][0] = 1u;
      for (uint32_t i = 1; i < NR_TB_THREADS; i++) {
        thread[t][i] = mulmod(thread[t][i - 1], x128, polys[t], ords[t]);
      }
      const uint32_t xs = mulmod(thread[t][NR_TB_THREADS - 1], x128, polys[t], ords[t]);  // x^(8 16 256)
      slice[t][0]       = 1u;
      for (uint32_t i = 1; i < NR_TB_MAX_SLICES; i++) {
        slice[t][i] = mulmod(slice[t][i - 1], xs, polys[t], ords[t]);
      }
    }
  }
};
static_assert(NR_TB_SLICE == 16 * NR_TB_THREADS, "slice = threads x 16 bytes");

// the 256-entry table of a CRC of `order` bits, MSB first (crc.c:38-67), into LDS
__device__ __forceinline__ void tb_crc_table(uint32_t* s_tab, uint32_t poly, int order)
{
  const uint32_t mask = (1u << order) - 1u;
  for (uint32_t v = threadIdx.x; v < 256; v += blockDim.x) {
    uint32_t c = v << (order - 8);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      c = (c & (1u << (order - 1))) ? ((c << 1) ^ poly) : (c << 1);
    }
    s_tab[v] = c & mask;
  }
}

}  // namespace srsran_amd
#endif
