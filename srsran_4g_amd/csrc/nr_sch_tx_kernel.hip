// srsran_4g_amd/csrc/nr_sch_tx_kernel.hip -- NR SCH transmit kernels for CDNA4 (gfx950).
//
// nr_tb_crc_kernel: the TB CRC over the payload (sch_nr.c:465) by the slice / shift-factor scheme of
//   nr_tb_kernel (nr_tb_crc.h): grid (TB, slice), 16 bytes per thread, the parts XOR into the TB's
//   accumulator word.
// nr_tx_cb_kernel: sch_nr.c:473-549 for every code block of a batch, one workgroup per block, entirely in
//   LDS.  The block's payload bytes are packed into the message (byte-aligned: the host refuses C > 1 with
//   (Kp - L_cb) % 8 != 0), the last block appends the TB CRC, CRC24B is attached when L_cb != 0 (4-byte
//   chunks shifted into place with x^n mod P and XOR-combined, as the decoder's early stop does), filler
//   bits are zeros (`1U &`, ldpc_enc_c.c:104).  ldpc_enc_core (ldpc_enc_core.h) computes only the rows
//   the transmitted span reaches, and the epilogue rate-matches straight out of LDS: output byte
//   t = j Qm + i is selected bit i cols + j (ldpc_rm.c:348-360), whose position comes in closed form from
//   nr_rm_tx_pos.h (the inverse of nr_rm_kernel's gather).  The codeword never goes to HBM.  Four output
//   bytes per thread, stored as one aligned dword where the block's E bytes cover it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc24_dev.h"
#include "ldpc_enc_core.h"
#include "nr_sch_tx_kernel.h"

namespace srsran_amd {

__constant__ TbCrcShift c_tx_shift = TbCrcShift();

__global__ __launch_bounds__(NR_TB_THREADS) void nr_tb_crc_kernel(const NrTxTb* __restrict__ tbs)
{
  __shared__ uint32_t s_tab[256];
  __shared__ uint32_t s_crc;
  const NrTxTb   d       = tbs[blockIdx.x];
  const uint32_t slice   = blockIdx.y;
  const uint32_t nslices = (d.nbytes + NR_TB_SLICE - 1) / NR_TB_SLICE;
  if (slice >= nslices) {
    return;
  }
  const uint32_t poly  = d.L_tb == 24 ? 0x1864CFBu : 0x11021u;  // CRC24A / CRC16 (sch_nr.c:433)
  const int      order = (int)d.L_tb;
  const uint32_t mask  = (1u << order) - 1u;
  if (threadIdx.x == 0) {
    s_crc = 0;
  }
  tb_crc_table(s_tab, poly, order);
  __syncthreads();
  // chunks are counted from the end of the payload, as in nr_tb_kernel
  const uint32_t back = slice * NR_TB_SLICE + threadIdx.x * NR_TB_BYTES;
  const uint32_t b1   = back < d.nbytes ? d.nbytes - back : 0u;
  const uint32_t b0   = b1 > NR_TB_BYTES ? b1 - NR_TB_BYTES : 0u;
  if (b0 < b1) {
    uint8_t v[NR_TB_BYTES];
#pragma unroll
    for (uint32_t k = 0; k < NR_TB_BYTES; ++k) {
      v[k] = k < b1 - b0 ? d.payload[b0 + k] : 0;
    }
    uint32_t crc = 0;
#pragma unroll
    for (uint32_t k = 0; k < NR_TB_BYTES; ++k) {
      if (k < b1 - b0) {
        crc = ((crc << 8) & mask) ^ s_tab[((crc >> (order - 8)) ^ v[k]) & 0xFFu];
      }
    }
    crc = mulmod(crc, c_tx_shift.thread[order == 24 ? 0 : 1][threadIdx.x], poly, order);
    atomicXor(&s_crc, crc & mask);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicXor(d.crc, mulmod(s_crc, c_tx_shift.slice[order == 24 ? 0 : 1][slice], poly, order) & mask);
  }
}

__device__ __forceinline__ uint32_t brev8(uint32_t b) { return __brev(b) >> 24; }

// byte `idx` of the message (bits 8 idx .. 8 idx + 7, first bit = MSB of v) into the LSB-first words
__device__ __forceinline__ void msg_or_byte(uint32_t* msg, uint32_t idx, uint32_t v)
{
  msg[idx >> 2] |= brev8(v & 0xFFu) << (8u * (idx & 3u));
}

template <int BG>
__device__ __forceinline__ void encode_and_match(LdpcEncLds& s, const NrTxCb& d)
{
  const int Z = d.Z;
  ldpc_enc_core<BG>(s, Z, d.hr_case, d.n_rows);
  const uint32_t E = d.E, Qm = d.Qm, cols = E / Qm, L = d.sel.L;
  const uint32_t magic_qm = Qm > 1 ? 0xFFFFFFFFu / Qm + 1u : 0u;  // ceil(2^32 / Qm)
  const bool     wrap     = E > L;
  const uint32_t a0       = (uint32_t)(reinterpret_cast<uintptr_t>(d.e) & 3u);
  const uint32_t nq       = (a0 + E + 3u) / 4u;
  for (uint32_t q = threadIdx.x; q < nq; q += blockDim.x) {
    const int t0 = (int)(4u * q) - (int)a0;
    uint32_t  v  = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int t = t0 + b;
      if (t >= 0 && (uint32_t)t < E) {
        const uint32_t j = Qm > 1 ? __umulhi((uint32_t)t, magic_qm) : (uint32_t)t;
        const uint32_t i = (uint32_t)t - j * Qm;
        uint32_t       k = nr_rm_tx_il(j, i, cols);
        if (wrap) {
          k -= L * (uint32_t)(((uint64_t)k * d.inv_L) >> 40);
        }
        v |= ldpc_enc_bit<BG>(s, Z, d.magic_ls, nr_rm_tx_pos(d.sel, k)) << (8 * b);
      }
    }
    if (t0 >= 0 && (uint32_t)t0 + 4u <= E) {
      *reinterpret_cast<uint32_t*>(d.e + t0) = v;
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int t = t0 + b;
        if (t >= 0 && (uint32_t)t < E) {
          d.e[t] = (uint8_t)(v >> (8 * b));
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void nr_tx_cb_kernel(const NrTxCb* __restrict__ cbs,
                                                        const uint32_t* __restrict__ xpow24b)
{
  __shared__ LdpcEncLds s;
  __shared__ uint32_t   s_crc;
  const NrTxCb   d  = cbs[blockIdx.x];
  const uint32_t Kr = (uint32_t)d.Z * (d.bg == 0 ? 22u : 10u);
  const uint32_t ne = d.bg == 0 ? LDPC_BG1_NEDGES : LDPC_BG2_NEDGES;
  for (uint32_t e = threadIdx.x; e < ne; e += blockDim.x) {
    s.sh[e] = d.sh[e];
  }
  if (threadIdx.x == 0) {
    s_crc = 0;
  }
  // payload bytes, MSB first, into LSB-first words; everything behind them zero (CRC bits are ORed in below)
  for (uint32_t j = threadIdx.x; j <= (Kr + 31u) / 32u; j += blockDim.x) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t m = 0; m < 4; ++m) {
      const uint32_t b = 4u * j + m;
      w |= b < d.data_bytes ? brev8(d.payload[d.byte0 + b]) << (8u * m) : 0u;
    }
    s.msg[j] = w;
  }
  __syncthreads();
  uint32_t nb = d.data_bytes;
  if (d.L_tb && threadIdx.x == 0) {  // the last block: TB CRC behind the payload (sch_nr.c:486-495)
    const uint32_t c = *d.tb_crc;
    for (uint32_t m = 0; m < d.L_tb / 8u; ++m) {
      msg_or_byte(s.msg, nb + m, c >> (d.L_tb - 8u - 8u * m));
    }
  }
  nb += d.L_tb / 8u;
  if (d.L_cb) {  // srsran_crc_attach of CRC24B over the nb bytes (sch_nr.c:509-512)
    __syncthreads();
    const uint32_t poly = 0x1800063u;
    for (uint32_t j = threadIdx.x; 4u * j < nb; j += blockDim.x) {
      const uint32_t end = min(4u * j + 4u, nb);
      const uint32_t w   = s.msg[j];
      uint32_t       crc = 0;
      for (uint32_t b = 4u * j; b < end; ++b) {
        crc = crc24_byte(crc, brev8((w >> (8u * (b & 3u))) & 0xFFu), poly);
      }
      atomicXor(&s_crc, clmul24(crc, xpow24b[8u * (nb - end)], poly) & 0xFFFFFFu);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t c = s_crc;
      for (uint32_t m = 0; m < 3; ++m) {
        msg_or_byte(s.msg, nb + m, c >> (16u - 8u * m));
      }
    }
  }
  __syncthreads();
  if (d.bg == 0) {
    encode_and_match<0>(s, d);
  } else {
    encode_and_match<1>(s, d);
  }
}

hipError_t nr_tb_crc_launch(const NrTxTb* d_tbs, uint32_t ntb, uint32_t slices, hipStream_t stream)
{
  if (ntb == 0) {
    return hipSuccess;
  }
  if (slices > NR_TB_MAX_SLICES) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(nr_tb_crc_kernel, dim3(ntb, slices > 0 ? slices : 1), dim3(NR_TB_THREADS), 0, stream, d_tbs);
  return hipGetLastError();
}

hipError_t nr_tx_cb_launch(const NrTxCb* d_cbs, uint32_t ncb, const uint32_t* xpow24b, uint32_t max_ls,
                           hipStream_t stream)
{
  if (ncb == 0) {
    return hipSuccess;
  }
  // up to Z = 32 a chunk is one word and no pass has more than 42 work items: one wave per block
  hipLaunchKernelGGL(nr_tx_cb_kernel, dim3(ncb), dim3(max_ls <= 32 ? 64 : 256), 0, stream, d_cbs, xpow24b);
  return hipGetLastError();
}

}  // namespace srsran_amd
