// srsran_4g_amd/csrc/ldpc_enc_kernel.hip -- NR LDPC encoder and stand-alone rate matcher for CDNA4 (gfx950).
//
// ldpc_enc_kernel: srsran_ldpc_encoder_encode_rm (ldpc_encoder.c:55-97) for a batch of messages of one
//   (base graph, lifting size), one workgroup per message.  The byte-per-bit message is packed into LDS
//   (`1U &` masks the filler flag, ldpc_enc_c.c:104), ldpc_enc_core (ldpc_enc_core.h) encodes it there,
//   and the codeword goes out as bytes: the systematic bytes behind the 2Z punctured ones are copied
//   through unmasked (ldpc_encoder.c:81-84), parity bytes are 0 / 1.  Only the rows the rate-matched
//   length needs are computed, and nothing is written beyond them.  One wave per message up to Z = 32
//   (every pass has at most 42 work items there), four waves above.
// ldpc_rm_tx_kernel: srsran_ldpc_rm_tx (ldpc_rm.c:582-610) by position: output byte t = j Qm + i is the
//   (i cols + j)-th selected bit, whose place in the circular buffer nr_rm_tx_pos.h gives in closed form.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldpc_enc_core.h"
#include "ldpc_enc_kernel.h"

namespace srsran_amd {

template <int BG>
__global__ __launch_bounds__(256) void ldpc_enc_kernel(LdpcEncArgs a)
{
  using T = LdpcEncTopo<BG>;
  __shared__ LdpcEncLds s;
  const int      Z   = a.ls;
  const int      K   = T::K * Z;
  const uint8_t* in  = a.in + (size_t)blockIdx.x * a.in_stride;
  uint8_t*       out = a.out + (size_t)blockIdx.x * a.out_stride;
  for (int e = threadIdx.x; e < T::NE; e += blockDim.x) {
    s.sh[e] = a.sh[e];
  }
  for (int j = threadIdx.x; j <= (K + 31) / 32; j += blockDim.x) {  // one word more: the funnel pad
    uint32_t w = 0;
    for (int b = 0; b < 32; ++b) {
      const int i = 32 * j + b;
      w |= i < K ? (uint32_t)(in[i] & 1u) << b : 0u;
    }
    s.msg[j] = w;
  }
  __syncthreads();
  ldpc_enc_core<BG>(s, Z, a.hr_case, a.n_rows);
  const uint32_t sys = (uint32_t)(T::K - 2) * Z, len = (uint32_t)(a.n_rows + T::K - 2) * Z;
  for (uint32_t p = threadIdx.x; p < len; p += blockDim.x) {
    out[p] = p < sys ? in[p + 2 * Z] : (uint8_t)ldpc_enc_bit<BG>(s, Z, a.magic_ls, p);
  }
}

__global__ __launch_bounds__(256) void ldpc_rm_tx_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                          uint32_t E, uint32_t Qm, NrRmTxSel sel)
{
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= E) {
    return;
  }
  const uint32_t j = t / Qm, i = t - j * Qm;
  const uint32_t k = nr_rm_tx_il(j, i, E / Qm);
  out[t]           = in[nr_rm_tx_pos(sel, k % sel.L)];
}

hipError_t ldpc_enc_launch(int bg, const LdpcEncArgs& a, hipStream_t stream)
{
  if (a.ncw == 0) {
    return hipSuccess;
  }
  const dim3 grid(a.ncw), block(a.ls <= 32 ? 64 : 256);
  if (bg == 0) {
    hipLaunchKernelGGL(ldpc_enc_kernel<0>, grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL(ldpc_enc_kernel<1>, grid, block, 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t ldpc_rm_tx_launch(const uint8_t* d_in, uint8_t* d_out, uint32_t E, uint32_t Qm, const NrRmTxSel& sel,
                             hipStream_t stream)
{
  if (E == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(ldpc_rm_tx_kernel, dim3((E + 255) / 256), dim3(256), 0, stream, d_in, d_out, E, Qm, sel);
  return hipGetLastError();
}

}  // namespace srsran_amd
