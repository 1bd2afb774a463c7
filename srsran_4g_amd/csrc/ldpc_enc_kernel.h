// srsran_4g_amd/csrc/ldpc_enc_kernel.h -- launch interface of the HIP NR LDPC encoder and of the
// stand-alone LDPC rate matcher (transmit side).
#ifndef SRSRAN_AMD_LDPC_ENC_KERNEL_H
#define SRSRAN_AMD_LDPC_ENC_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nr_rm_tx_pos.h"

namespace srsran_amd {

// the high-rate solution 1..4 of a (base graph, lifting-size set index) (ldpc_encoder.c:109-116)
inline int ldpc_enc_hr_case(int bg, int set)
{
  return bg == 0 ? (set != 6 ? 1 : 2) : ((set != 3 && set != 7) ? 3 : 4);
}

// One batch of messages of one (base graph, lifting size), byte-per-bit buffers as ldpc_encoder.c.
struct LdpcEncArgs {
  const uint8_t*  in;          // ncw x liftK bytes (bit in the LSB; 254 marks a filler bit), in_stride apart
  uint32_t        in_stride;
  uint8_t*        out;         // ncw x out_len bytes, out_stride apart: systematic bytes copied, parity 0 / 1
  uint32_t        out_stride;
  uint32_t        ncw;
  int             ls;
  int             hr_case;     // ldpc_enc_hr_case(bg, set index)
  int             n_rows;      // base-graph rows computed; out_len = (n_rows + bgK - 2) ls bytes are written
  const uint32_t* sh;          // V mod ls per edge, edge order (device)
  uint32_t        magic_ls;    // ceil(2^32 / ls)
};

hipError_t ldpc_enc_launch(int bg, const LdpcEncArgs& a, hipStream_t stream);

// out[j Qm + i] = in[pos(rank(i cols + j))], E bytes (srsran_ldpc_rm_tx, ldpc_rm.c:582-610)
hipError_t ldpc_rm_tx_launch(const uint8_t* d_in, uint8_t* d_out, uint32_t E, uint32_t Qm, const NrRmTxSel& sel,
                             hipStream_t stream);

}  // namespace srsran_amd
#endif
