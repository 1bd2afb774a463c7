// srsran_4g_amd/csrc/csi_kernel.h -- channel-state feedback of a 2-port x 2-rx cell from the device-resident
// channel estimate: the SINR of every codebook entry (1 and 2 layers), the condition number, and the RI / PMI
// decisions the reference's callers take from them (include/srsran_ue_dl.h: srsran_csi_gpu_t).
#ifndef SRSRAN_AMD_CSI_KERNEL_H
#define SRSRAN_AMD_CSI_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/srsran_ue_dl.h"

namespace srsran_amd {

struct CsiArgs {
  const float2*     ce;          // subframe 0's rows h[port][rx], row (2 port + rx) at ce + that * row_stride
  size_t            sf_stride;   // float2 between subframes
  size_t            row_stride;  // float2 between rows
  uint32_t          row_len;     // index j reads row[j % row_len]: 12 nof_prb for the one-row AVERAGE estimate,
                                 // nof_symbols for a full one
  uint32_t          nof_symbols; // SRSRAN_NOF_RE(cell), >= 192
  const float*      noise;       // device: subframe b's noise estimate at noise[b * noise_stride]; null: noise_val
  uint32_t          noise_stride;
  float             noise_val;
  srsran_csi_gpu_t* out;         // one record a subframe
};
// one workgroup a subframe, grid = nsf
hipError_t csi_launch(const CsiArgs& a, uint32_t nsf, hipStream_t stream);

}  // namespace srsran_amd
#endif
