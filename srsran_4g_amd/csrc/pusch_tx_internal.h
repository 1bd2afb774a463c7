// srsran_4g_amd/csrc/pusch_tx_internal.h -- the UL-SCH transmit step shared by srsran_ulsch_encode (sch_api.cpp) and
// the PUSCH / UE uplink transmit paths (pusch_api.cpp): the host part of srsran_ulsch_encode (sch.c:1195-1337) for a
// batch of transmissions and the launches that leave each TB's rate-matched bits on the device.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/srsran_sch.h"
#include "pusch_tx_kernel.h"

namespace srsran_amd {

struct UlschTxJob {
  srsran_pusch_cfg_t*       cfg;     // K_segm is written
  const srsran_uci_value_t* uci;
  const uint8_t*            d_data;  // device payload, tbs / 8 bytes (may be null with tbs == 0)
  bool                      want_g;  // the packed g bits are produced (PuschTxUe::g_pack)
  bool                      want_q;  // the packed q bits before scrambling are produced (PuschTxUe::q_pack)
  int                       ret;     // out: srsran_ulsch_encode's return, (Q'_ACK + Q'_RI) Qm, or an error
};

// For every job: segmentation, Q'_RI / Q'_CQI / Q'_ACK, the coded CQI bits and the RI / ACK bit types (host), then
// one TB CRC launch and one code block launch over the batch.  Fills the multiplexing fields of desc[i] (device
// pointers into the object's transmit scratch, valid until the next call on q; seed is left to the caller) and leaves
// the other fields as they are.  Returns SRSRAN_SUCCESS when every job was accepted; otherwise the first failing
// job's error (in its ret) and nothing is launched.
int ulsch_tx_prepare(srsran_sch_t* q, uint32_t n, UlschTxJob* jobs, PuschTxUe* desc, hipStream_t st);

}  // namespace srsran_amd
