// srsran_4g_amd/csrc/sch_internal.h -- what the other units of the library call in the units behind srsran_sch.h
// beside the public header: the UL-SCH decode on device LLRs and its batch (ulsch_api.cpp) and the object's stream
// (sch_api.cpp), for pusch_api.cpp and ue_ul_api.cpp; the UL-SCH transmit step (ulsch_api.cpp, for pusch_api.cpp); the
// device views of a soft buffer (softbuffer_api.cpp, for nr_sch_api.cpp); the transmitter's rate-matching table
// (rm_turbo_api.cpp).  What those units share among themselves is in sch_units.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/srsran_sch.h"
#include "pusch_tx_kernel.h"

namespace srsran_amd {

// srsran_ulsch_decode on the device: d_q the PUSCH-order LLRs, d_c the unpacked scrambling sequence (UCI) or null
int ulsch_decode_dev(srsran_sch_t* q, srsran_pusch_cfg_t* cfg, int16_t* d_q, const uint8_t* d_c, uint8_t* data,
                     srsran_uci_value_t* uci_data);

hipStream_t sch_stream(srsran_sch_t* q);

// moves the object's decode stream to a hardware queue of its own
int sch_own_queue(srsran_sch_t* q);

// ---- the batched UL-SCH receive behind srsran_pusch_gpu_decode_batch: srsran_ulsch_decode (sch.c:994-1193) for many
// UEs at once, UCI included, with every stage one launch over the batch (ACK/RI decode, de-interleaver, CQI decode,
// decode_tb) ----
struct UlschBatchUe {
  srsran_pusch_cfg_t* cfg;
  int16_t*            d_q;       // device: the UE's PUSCH-order LLRs (nof_bits; ACK positions zeroed in place)
  const uint8_t*      d_c;       // device: its unpacked scrambling sequence (1-bit ACK / RI), or null
  int16_t*            d_g;       // device scratch: nof_bits de-interleaved LLRs
  uint8_t*            d_data;    // device scratch inside [d_data_base, + data_bytes): tbs / 8 bytes
  bool                new_data;  // a new transmission: the soft buffer is reset first
  uint8_t*            data;      // host out: the TB (tbs / 8 bytes), or null
  srsran_uci_value_t* uci;       // host out (required when the UE carries UCI)
  int                 ret;       // out: srsran_ulsch_decode's return for this UE
  float               avg;       // out: avg_iterations of this UE's TB (the previous TB's without one)
};

// Enqueues the whole batch on `st` (the UL-SCH object's stream), waits for it (one host sync, two
// when a higher-layer subband CQI report's size depends on a decoded RI) and fills the outputs.
// Returns SRSRAN_SUCCESS when the batch ran (per-UE errors are in ret), an error otherwise.
int ulsch_decode_batch_dev(srsran_sch_t* q, uint32_t n, UlschBatchUe* ues, const uint8_t* d_data_base,
                           size_t data_bytes, hipStream_t st);

// ---- the UL-SCH transmit step shared by srsran_ulsch_encode and the PUSCH / UE uplink transmit paths: the host part
// of srsran_ulsch_encode (sch.c:1195-1337) for a batch of transmissions and the launches that leave each TB's
// rate-matched bits on the device ----
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

// device views of a soft buffer
uint8_t* softbuffer_dflags(srsran_softbuffer_rx_t* q);
uint8_t* softbuffer_ddata(srsran_softbuffer_rx_t* q);
uint32_t softbuffer_data_stride(srsran_softbuffer_rx_t* q);

// rate-matching read-out table of (code block size index, rv) for the transmitter, period *N
bool rm_fwd_table(uint32_t cb_idx, uint32_t rv, const uint16_t** d_fwd, uint32_t* N);

}  // namespace srsran_amd
