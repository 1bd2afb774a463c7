// srsran_4g_amd/csrc/sch_units.h -- what the host units behind include/srsran_sch.h need of one another
// (rm_turbo_api.cpp, softbuffer_api.cpp, sch_api.cpp, ulsch_api.cpp): the de-matching tables, a soft buffer's device
// state, the srsran_sch_t object's device context and the DL-SCH steps the UL-SCH paths reuse.  The structs live here
// so that the per-code-block loops read their fields directly.  What the rest of the library calls is in
// sch_internal.h; the HIP-free host arithmetic in uci_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <utility>
#include <vector>

#include "../../include/srsran_sch.h"
#include "dev_buf.h"
#include "enc_kernel.h"
#include "sch_kernel.h"
#include "stage_copy.h"

namespace srsran_amd {

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// ---------------- rate de-matching tables (rm_turbo_api.cpp; rm_turbo.c:175-317) ----------------
// For one (K, rv, layout): inv[p] = index, in the rv's circular read-out order with
// the dummy bits dropped, of the coded bit stored at soft-buffer position p; that
// order repeats with period N = 3K+12 along the E received LLRs.
struct InvTable {
  uint16_t* d   = nullptr;
  uint32_t  len = 0;  // soft buffer positions of the layout
  uint32_t  N   = 0;  // 3K + 12
};
// nsb: sub-blocks of the decoder layout (0 natural; 8 / 16 / 32 as rm_turbo.c's deinterleaver_sb)
bool inv_table_nsb(uint32_t cb_idx, uint32_t rv, uint32_t nsb, InvTable* out);
// the natural layout, or that of the 16-bit decoder that takes the size
bool inv_table(uint32_t cb_idx, uint32_t rv, bool tdec_layout, InvTable* out);

// ---------------- a soft buffer's device state (softbuffer_api.cpp) ----------------
struct SbGpu {
  short*          d_buf = nullptr;  // max_cb x stride int16, from the arena (sb_arena_alloc / sb_arena_free)
  DevBuf<uint8_t> d_data;           // max_cb x data_stride bytes
  DevBuf<uint8_t> d_flags;          // [0, max_cb): cb_crc, [max_cb]: tb_crc
  uint32_t stride = 0, data_stride = 0;
  size_t   buf_bytes = 0;      // d_buf size (rounded as the arena hands it out)
  int      buf_dev   = -1;     // >= 0: d_buf lives in that device's soft-buffer arena
  int      dev       = 0;      // the device every buffer of this soft buffer lives on
};

// ---------------- sch object device context (sch_api.cpp) ----------------
// Descriptor staging of one batch.  A ring of kStageRing slots: the host builds the next batches while the GPU
// still reads earlier ones' descriptors, and waits only for the slot's previous user (kStageRing batches back).
constexpr int kStageRing = 3;
struct StageSlot {
  hipEvent_t staged = nullptr;  // SRSRAN_AMD_STAGE=side: this slot's last upload done (pinned staging reusable)
  hipEvent_t done   = nullptr;  // SRSRAN_AMD_STAGE=side: the batch that last used this slot finished with it
  uint32_t   seq    = 0;        // default staging: fence sequence number of the batch that last filled the slot
  bool       used   = false;
  char*      h      = nullptr;  // pinned coherent host memory (stage_host_alloc)
  char*      hd     = nullptr;  // its device alias
  DevBuf<char> d;               // same capacity
};

struct SchCtx {
  hipStream_t stream = nullptr;
  hipStream_t copy   = nullptr;  // descriptor uploads of the batch path, ahead of the launches that read them
  hipEvent_t  done   = nullptr;  // last batch finished with the shared scratch (cbout, flags, chunk CRCs, wide rows)
  StageSlot   ring[kStageRing];
  uint32_t    ring_next = 0;
  StageFence    fence;  // the copy kernel's "slot read" words (stage_copy.h)
  StreamHandoff ho;     // stream of the previous batch (device-side reuse of slots and scratch)
  DevBuf<uint8_t> d_cbout;   // SCH_SLOT_BYTES a slot
  DevBuf<uint8_t> d_noi;     // a byte a slot
  DevBuf<uint8_t> d_crc_ok;  // a byte a slot; the three grow together
  // synchronous decode scratch
  DevBuf<int16_t> d_e;       // int8 values with llr_is_8bit
  DevBuf<uint8_t> d_data;
  DevBuf<int32_t> d_res;
  DevBuf<float>   d_avg;
  PinBuf<uint8_t> h_io;      // flags in/out, result, avg
  DevBuf<uint8_t> d_zero;    // a cleared cb_crc flag for new transmissions
  bool        used = false;
  DevBuf<int16_t> d_ul;      // srsran_ulsch_decode: q then g bits
  DevBuf<UlDeint> d_uldesc;  // srsran_ulsch_gpu_decode_batch descriptors (device)
  PinBuf<UlDeint> h_uldesc;  // their pinned staging, grown with d_uldesc
  hipEvent_t  uldesc_used = nullptr;  // recorded after the de-interleaver launch that reads them
  bool        uldesc_live = false;
  DevBuf<uint8_t> d_uci;     // srsran_ulsch_decode with UCI: descriptors, results, sequence
  DevBuf<uint8_t> d_ubs;     // the batched UL-SCH receive: descriptors and results (device)
  PinBuf<uint8_t> h_ubs;     // its pinned staging
  DevBuf<uint8_t> d_enc;     // DL-SCH encode: descriptors, TB CRCs, unpacked e bits, staging
  DevBuf<uint8_t> d_ultx;    // UL-SCH transmit: descriptors, UCI bit lists, e / g / q bits, symbols
  DevBuf<short>   d_wide;    // llr_is_8bit, K <= 800: the widened soft buffers the 16-bit decoders read
  size_t      wide_cap = 0;  // rows of kWideStride in d_wide
};

// decode_tb of one TB, host-synchronous; LLRs from the host (e_bits) or already on the device (d_e_bits)
int dlsch_decode_sync(srsran_sch_t* q, srsran_pdsch_cfg_t* cfg, const int16_t* e_bits, const int16_t* d_e_bits,
                      uint8_t* data, int tb_idx, uint32_t nof_layers);

// encode_tb_off's split of the E bits over the blocks (sch.c:271-305); the K2 blocks come first.  Appends the TB's
// code block descriptors: c.e holds the byte offset e_off + (bits before the block) and c.tb_crc the TB index t, both
// fixed up once the scratch is allocated.  *wp: the E bits used.
typedef std::map<uint32_t, std::pair<const uint16_t*, uint32_t>> EncFwdMap;  // (cb_idx, rv) -> table, looked up once
int enc_push_cbs(std::vector<EncCb>& cb, EncFwdMap& fwd, const srsran_cbsegm_t& s, uint32_t Qm, uint32_t rv,
                 uint32_t nof_e_bits, const uint8_t* d_data, uint32_t tbs, size_t e_off, uint32_t t, uint32_t* wp_out);

}  // namespace srsran_amd
