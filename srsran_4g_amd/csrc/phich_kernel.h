// srsran_4g_amd/csrc/phich_kernel.h -- PHICH transmit / receive kernels (phich_kernel.hip), host interface.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srsran_amd {

// One PHICH resource of a batch (device copy of srsran_phich_gpu_item_t, with what the host derived).
struct PhichItem {
  uint32_t sf;    // subframe in the batch's grids
  uint32_t unit;  // mapping unit: ngroup, or ngroup / 2 with the extended CP
  uint32_t half;  // extended CP: ngroup % 2 (which symbol pair of every REG carries the group)
  uint32_t nseq;
  uint32_t seq;   // bit m: srsran_sequence_phich bit of symbol m (12 bits)
  uint32_t ack;
};

// A (subframe, mapping unit) that has items: items[first .. first + count), in put order.
struct PhichUnit {
  uint32_t sf, unit, first, count;
};

struct PhichTxArgs {
  const PhichItem* items;
  const PhichUnit* units;
  const uint32_t*  re;     // 12 grid indices per mapping unit
  float2*          grids;  // [sf][port][sf_re]
  uint32_t         nports, sf_re, ext_cp;
};

struct PhichOut {  // srsran_phich_gpu_res_t
  uint32_t ack;
  float    distance;
};

struct PhichRxArgs {
  const PhichItem* items;
  const uint32_t*  re;
  const float2*    grids;  // [sf][rx][sf_re]
  const float2*    ce;     // [sf][port][rx][ce_row], read at grid index % ce_row
  const float*     noise;  // subframe s: noise[s * noise_stride]
  PhichOut*        out;    // one per item
  uint32_t         nports, nrx, sf_re, ce_row, noise_stride, ext_cp;
};

hipError_t phich_tx_launch(const PhichTxArgs& a, uint32_t nunits, hipStream_t stream);
hipError_t phich_rx_launch(const PhichRxArgs& a, uint32_t nitems, hipStream_t stream);

}  // namespace srsran_amd
