// srsran_4g_amd/csrc/srs_kernel.h -- launch interface of the sounding reference signal kernels.  UE side: r_srs(i) of
// 36.211 5.5.3.1 formed on the device and mapped to the comb of the subframe's last symbol (refsignal_ul.c:870-906),
// for every SRS-carrying transmission of a batch in one launch.  eNB side: srsran_chest_ul_estimate_srs
// (chest_ul.c:298-396, 612-647) for many UEs in one launch, with the same sequence function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pusch_kernel.h"

namespace srsran_amd {

static constexpr uint32_t SRS_MAX_M_SC = 576;  // m_SRS = 96 PRB: 96 * 12 / 2

// The base sequence of one SRS: what zc_sequence.c:214-241, 282 needs.  n_zc == 0: the phi table of M_sc = 24
// (phi holds the row of group u); otherwise the Zadoff-Chu branch with the root q as the reference holds it, in
// single precision.  alpha: 2 pi n_srs / 8 rounded to single precision (refsignal_ul.c:882).
struct SrsSeq {
  uint32_t n_zc;
  float    q;
  float    alpha;
  int8_t   phi[24];
};

// One SRS transmission.  The host gives the sequence parameters, the comb start k0 (hopping applied,
// refsignal_ul.c:805-825) and M_sc; the device forms the M_sc values and stores them to
// grid[(nsym - 1) ncell_re + k0 + 2 i].
struct SrsTxUe {
  float2*  grid;       // subframe grid of the cell, nsym x ncell_re
  uint32_t ncell_re;   // 12 * cell PRBs
  uint32_t nsym;       // symbols of the subframe: 14 / 12
  uint32_t zero_rest;  // 1: every RE that is not an SRS RE of this transmission is zeroed (the SRS-only subframe)
  uint32_t k0;
  uint32_t m_sc;
  SrsSeq   seq;
};

// one workgroup per transmission; every pointer of a descriptor is device memory
hipError_t srs_tx_launch(const SrsTxUe* d_ues, uint32_t nue, hipStream_t stream);

// One SRS estimate.  grid: the received subframe grid of the cell; ce: where the M_sc smoothed (or copied) estimates
// go, contiguously (the caller points it at symbol L(0, cp), subcarrier 0 of the estimate grid, chest_ul.c:347-364),
// or nullptr; out: noise, ta_us, rsrp, epre (cfo_hz = NAN, data_pow = 0).
struct SrsRxUe {
  const float2* grid;
  float2*       ce;
  ChestUlOut*   out;
  uint32_t      ncell_re;
  uint32_t      nsym;
  uint32_t      k0;
  uint32_t      m_sc;      // <= SRS_MAX_M_SC
  int32_t       smooth;    // smooth_filter_len == 3
  float         filt[3];
  double        noise_div; // a * 0.8 of estimate_noise_pilots (chest_ul.c:220-225)
  SrsSeq        seq;       // the known sequence
};

// one workgroup per estimate; every pointer of a descriptor is device memory
hipError_t srs_chest_launch(const SrsRxUe* d_ues, uint32_t nue, hipStream_t stream);

}  // namespace srsran_amd
