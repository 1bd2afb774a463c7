// srsran_4g_amd/csrc/pucch_kernel.h -- launch interface of the PUCCH receive kernel (formats
// 1/1a/1b/2/2a/2b/3): srsran_chest_ul_estimate_pucch + srsran_pucch_decode for every candidate
// (resource, hypothesis pass) of every UE in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srsran_amd {

static constexpr uint32_t PUCCH_MAX_RS = 3;    // DMRS symbols of a slot
static constexpr uint32_t PUCCH_MAX_SF = 5;    // data symbols of a slot
static constexpr uint32_t PUCCH_MAX_RE = 120;  // SRSRAN_PUCCH_MAX_SYMBOLS

// Every reference value of PUCCH is a 24th root of unity: r_u,v(alpha)(n) = exp(j pi (3 phi(n) +
// 2 n_cs n) / 12), and the orthogonal covers, S(ns) and d(10) are multiples of pi / 6.  The host
// gives phi(n) of the slot's group, n_cs and the cover phase (units of pi / 12) per symbol; the
// device builds the sequences from them.
struct PucchCand {
  // compact == 0: the device subframe grid of the cell.  compact == 1 (decode only): the gathered
  // data REs (pucch_get order) and, in ce_in, the channel estimates at the same REs.
  const float2* grid;
  const float2* ce_in;
  float2*       ce;         // estimate grid to fill (both slots' PRBs, all symbols) or nullptr
  uint32_t      compact;
  uint32_t      do_decode;  // 0: estimate only
  uint32_t      ncell_re;   // 12 * cell PRBs
  uint32_t      nsym_slot;  // 7 / 6
  uint32_t      format;     // srsran_pucch_format_t
  uint32_t      n_prb[2];
  uint32_t      n_rs;       // DMRS symbols per slot
  uint32_t      n_sf[2];    // data symbols per slot
  int8_t        phi[2][12];                 // phi(n) of the slot's base sequence group u
  uint8_t       rs_sym[PUCCH_MAX_RS];       // symbol index within the slot
  uint8_t       data_sym[PUCCH_MAX_SF];
  uint8_t       rs_ncs[2][PUCCH_MAX_RS];    // n_cs per slot and DMRS symbol
  uint8_t       rs_ph[2][PUCCH_MAX_RS];     // w-bar phase, units of pi / 12 (without d(10))
  uint8_t       data_ncs[2][PUCCH_MAX_SF];  // format 1x / 2x: n_cs; format 3: n_cs_cell(ns, l)
  uint8_t       data_ph[2][PUCCH_MAX_SF];   // format 1x: w_n_oc + S(ns), units of pi / 12
  uint8_t       f3_noc[2];                  // format 3: n_oc of each slot
  uint64_t      scr;           // the first 48 bits of the format 2x / 3 scrambling sequence
  uint32_t      nof_uci_bits;  // A of the (20, A) code
  float         thr_format1, thr_format3, thr_dmrs;
  float         noise_in;      // compact: the estimator's noise_estimate
  float         filt[3];       // 3-tap smoothing filter
  double        noise_div;     // a * 0.8 of estimate_noise_pilots_pucch
  uint32_t      meas_ta;
};

struct PucchCandOut {
  float    epre, rsrp, noise, ta_us;
  float    corr, dmrs_corr;
  uint32_t dmrs_checked;  // DMRS detection ran
  uint32_t dmrs_failed;   // ... and returned early (correlation 0, not detected, no UCI written)
  uint32_t found;         // decode_signal's return
  uint8_t  drs_bits[2];   // 2a / 2b DMRS hypothesis
  uint8_t  bits[16];      // pucch_bits (format 2x: the 13 bits of the codeword index, MSB first)
};

// one 64-lane workgroup per candidate
hipError_t pucch_launch(const PucchCand* d_cand, PucchCandOut* d_out, uint32_t ncand, hipStream_t stream);

}  // namespace srsran_amd
