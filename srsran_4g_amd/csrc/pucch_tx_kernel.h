// srsran_4g_amd/csrc/pucch_tx_kernel.h -- launch interface of the PUCCH transmit kernel (UE side, formats
// 1/1a/1b/2/2a/2b/3): bits to symbols, the data symbols of pucch.c:136-203, 374-504, the DMRS of
// refsignal_ul.c:432-512 and the mapping of pucch.c:321-367 / refsignal_ul.c:514-552 for every
// transmission of a batch in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pucch_kernel.h"

namespace srsran_amd {

// One PUCCH transmission; mirrors PucchCand.  The host gives phi(n) of each slot's group, n_cs and the cover
// argument per slot and symbol, the coded bits and the scrambling bits; the device forms the modulation symbols,
// the sequences (the single-precision argument phi(n) pi / 4 + alpha n, one rounding, accurate sine / cosine),
// the format 3 spreading and DFT, and writes the REs.
struct PucchTxUe {
  float2*  grid;        // subframe grid of the cell, 2 nsym_slot x ncell_re, or nullptr
  float2*  z_out;       // optional: the data symbols in pucch.c's z order, (n_sf[0] + n_sf[1]) x 12
  float2*  r_out;       // optional: the DMRS in refsignal_ul.c's r_pucch order, 2 n_rs x 12
  uint32_t zero_rest;   // grid: 1: every RE that is not a PUCCH RE of this transmission is zeroed
  uint32_t ncell_re;    // 12 * cell PRBs
  uint32_t nsym_slot;   // 7 / 6
  uint32_t format;      // srsran_pucch_format_t
  uint32_t n_prb[2];
  uint32_t n_rs;        // DMRS symbols per slot
  uint32_t n_sf[2];     // data symbols per slot
  int8_t   phi[2][12];                 // phi(n) of the slot's base sequence group u
  uint8_t  rs_sym[PUCCH_MAX_RS];       // symbol index within the slot
  uint8_t  data_sym[PUCCH_MAX_SF];
  uint8_t  rs_ncs[2][PUCCH_MAX_RS];    // n_cs per slot and DMRS symbol
  uint8_t  data_ncs[2][PUCCH_MAX_SF];  // format 1x / 2x: n_cs; format 3: n_cs_cell(ns, l)
  float    rs_warg[2][PUCCH_MAX_RS];   // argument of w-bar(m), as the reference holds it in single precision
  float    data_warg[2][PUCCH_MAX_SF]; // format 1x: argument of w_n_oc(m) plus S(ns)
  uint8_t  f3_noc[2];                  // format 3: n_oc of each slot
  uint8_t  drs[2];                     // 2a / 2b: the bits of d(10)
  uint64_t bits;  // bit i: b(i); format 1a / 1b the 1 / 2 HARQ-ACK bits, 2x the 20, 3 the 48 coded bits
  uint64_t scr;   // the first 48 bits of the format 2x / 3 scrambling sequence
};

// The value of RE n of data symbol i (is_rs false) or DMRS symbol i (is_rs true) of slot s: what a lane of the
// kernel computes, also callable on the host (srsran_refsignal_dmrs_pucch_gen_cell has no device object).
__host__ __device__ float2 pucch_tx_re(const PucchTxUe& u, uint32_t s, bool is_rs, uint32_t i, uint32_t n);

// one workgroup per (grid symbol, transmission); every pointer of a descriptor is device memory
hipError_t pucch_tx_launch(const PucchTxUe* d_ues, uint32_t nue, hipStream_t stream);

}  // namespace srsran_amd
