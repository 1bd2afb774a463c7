// srsran_4g_amd/csrc/pusch_tx_kernel.h -- launch interface of the PUSCH transmit kernels (UE side):
// UL-SCH / UCI multiplexing, channel interleaver, scrambling and mapping (sch.c:661-991, 1278-1333,
// pusch.c:299-334), transform precoding with RE mapping and DMRS insertion (dft_precoding.c:114-126,
// pusch.c:48-95, refsignal_ul.c:194-225) and the subframe normalisation (ue_ul.c:246-299).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pusch_kernel.h"

namespace srsran_amd {

// bit types of the RI / ACK lists (uci.h's srsran_uci_bit_type_t)
enum : uint8_t { TX_BIT_0 = 0, TX_BIT_1 = 1, TX_BIT_REPETITION = 2, TX_BIT_PLACEHOLDER = 3 };

static constexpr uint32_t PUSCH_TX_SYM_PER_THREAD = 4;  // 4 Qm bits = Qm / 2 whole bytes of q for every Qm

// One PUSCH transmission.  Bit buffers hold one bit a byte unless "packed" (MSB first).
struct PuschTxUe {
  // ---- multiplexing, interleaving, scrambling, mapping
  const uint8_t* cqi;      // ncqi coded CQI bits (the head of g)
  const uint8_t* e;        // ne rate-matched UL-SCH bits (the rest of g); nullptr without a TB
  const uint8_t* ri;       // types of the Q'_RI symbols' bits, Qm each, in the order uci.c generates them
  const uint8_t* ack;      // types of the Q'_ACK symbols' bits
  uint8_t*       g_pack;   // out (optional): packed g bits, ceil((ncqi + ne) / 8) bytes
  uint8_t*       q_pack;   // out (optional): packed q bits before scrambling, H Qm / 8 bytes
  uint8_t*       s_pack;   // out (optional): packed q bits after scrambling and the placeholder rule
  float2*        d;        // out: H modulation symbols
  uint32_t       seed;     // scrambling c_init (sequences.c:119-122)
  uint32_t       mod;      // srsran_mod_t: 1 QPSK, 2 16QAM, 3 64QAM
  uint32_t       Qm;
  uint32_t       rows, cols, H;  // interleaver: cols = N_symb, rows = M_sc, H = rows cols
  uint32_t       ncqi, ne;
  uint32_t       ri_Qp, ack_Qp;
  uint8_t        ri_col[4], ack_col[4];  // column sets, indexed by (3 i) mod 4 of RI / ACK symbol i
  // ---- transform precoding, mapping, DMRS (grid == nullptr: stage skipped for this entry)
  float2*        grid;      // subframe grid of the cell, 2 nsym_slot x ncell_re
  const float2*  dmrs;      // 2 M values (slot 0, slot 1)
  uint32_t       ncell_re;  // 12 cell nof_prb
  uint32_t       M;         // 12 L_prb
  uint32_t       nsym_slot;
  uint32_t       n_tilde[2];
  uint32_t       nof_symb;  // data symbols
  uint8_t        data_sym[14];
  uint8_t        radix[PUSCH_MAX_STAGES];
  uint32_t       nstages;
  float          dft_norm;
  uint32_t       put_dmrs;  // 1: the two DMRS symbols are written
  uint32_t       zero_rest; // 1: every RE outside the grant's data / DMRS REs is zeroed, else left untouched
  // ---- normalisation (samples_in == nullptr: stage skipped for this entry)
  const float2*  samples_in;
  float2*        samples_out;
  uint32_t       sf_len;
  uint32_t       norm_mode;   // 0 AUTO, 1 FORCE_AMPLITUDE
  float          norm_factor; // AUTO: the starting factor
  float          force_peak;  // FORCE_AMPLITUDE: the peak to reach (> 0)
};

// one thread per PUSCH_TX_SYM_PER_THREAD modulation symbols of every entry; max_H = largest H
hipError_t pusch_tx_mux_launch(const PuschTxUe* d_ues, uint32_t nue, uint32_t max_H, hipStream_t stream);
// one workgroup per (grid symbol, entry)
hipError_t pusch_tx_grid_launch(const PuschTxUe* d_ues, uint32_t nue, hipStream_t stream);
// one workgroup per entry: peak of |re|, |im| over the subframe, then the scale
hipError_t pusch_tx_norm_launch(const PuschTxUe* d_ues, uint32_t nue, hipStream_t stream);

}  // namespace srsran_amd
