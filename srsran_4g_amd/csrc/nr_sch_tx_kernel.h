// srsran_4g_amd/csrc/nr_sch_tx_kernel.h -- NR SCH transmit kernels: TB CRC and the fused code-block
// encoder (segmentation, CRC attachment, LDPC encoding, rate matching).
#ifndef SRSRAN_AMD_NR_SCH_TX_KERNEL_H
#define SRSRAN_AMD_NR_SCH_TX_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nr_rm_tx_pos.h"
#include "nr_tb_crc.h"

namespace srsran_amd {

// One TB's CRC over its payload (sch_nr.c:465).
struct NrTxTb {
  const uint8_t* payload;  // nbytes = tbs / 8 (device)
  uint32_t*      crc;      // accumulator, zero before the launch; afterwards the CRC of L_tb bits
  uint32_t       nbytes;
  uint32_t       L_tb;     // 24: CRC24A, 16: CRC16
};

// One code block (sch_nr.c:473-549): payload bits -> e_bits.
struct NrTxCb {
  const uint8_t*  payload;   // the TB's payload (device)
  uint8_t*        e;         // where the block's E rate-matched bits go, one per byte (device)
  const uint32_t* tb_crc;    // the TB's CRC accumulator (read by the last block)
  const uint32_t* sh;        // V mod Z per edge of (bg, Z) (device)
  uint64_t        inv_L;     // ceil(2^40 / sel.L): k / L for k < 2^21
  uint32_t        byte0;     // first payload byte of the block
  uint32_t        data_bytes;  // payload bytes the block carries
  uint32_t        L_tb;      // TB CRC bits behind them (the last block), else 0
  uint32_t        L_cb;      // 24: CRC24B behind that, else 0
  uint32_t        E, Qm;
  uint32_t        magic_ls;  // ceil(2^32 / Z)
  uint16_t        Z;
  uint16_t        n_rows;    // base-graph rows the transmitted span needs
  uint8_t         bg, hr_case;
  NrRmTxSel       sel;       // fillers at [Kp - 2Z, Kr - 2Z)
};

// slices = max over the TBs of ceil(nbytes / NR_TB_SLICE), at most NR_TB_MAX_SLICES
hipError_t nr_tb_crc_launch(const NrTxTb* d_tbs, uint32_t ntb, uint32_t slices, hipStream_t stream);
// xpow24b: x^n mod CRC24B, n = 0 .. 8448 (device); max_ls: the largest Z among the blocks
hipError_t nr_tx_cb_launch(const NrTxCb* d_cbs, uint32_t ncb, const uint32_t* xpow24b, uint32_t max_ls,
                           hipStream_t stream);

}  // namespace srsran_amd
#endif
