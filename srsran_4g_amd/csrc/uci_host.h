// srsran_4g_amd/csrc/uci_host.h -- the host arithmetic of UCI on PUSCH (uci_host.cpp) that the UL-SCH units call:
// the offset tables, Q', the interleaver's RI / ACK columns and the transmitter's UCI channel coding.  No HIP here:
// uci_host.cpp and fec_host.cpp build with a plain C++ compiler (tools/sch_host_check.cpp runs them under sanitizers).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/srsran_sch.h"

namespace srsran_amd {

// Offset tables of 36.213 Tables 8.6.3-1/-2/-3 with the reference's out-of-range behaviour
// (sch.c:43-95: an error message and the first valid entry).
float beta_harq(uint32_t i);
float beta_ri(uint32_t i);
float beta_cqi(uint32_t i);

// Q'_ACK / Q'_RI, 36.212 5.2.2.6 (uci.c:414-440); float arithmetic in the reference's order
uint32_t qprime_ri_ack(uint32_t K, uint32_t L_prb, uint32_t nof_symb, uint32_t O, uint32_t O_cqi, float beta);
// the same for O bits of a PUSCH whose K_segm is set, from the bits' own offset: without a TB the offset is taken
// relative to the CQI's (36.212 5.2.4.1; sch.c:1046-1049, 1248-1251)
uint32_t qprime_ri_ack_cfg(const srsran_pusch_cfg_t* cfg, bool no_tb, uint32_t nof_symb, uint32_t O, uint32_t O_cqi,
                           float beta);
// Q'_CQI (uci.c:170-186)
uint32_t qprime_cqi(uint32_t K, uint32_t L_prb, uint32_t nof_symb, uint32_t O, float beta, uint32_t Q_prime_ri);

// The interleaver columns that carry RI (uci.c:397-398) and HARQ-ACK (uci.c:370-371) with nof_symb data symbols a
// subframe (normal / extended CP): four of them, RI / ACK symbol i in column set[(3 i) mod 4]
const uint8_t* uci_ri_cols(uint32_t nof_symb);
const uint8_t* uci_ack_cols(uint32_t nof_symb);

// bit types of the RI / ACK lists (uci.h's srsran_uci_bit_type_t), as pusch_tx_kernel.h's TX_BIT_*
enum : uint8_t { UCI_BIT_0 = 0, UCI_BIT_1 = 1, UCI_BIT_REPETITION = 2, UCI_BIT_PLACEHOLDER = 3 };

// srsran_block_encode (block.c:78-104): the codeword of the first 11 input bits, repeated up to nout bits
void block_encode(const uint8_t* in, uint32_t nin, uint8_t* out, uint32_t nout);
// encode_cqi_long (uci.c:225-257): CRC8 (0x19B), the tail-biting rate-1/3 code (0x6D, 0x4F, 0x57, K = 7;
// convcoder.c:43-69) and srsran_rm_conv_tx (rm_conv.c:43-88) to Q bits
bool cqi_encode_long(const uint8_t* data, uint32_t nbits, uint8_t* out, uint32_t Q);
// encode_ri_ack / encode_ack_long and the repetition of srsran_uci_encode_ack_ri (uci.c:457-510, 600-613): the type
// of every bit of the Q' symbols
void ri_ack_types(const uint8_t* data, uint32_t O, uint32_t Qm, uint32_t Qp, std::vector<uint8_t>& t);
// uci_ack_scramble_tdd (uci.c:548-579)
void ack_scramble_tdd(std::vector<uint8_t>& q, uint32_t O_ack, uint32_t N_bundle);

}  // namespace srsran_amd
