// srsran_4g_amd/csrc/lte_seq_host.h -- the LTE Gold sequence c(n) of 36.211 7.2 (srsran_sequence_LTE_pr, sequence.c)
// on the host, for every unit that builds a scrambling or reference-signal table there.  Plain C++: no HIP include.
// The device side (seq_mod_dev.h, llr_kernel.hip) has its own tables.
#pragma once
#include <stdint.h>

namespace srsran_amd {

// c(0..len-1) of c_init, one byte per bit.  Only the low 31 bits of c_init seed x2 (a 31-bit register): the rest is
// masked here.
void gold_bytes(uint32_t c_init, uint8_t* out, uint32_t len);

// The same bits packed: bit n & 31 of out[n >> 5] is c(n).  Writes (len + 31) / 32 words; the bits from len on are 0.
void gold_words(uint32_t c_init, uint32_t* out, uint32_t len);

}  // namespace srsran_amd
