// srsran_4g_amd/csrc/lte_seq_host.cpp -- the host Gold sequence of lte_seq_host.h (36.211 7.2, Nc = 1600).
#include "lte_seq_host.h"

namespace srsran_amd {
namespace {

// 31-bit registers, bit n of the state = x(n)
uint32_t step_x1(uint32_t s) { return (s >> 1) ^ (((s ^ (s >> 3)) & 1u) << 30); }
uint32_t step_x2(uint32_t s) { return (s >> 1) ^ (((s ^ (s >> 1) ^ (s >> 2) ^ (s >> 3)) & 1u) << 30); }

// The states after the 1600 warm-up steps: x1's is a constant, x2's is linear in c_init, so it is the
// xor of the columns of the set seed bits.
struct GoldJump {
  uint32_t x1;
  uint32_t col[31];
  GoldJump()
  {
    x1 = 1;
    for (int n = 0; n < 1600; n++) {
      x1 = step_x1(x1);
    }
    for (int b = 0; b < 31; b++) {
      uint32_t x2 = 1u << b;
      for (int n = 0; n < 1600; n++) {
        x2 = step_x2(x2);
      }
      col[b] = x2;
    }
  }
};

// calls emit(n, c(n)) for n = 0..len-1
template <class Emit>
void gold_run(uint32_t c_init, uint32_t len, Emit emit)
{
  static const GoldJump jump;
  uint32_t              x1 = jump.x1, x2 = 0;
  for (int b = 0; b < 31; b++) {  // bit 31 of c_init is not part of the seed
    if ((c_init >> b) & 1u) {
      x2 ^= jump.col[b];
    }
  }
  for (uint32_t n = 0; n < len; n++) {
    emit(n, (x1 ^ x2) & 1u);
    x1 = step_x1(x1);
    x2 = step_x2(x2);
  }
}

}  // namespace

void gold_bytes(uint32_t c_init, uint8_t* out, uint32_t len)
{
  gold_run(c_init, len, [out](uint32_t n, uint32_t c) { out[n] = (uint8_t)c; });
}

void gold_words(uint32_t c_init, uint32_t* out, uint32_t len)
{
  for (uint32_t w = 0; w < (len + 31) / 32; w++) {
    out[w] = 0;
  }
  gold_run(c_init, len, [out](uint32_t n, uint32_t c) { out[n >> 5] |= c << (n & 31); });
}

}  // namespace srsran_amd
