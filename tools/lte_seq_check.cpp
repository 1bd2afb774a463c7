// tools/lte_seq_check.cpp -- host-only check of csrc/lte_seq_host.cpp, the library's one host Gold sequence.
//
// For every (seed, length) prints one line "seed length bits words": gold_bytes' output as a string of 0 / 1 and
// gold_words' output as 8 hex digits a word, after checking that the two agree bit for bit, that gold_words leaves
// the last word's bits from `length` on zero and that neither writes past its output (guard values here, the
// sanitizers' red zones on the heap blocks).  tests/test_lte_seq_host.py compares the printed bits with the oracle.
//
// Build and run (no GPU):  c++ -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//                              tools/lte_seq_check.cpp srsran_4g_amd/csrc/lte_seq_host.cpp -o /tmp/lte_seq_check && /tmp/lte_seq_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../srsran_4g_amd/csrc/lte_seq_host.h"

using namespace srsran_amd;

namespace {

[[noreturn]] void fail(const char* what, uint32_t seed, uint32_t len, uint32_t n)
{
  fprintf(stderr, "FAIL %s: seed=%u len=%u n=%u\n", what, seed, len, n);
  exit(1);
}

void run(uint32_t seed, uint32_t len, bool print)
{
  const uint32_t        nw = (len + 31) / 32;
  std::vector<uint8_t>  b(len + 1, 0xA5);  // one guard element each
  std::vector<uint32_t> w(nw + 1, 0xDEADBEEFu);
  gold_bytes(seed, b.data(), len);
  gold_words(seed, w.data(), len);
  if (b[len] != 0xA5 || w[nw] != 0xDEADBEEFu) {
    fail("write past the output", seed, len, len);
  }
  for (uint32_t n = 0; n < 32 * nw; n++) {
    const uint32_t bit = (w[n >> 5] >> (n & 31)) & 1u;
    if (n < len ? (b[n] > 1 || bit != b[n]) : bit != 0) {
      fail(n < len ? "gold_bytes and gold_words differ" : "gold_words sets a bit past the length", seed, len, n);
    }
  }
  if (!print) {
    return;
  }
  printf("%u %u ", seed, len);
  for (uint32_t n = 0; n < len; n++) {
    putchar('0' + b[n]);
  }
  putchar(' ');
  for (uint32_t k = 0; k < nw; k++) {
    printf("%08x", w[k]);
  }
  putchar('\n');
}

}  // namespace

int main()
{
  const uint32_t id = 503, rnti = 0xFFFF;  // the largest cell id and RNTI: each formula's largest seed
  const uint32_t seeds[] = {
      0,
      1,
      1u << 30,
      0x7FFFFFFFu,
      ((id / 30) << 5) + (((id % 30) + 29) % 30),           // hopping_tables: n_PN / sequence hopping, delta_ss = 29
      id / 30,                                              // f_gh
      id,                                                   // PUCCH n_cs_cell, PBCH
      ((9 + 1) * (2 * id + 1) << 16) + rnti,                // PUCCH scrambling, subframe 9
      512 * (7 * (19 + 1) + 4 + 1) * (2 * 255 + 1) + 255,   // MBSFN reference signal: slot 19, l' = 4, area 255
      1024 * (7 * (19 + 1) + 4 + 1) * (2 * id + 1) + 2 * id + 1,  // CRS: slot 19, symbol 4, normal CP
      (9 + 1) * (2 * id + 1) * 512 + id,                    // PCFICH / PHICH, subframe 9
      9 * 512 + id,                                         // PDCCH, subframe 9
  };
  const uint32_t lens[] = {1, 31, 32, 33, 48, 1920, 2200};
  for (uint32_t seed : seeds) {
    for (uint32_t len : lens) {
      run(seed, len, true);
    }
  }
  // bit 31 of the seed is not part of it
  std::vector<uint8_t> a(2200), b(2200);
  gold_bytes(0x7FFFFFFFu, a.data(), 2200);
  gold_bytes(0xFFFFFFFFu, b.data(), 2200);
  if (a != b) {
    fail("bit 31 of the seed changes the sequence", 0xFFFFFFFFu, 2200, 0);
  }
  run(0x80000001u, 2200, false);
  return 0;
}
