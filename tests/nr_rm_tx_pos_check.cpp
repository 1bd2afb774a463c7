// Host check of csrc/nr_rm_tx_pos.h (CPU only, built under ASan + UBSan by tests/test_nr_sch_tx_host.py):
// the closed forms the transmit kernels use against the reference's sequential definitions written out as
// loops -- the bit_selection_rm_tx walk over a byte buffer with filler bytes (ldpc_rm.c:173-193), the bit
// interleaver (ldpc_rm.c:348-360), k0 / Ncb (ldpc_rm.c:126-164) and sch_nr_get_E with the running output
// offset (sch_nr.c:178-189, 534-548).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nr_rm_tx_pos.h"

using namespace srsran_amd;

static const uint8_t  FILLER       = 254;
static const uint32_t BASEK0[4][2] = {{0, 0}, {17, 13}, {33, 25}, {56, 43}};

static long g_checks = 0;

#define CHECK(c, ...)                                                                                                  \
  do {                                                                                                                 \
    if (!(c)) {                                                                                                        \
      fprintf(stderr, "FAILED %s:%d: " #c " -- ", __FILE__, __LINE__);                                                 \
      fprintf(stderr, __VA_ARGS__);                                                                                    \
      fprintf(stderr, "\n");                                                                                           \
      exit(1);                                                                                                         \
    }                                                                                                                  \
    g_checks++;                                                                                                        \
  } while (0)

// srsran_ldpc_rm_tx as the reference runs it
static std::vector<uint8_t> walk(const std::vector<uint8_t>& cw, uint32_t E, uint32_t Qm, uint32_t k0, uint32_t Ncb)
{
  std::vector<uint8_t> sel(E), out(E);
  uint32_t             k = 0, j = 0;
  while (k < E) {
    const uint32_t icwd = (k0 + j) % Ncb;
    if (cw[icwd] != FILLER) {
      sel[k] = cw[icwd];
      k++;
    }
    j++;
  }
  if (Qm == 1) {
    return sel;
  }
  const uint32_t cols = E / Qm;
  for (uint32_t c = 0; c < cols; c++) {
    for (uint32_t i = 0; i < Qm; i++) {
      out[i + c * Qm] = sel[i * cols + c];
    }
  }
  return out;
}

static void check_rm(uint32_t bg, uint32_t Z, uint32_t rv, uint32_t Nref, uint32_t F)
{
  const uint32_t N = Z * (bg == 0 ? 66u : 50u), Kr2 = Z * (bg == 0 ? 22u : 10u) - 2 * Z;
  const uint32_t ini = Kr2 - F, end = Kr2;
  uint32_t       k0, Ncb;
  nr_rm_tx_k0_ncb(bg, Z, rv, Nref, &k0, &Ncb);
  const uint32_t want_ncb = N <= Nref ? N : Nref;
  const uint32_t want_k0  = N <= Nref ? Z * BASEK0[rv][bg] : Z * ((BASEK0[rv][bg] * Nref) / N);
  CHECK(k0 == want_k0 && Ncb == want_ncb, "bg %u Z %u rv %u Nref %u", bg, Z, rv, Nref);
  std::vector<uint8_t> cw(N);
  for (uint32_t p = 0; p < N; p++) {
    cw[p] = (p >= ini && p < end) ? FILLER : (uint8_t)(p % 251u);
  }
  const NrRmTxSel sel = nr_rm_tx_sel(k0, Ncb, ini, end);
  uint32_t        L   = 0;
  for (uint32_t p = 0; p < Ncb; p++) {
    L += cw[p] != FILLER;
  }
  CHECK(sel.L == L && L > 0, "L %u vs %u", sel.L, L);
  static const uint32_t QM[5] = {1, 2, 4, 6, 8};
  for (uint32_t Qm : QM) {
    const uint32_t es[5] = {Qm, L - Qm, L, L + Qm, 3 * L + Qm};
    for (uint32_t e : es) {
      const uint32_t E = e > 4u * N ? 0u : e / Qm * Qm;  // L - Qm wrapped below zero: skip
      if (E == 0) {
        continue;
      }
      const std::vector<uint8_t> want = walk(cw, E, Qm, k0, Ncb);
      const uint32_t             cols = E / Qm;
      for (uint32_t t = 0; t < E; t++) {
        const uint32_t j = t / Qm, i = t % Qm;
        const uint32_t k = Qm == 1 ? t : nr_rm_tx_il(j, i, cols);
        const uint32_t p = nr_rm_tx_pos(sel, k % L);
        CHECK(p < Ncb && cw[p] == want[t], "bg %u Z %u rv %u Nref %u F %u Qm %u E %u t %u: position %u", bg, Z, rv,
              Nref, F, Qm, E, t, p);
      }
    }
  }
}

// sch_nr_get_E (sch_nr.c:178-189)
static uint32_t ref_E(uint32_t G, uint32_t Nl, uint32_t Qm, uint32_t Cp, uint32_t j)
{
  if (j <= (Cp - (G / (Nl * Qm)) % Cp - 1)) {
    return Nl * Qm * (G / (Nl * Qm * Cp));
  }
  return Nl * Qm * ((G + Nl * Qm * Cp - 1) / (Nl * Qm * Cp));
}

int main()
{
  static const uint32_t ZS[4] = {2, 7, 20, 384};
  for (uint32_t bg = 0; bg < 2; bg++) {
    for (uint32_t Z : ZS) {
      const uint32_t N = Z * (bg == 0 ? 66u : 50u), Kr2 = Z * (bg == 0 ? 22u : 10u) - 2 * Z;
      const uint32_t FS[3] = {0, 8, 2 * Z - 1};
      for (uint32_t F : FS) {
        // the whole buffer, 0.6 N, just above the filler range, inside the filler range
        const uint32_t NREF[4] = {N, (uint32_t)(0.6 * N), Kr2 + 1, Kr2 - F / 2};
        for (uint32_t Nref : NREF) {
          for (uint32_t rv = 0; rv < 4; rv++) {
            check_rm(bg, Z, rv, Nref, F);
          }
        }
      }
    }
  }
  static const uint32_t NRE[6] = {24, 100, 1200, 2501, 8113, 42588};
  static const uint32_t QM[5]  = {1, 2, 4, 6, 8};
  for (uint32_t nre : NRE) {
    for (uint32_t Qm : QM) {
      for (uint32_t Nl = 1; Nl <= 4; Nl++) {
        for (uint32_t Cp = 1; Cp <= 41; Cp++) {
          const uint32_t G   = nre * Qm * Nl;
          const NrSchE   e   = nr_sch_E(G, Nl, Qm, Cp);
          uint32_t       off = 0;
          for (uint32_t j = 0; j < Cp; j++) {
            CHECK(nr_sch_E_of(e, j) == ref_E(G, Nl, Qm, Cp, j) && nr_sch_E_offset(e, j) == off,
                  "G %u Nl %u Qm %u Cp %u j %u", G, Nl, Qm, Cp, j);
            off += ref_E(G, Nl, Qm, Cp, j);
          }
          CHECK(nr_sch_E_offset(e, Cp) == off && off <= G, "G %u Nl %u Qm %u Cp %u: total %u", G, Nl, Qm, Cp, off);
        }
      }
    }
  }
  printf("nr_rm_tx_pos OK: %ld checks\n", g_checks);
  return 0;
}
