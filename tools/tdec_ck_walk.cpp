// tools/tdec_ck_walk.cpp -- host-only walk over the window-checkpoint scratch of the fused 16-step launches.
//
// For every 16-sub-block size K (816 .. 6144) and batches of 1, 4, 5 and 1024 blocks a size, lays the groups of
// one launch out as srsran_tdec_gpu_run_multi does (group after group, csrc/tdecs_ck_geo.h) and walks every
// (workgroup, wave, lane, window) access of tdecs_kernel.hip's GCK build:
//   * phase-1 stores: the forward wave windows [0, h), the backward wave [h, M) -- every 16-byte cell of the launch
//     is written by exactly one (group, workgroup, wave, lane, window): no overlap, no cell outside the buffer;
//   * phase-2 loads, the prefetched ones included (forward wave: h .. M-1 and min(m + 1, M - 1); backward wave:
//     h-1 .. 0 and max(m - 1, 0)): each inside the workgroup's own region, on a cell the OTHER wave of the same
//     lane wrote;
//   * the buffer resource of a workgroup (base, bytes) lies inside its group's part, and the parts inside the buffer.
// All 64 lanes are walked whatever the batch: the dead blocks of a partly filled last workgroup store too.
//
// Build and run (no GPU):  c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//                              -I srsran_4g_amd/csrc tools/tdec_ck_walk.cpp -o /tmp/tdec_ck_walk && /tmp/tdec_ck_walk
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tdecs_ck_geo.h"

using namespace srsran_amd;

namespace {
constexpr int W = 16, NSB = 16, CPWG = 64 / NSB;

std::vector<uint32_t> sizes16()
{
  std::vector<uint32_t> v;
  for (uint32_t K = 816; K <= 1024; K += 16) v.push_back(K);
  for (uint32_t K = 1056; K <= 2048; K += 32) v.push_back(K);
  for (uint32_t K = 2112; K <= 6144; K += 64) v.push_back(K);
  return v;
}

[[noreturn]] void fail(const char* what, uint32_t K, uint32_t ncb, uint32_t wg, int wave, int lane, int m)
{
  fprintf(stderr, "FAIL %s: K=%u batch=%u wg=%u wave=%d lane=%d window=%d\n", what, K, ncb, wg, wave, lane, m);
  exit(1);
}
}  // namespace

int main()
{
  const std::vector<uint32_t> Ks = sizes16();
  uint64_t                    cells_total = 0;
  for (uint32_t ncb : {1u, 4u, 5u, 1024u}) {
    // the launch's layout: group g at base[g], as the host hands it out
    std::vector<uint64_t> base(Ks.size()), bytes(Ks.size());
    uint64_t              total = 0;
    for (size_t g = 0; g < Ks.size(); g++) {
      base[g]  = total;
      bytes[g] = tdecs_ck_group_bytes(Ks[g] / NSB, (ncb + CPWG - 1) / CPWG);
      total += bytes[g];
    }
    if (total % TDECS_CK_STATE) fail("buffer size not a multiple of a checkpoint", 0, ncb, 0, 0, 0, 0);
    std::vector<uint8_t> owner(total / TDECS_CK_STATE, 0);  // 0 free, 1 forward wave's, 2 backward wave's
    for (size_t g = 0; g < Ks.size(); g++) {
      const uint32_t K = Ks[g], L = K / NSB, nwg = (ncb + CPWG - 1) / CPWG;
      const int      M = (int)tdecs_ck_windows(L);
      const int      h = std::max(1, std::min((int)(L + 2 * W - 1) / (2 * W), (int)L / W));
      if (M != (int)((L + W - 1) / W) || h >= M) fail("window count / crossover", K, ncb, 0, 0, 0, M);
      for (uint32_t wg = 0; wg < nwg; wg++) {
        const uint64_t off   = tdecs_ck_wg_off(L, wg);
        const uint32_t avail = tdecs_ck_wg_avail(L, wg, bytes[g]);  // the buffer resource: [base + off, + avail)
        if (off + avail > bytes[g] || base[g] + off + avail > total) fail("resource outside its group", K, ncb, wg, 0, 0, 0);
        if (avail != tdecs_ck_wg_bytes(L)) fail("region clipped", K, ncb, wg, 0, 0, 0);
        auto cell = [&](int wave, int lane, int m) -> uint64_t {
          const uint64_t a = (uint64_t)tdecs_ck_row(m) + tdecs_ck_lane((uint32_t)lane);
          if (a + TDECS_CK_STATE > avail) fail("access outside the workgroup's region", K, ncb, wg, wave, lane, m);
          if (a % TDECS_CK_STATE) fail("misaligned access", K, ncb, wg, wave, lane, m);
          return (base[g] + off + a) / TDECS_CK_STATE;
        };
        for (int lane = 0; lane < (int)TDECS_CK_LANES; lane++) {
          for (int m = 0; m < M; m++) {  // phase 1
            const int      wave = m < h ? 0 : 1;
            const uint64_t c    = cell(wave, lane, m);
            if (owner[c]) fail("cell written twice", K, ncb, wg, wave, lane, m);
            owner[c] = (uint8_t)(1 + wave);
            cells_total++;
          }
          for (int m = h; m < M; m++) {  // phase 2, forward wave: its window and the one prefetched
            for (int mm : {m, std::min(m + 1, M - 1)}) {
              if (owner[cell(0, lane, mm)] != 2) fail("forward wave loads a cell the backward wave did not write", K, ncb, wg, 0, lane, mm);
            }
          }
          for (int m = h - 1; m >= 0; m--) {  // phase 2, backward wave
            for (int mm : {m, std::max(m - 1, 0)}) {
              if (owner[cell(1, lane, mm)] != 1) fail("backward wave loads a cell the forward wave did not write", K, ncb, wg, 1, lane, mm);
            }
          }
        }
      }
    }
    for (uint8_t o : owner) {
      if (!o) fail("cell of the buffer that no workgroup owns", 0, ncb, 0, 0, 0, 0);
    }
    printf("batch %4u: %zu sizes, %.1f MB of scratch, every cell owned once\n", ncb, Ks.size(), (double)total / 1e6);
  }
  printf("ok: %llu checkpoint cells walked\n", (unsigned long long)cells_total);
  return 0;
}
