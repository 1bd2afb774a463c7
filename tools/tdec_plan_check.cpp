// tools/tdec_plan_check.cpp -- host-only print-out of csrc/tdec_plan.h: the launches of srsran_tdec_gpu_run_multi.
//
// For each case below prints "case X", then one line a launch in issue order
//   launch <build> fused=<0|1> scratch=<0|1> slot=<n> stream=<n> gated=<0|1> wg=<workgroups> K=<sizes> ck=<offsets>
// with a line "large_done" where the event that gates the other classes is recorded, and last "reserved <bytes>".
// ck holds, for a launch that uses the checkpoint scratch, "offset+bytes" of each size's part of it, assigned the way
// the issuer does: the scratch is reserved for the sum of the parts of every such launch, then each launch's sizes take
// theirs in order.  tests/test_tdec_plan_host.py compares the lines with the expectations written out there.
//
// Build and run (no GPU), with -std=c++17 -O1 -fsanitize=address,undefined -fno-sanitize-recover=all:
//   c++ <flags> tools/tdec_plan_check.cpp -o /tmp/tdec_plan_check && /tmp/tdec_plan_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../srsran_4g_amd/csrc/tdec_plan.h"
#include "../srsran_4g_amd/csrc/tdecs_ck_geo.h"

using namespace srsran_amd;

namespace {

// names and code blocks a workgroup of the builds, in TdecBuild order
const char* const kName[TDEC_NOF_BUILDS] = {"quad<16>", "quad<8>",  "quad<1>",  "tdec16", "tdecs16",
                                            "tdecs16w8", "tdecs8", "tdecs8w8", "tdecs1"};
const uint32_t kCpw[TDEC_NOF_BUILDS] = {1, 2, 16, 2, 4, 4, 8, 8, 64};

int res_design(uint32_t K) { return K >= 4864 ? 3 : 4; }  // workgroups a CU
int res_failed(uint32_t) { return 0; }

uint64_t ck_bytes(const TdecGroup& g) { return tdecs_ck_group_bytes(g.K / 16, (g.ncb + 3) / 4); }

void run(const char* name, const std::vector<TdecGroup>& g, bool layout_sb, const TdecTuning& t, int (*res)(uint32_t))
{
  const TdecMultiPlan plan = tdec_multi_plan(g.data(), (uint32_t)g.size(), layout_sb, t, res);
  uint64_t            reserved = 0, used = 0;
  for (const TdecMultiLaunch& l : plan.launches) {
    for (const uint32_t i : l.groups) {
      reserved += l.scratch ? ck_bytes(g[i]) : 0;
    }
  }
  printf("case %s\n", name);
  for (size_t li = 0; li <= plan.launches.size(); li++) {
    if (li == plan.large_done_at) {
      printf("large_done\n");
    }
    if (li == plan.launches.size()) {
      break;
    }
    const TdecMultiLaunch& l  = plan.launches[li];
    uint32_t               wg = 0;
    for (const uint32_t i : l.groups) {
      wg += (g[i].ncb + kCpw[l.build] - 1) / kCpw[l.build];
    }
    printf("launch %s fused=%d scratch=%d slot=%d stream=%d gated=%d wg=%u K=", kName[l.build], l.fused,
           l.scratch, l.slot, l.stream, l.gated, wg);
    for (size_t k = 0; k < l.groups.size(); k++) {
      printf("%s%u", k ? "," : "", g[l.groups[k]].K);
    }
    printf(" ck=");
    for (size_t k = 0; l.scratch && k < l.groups.size(); k++) {
      printf("%s%llu+%llu", k ? "," : "", (unsigned long long)used, (unsigned long long)ck_bytes(g[l.groups[k]]));
      used += ck_bytes(g[l.groups[k]]);
    }
    printf("\n");
  }
  printf("reserved %llu\n", (unsigned long long)reserved);
}

}  // namespace

int main()
{
  std::vector<TdecGroup> s12, all188;
  for (const uint32_t K : {40, 400, 408, 800, 816, 1536, 1568, 2048, 2112, 4800, 4864, 6144}) {
    s12.push_back({K, 5});
  }
  for (uint32_t K = 40; K <= 6144; K += K < 512 ? 8 : K < 1024 ? 16 : K < 2048 ? 32 : 64) {
    all188.push_back({K, 1024});
  }
  const TdecTuning def;
  TdecTuning       single = def;  // the window classes on their single-lane builds
  single.single16_min_cb = single.single8_min_cb = 0;
  TdecTuning every = single;  // and the generic class on its
  every.single1_min_cb = 0;
  TdecTuning nomid = single;
  nomid.mid_cut    = 0;
  run("A", s12, true, single, res_design);
  run("B", s12, true, def, res_design);
  run("C", all188, true, def, res_design);
  run("D", {{6144, 1024}, {40, 1}}, true, def, res_design);
  run("E", s12, false, every, res_design);
  run("F", s12, true, single, res_failed);
  run("G", s12, true, nomid, res_design);
  return 0;
}
