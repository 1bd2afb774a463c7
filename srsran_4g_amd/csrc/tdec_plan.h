// srsran_4g_amd/csrc/tdec_plan.h -- which build of the turbo decoder a launch runs, and the launches of one
// srsran_tdec_gpu_run_multi call.  Pure host code without HIP: tdec_dispatch.cpp and tdec_api.cpp act on it,
// tools/tdec_plan_check.cpp (tests/test_tdec_plan_host.py) prints it.
#ifndef SRSRAN_AMD_TDEC_PLAN_H
#define SRSRAN_AMD_TDEC_PLAN_H
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <functional>
#include <vector>

namespace srsran_amd {

// The thresholds and cuts of the choice (tdec_dispatch.cpp holds the process's; the srsran_tdec_gpu_set_* entry
// points move them, tests force each kernel onto small batches with 0).
struct TdecTuning {
  // Which 16-sub-block decoder a launch of n blocks gets (K = 6144, 8 half-iterations, ms per launch,
  // gpurun_out r03d -> profiles/r03_tdec_kernels.jsonl):
  //      n      quad (tdec_kernel<16>)   lane pair (tdec16_kernel)   single lane (tdec16s_kernel)
  //    256            0.258                    0.275                        0.344
  //    512            0.339                    0.282                        0.348
  //   1024            0.403                    0.394                        0.362
  //   2048            0.766                    0.457                        0.382
  // The quad decoder (one block a workgroup) fills the chip best below ~512 blocks, the lane pair between,
  // and the single-lane decoder (64 lanes a wave on 4 blocks, the densest mapping) from 1024 on.
  uint32_t pair_min_cb = 512u;  // srsran_tdec_gpu_set_pair_threshold()
  // srsran_tdec_gpu_set_single_threshold(): blocks a launch from which the single-lane decoders
  // (tdecs_kernel.hip, 16-sub-block class) replaces the lane pair.  Between 512 and 1024 blocks
  // (K = 6144, gpurun_out r03af): single lane / lane pair 0.345 / 0.385 ms at 640, 0.349 / 0.390 at 768,
  // 0.359 / 0.394 at 896, 0.361 / 0.397 at 1014 (the PUSCH batch of 78 UEs x 13 blocks: 0.108 vs 0.113 ms
  // with early stop); the lane pair is ahead at 512 (0.282 vs 0.348): from 576 blocks.
  uint32_t single16_min_cb = 576u;
  // The 8-sub-block class: its quad decoder (one block a workgroup) stays ahead up to ~1024 blocks a launch
  // (K = 512: 0.060 vs 0.085 ms at 512, 0.081 vs 0.086 ms at 1024) and the single-lane decoder is ahead on
  // the fused class launch (32 sizes x 256 = 8192 blocks: 0.30 vs 0.53 ms): from 4096 blocks by default.
  uint32_t single8_min_cb = 4096u;
  // srsran_tdec_gpu_set_generic_single_threshold(): the generic class (K <= 400) keeps tdec_kernel.hip's
  // quad decoder by default: one lane per block and direction runs the whole K-step recursion serially, and
  // at 1024 blocks per size (47104 blocks) tdec1s_kernel takes 1.47 ms against the quad decoder's 0.78 ms
  // (profiles/r03_tdec_kernels.jsonl), so tdec1s is selected only when a caller lowers this threshold.
  uint32_t single1_min_cb = 0xffffffffu;
  // srsran_tdec_gpu_set_w8_max_k(): single-lane launches whose block sizes are all <= this K use the build
  // with 8-step windows (tdecs_kernel.hip, TDECS_W = 8: 164-191 VGPRs, two waves a SIMD where LDS allows).
  // Default 800 = the whole 8-sub-block class (408 <= K <= 800), where it wins: the fused class launch of
  // 32 sizes x 1024 blocks 0.71 vs 0.91 ms, x 4096 blocks 2.30 vs 3.39 ms (gpurun_out r03l).  The 16-sub-block
  // class keeps 16-step windows: its 8-step build is slower at every K measured (2048 blocks, K = 1024 / 2048
  // / 4096 / 6144: 0.129 / 0.219 / 0.395 / 0.738 ms against 0.096 / 0.153 / 0.268 / 0.380 ms): twice the
  // windows a sub-block for the same training overlap, and at 19 KB of LDS a block the second wave a
  // SIMD does not fit at large K anyway.
  uint32_t w8_max_k = 800u;
  // srsran_tdec_gpu_set_w8_fused_max_k(): in a fused multi-size launch of the 16-sub-block single-lane class,
  // the sizes up to this K form their own launch on the 8-step-window build (their workgroups, at 164-191
  // registers and little LDS, share SIMDs with the large sizes' workgroups).  All-188 step, one box,
  // alternating runs (gpurun_out r03z): cut at 800 (none) 12.22 ms, 1536 11.65 ms, 2368 11.71-11.73 ms,
  // 3136 12.37 ms.  With the 16-step part cut again at SRSRAN_AMD_TDEC_MIDCUT = 3072 (r06v, one box, alternating):
  // 1024 10.95 ms, 1536 10.615 / 10.621 ms, 1792 10.68 ms, 2048 10.686 / 10.71 ms, 2560 11.34 ms.
  uint32_t w8_fused_max_k = 1536u;
  // The 16-step part of a fused 16-sub-block class is cut once more at this K (SRSRAN_AMD_TDEC_MIDCUT, read once;
  // 0 = no mid part): its sizes above run first, cut by residency (tdec_multi_plan: three or four workgroups a CU
  // at two waves a SIMD, nothing else fits beside them), its sizes up to the cut follow on the same stream with
  // their own, smaller LDS figure -- room beside them for the 8-step part's, the 8-sub-block class's and the generic
  // class's workgroups.  2048 from the sweep with the two-wave kernel (HISTORY.md; 3072 at one wave a SIMD).
  uint32_t mid_cut = 2048u;
};

// The nine builds: the quad decoder per class (tdec_kernel.hip), the lane pair (tdec16_kernel.hip), one lane per
// sub-block with 16- and 8-step windows (tdecs_kernel.hip) and the generic single lane (tdec1s_kernel.hip).
enum TdecBuild {
  TDEC_QUAD16,
  TDEC_QUAD8,
  TDEC_QUAD1,
  TDEC_PAIR16,
  TDEC_S16,
  TDEC_S16W8,
  TDEC_S8,
  TDEC_S8W8,
  TDEC_S1,
  TDEC_NOF_BUILDS
};

// AUTO's sub-blocks of a size (turbodecoder.c:381-408): 16, 8, or 1 for the generic decoder
inline int tdec_auto_nsb(uint32_t K) { return !(K % 16) && K > 800 ? 16 : !(K % 8) && K > 400 ? 8 : 1; }

// The build of a launch of ncb blocks of the nsb-sub-block class.  The window classes leave the quad decoder
// only on the SB input layout and without state save / restore (`resumable`: n_start != 0 or a state buffer; every
// size of theirs has the 40 positions a sub-block that the other decoders train on, get_config()).  In a fused
// multi-size launch ncb is the class's block count and K the launch's largest size, and the 16-sub-block class's
// 8-step cut is the larger of the two.
inline TdecBuild tdec_pick_build(const TdecTuning& t, int nsb, uint32_t K, uint32_t ncb, bool layout_sb,
                                 bool resumable, bool fused)
{
  const bool window = layout_sb && !resumable;
  if (nsb == 16 && window && ncb >= t.single16_min_cb) {
    return K <= (fused ? std::max(t.w8_max_k, t.w8_fused_max_k) : t.w8_max_k) ? TDEC_S16W8 : TDEC_S16;
  }
  if (nsb == 16 && window && ncb >= t.pair_min_cb) {
    return TDEC_PAIR16;
  }
  if (nsb == 8 && window && ncb >= t.single8_min_cb) {
    return K <= t.w8_max_k ? TDEC_S8W8 : TDEC_S8;
  }
  if (nsb == 1 && !resumable && ncb >= t.single1_min_cb) {
    return TDEC_S1;  // always the natural layout (rm_turbo.c:403-425)
  }
  return nsb == 16 ? TDEC_QUAD16 : nsb == 8 ? TDEC_QUAD8 : TDEC_QUAD1;
}

struct TdecGroup {
  uint32_t K;
  uint32_t ncb;
};

// One launch of a multi-size call.
struct TdecMultiLaunch {
  TdecBuild build;
  bool      fused;    // several sizes in one grid; false: one size, through tdec_launch
  bool      scratch;  // the fused 16-step kernel: window checkpoints in the pool's device scratch
  bool      gated;    // waits for the sizes above the mid cut (large_done)
  int       slot;     // staging slot of its descriptors
  int       stream;   // pool stream
  std::vector<uint32_t> groups;  // in launch order
};

struct TdecMultiPlan {
  std::vector<TdecMultiLaunch> launches;
  size_t large_done_at = 0;  // large_done is recorded on stream 0 in front of launches[large_done_at]
};

static constexpr int kTdecPlanSlots = 6;

// Rough serial-latency model used only to order launches (longest first).
inline double tdec_launch_cost(uint32_t K, uint32_t ncb)
{
  const int    nsb   = tdec_auto_nsb(K);
  const double chain = nsb > 1 ? 3.0 * (K / nsb) + 160.0 : 3.0 * (K + 3);
  const double waves = (double)ncb * 4 * nsb / 64.0;
  return chain * (1.0 + waves / 1024.0);
}

// The launches of one call, in issue order.  One fused launch per decoder class (16 / 8 / generic): the sizes of a
// class share one grid (more workgroups in flight than per-size launches, no per-launch tail), longest first; the
// class's build is chosen on its total block count, and a part left with one size is a plain launch of that size.
// Classes run on separate pool streams.  A single-lane 16-sub-block class is cut in four:
//   slot 0  K > max(8-step cut, mid cut) at the residency of the largest K      stream 0
//   slot 1  the other K > max(8-step cut, mid cut)                              stream 0
//   slot 2  8-step cut < K <= mid cut                                           stream 0, behind large_done
//   slot 3  K <= 8-step cut, on 8-step windows (fewer registers and little LDS a workgroup: they share SIMDs with
//           the larger sizes' workgroups)                                       stream 1
// then slot 4, the 8-sub-block class (stream 2), and slot 5, the generic class (stream 3).  The fused 16-step kernel
// runs two waves a SIMD and keeps its checkpoints out of LDS, so the workgroups a CU holds depend on the launch's
// LDS figure: `residency(K)` is that count for a launch whose largest size is K (three a CU at K = 6144, four -- the
// register limit -- from about K = 4600 down; 0 when the query failed), and each part is launched with the LDS of
// its own largest K.  With a mid part, the launches on the other streams wait for the large sizes to finish: started
// at once they only take CUs the large workgroups would have used, since no large workgroup leaves room beside it.
inline TdecMultiPlan tdec_multi_plan(const TdecGroup* groups, uint32_t nof_groups, bool layout_sb, const TdecTuning& t,
                                     const std::function<int(uint32_t)>& residency)
{
  std::vector<uint32_t> order(nof_groups);
  for (uint32_t g = 0; g < nof_groups; g++) {
    order[g] = g;
  }
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return tdec_launch_cost(groups[a].K, groups[a].ncb) > tdec_launch_cost(groups[b].K, groups[b].ncb);
  });
  TdecMultiPlan plan;
  bool          mid_run = false;
  const struct {
    int nsb, slot, stream;
  } classes[] = {{16, 0, 0}, {8, 4, 2}, {1, 5, 3}};
  for (const auto& c : classes) {
    const int             nsb = c.nsb;
    std::vector<uint32_t> cls;
    uint32_t              cls_cb = 0, kmax = 0;  // blocks of the whole class (decide the build)
    for (const uint32_t g : order) {
      if (tdec_auto_nsb(groups[g].K) == nsb && groups[g].ncb > 0) {
        cls.push_back(g);
        cls_cb += groups[g].ncb;
        kmax = std::max(kmax, groups[g].K);
      }
    }
    // the sizes of the class that `in_part` takes, as one launch
    auto part = [&](int slot, int stream, auto&& in_part) {
      TdecMultiLaunch l{};
      uint32_t        top = 0;
      for (const uint32_t g : cls) {
        if (in_part(groups[g].K)) {
          l.groups.push_back(g);
          top = std::max(top, groups[g].K);
        }
      }
      if (l.groups.empty()) {
        return false;
      }
      l.fused   = l.groups.size() > 1;
      l.build   = l.fused ? tdec_pick_build(t, nsb, top, cls_cb, layout_sb, false, true)
                          : tdec_pick_build(t, nsb, top, groups[l.groups[0]].ncb, layout_sb, false, false);
      l.scratch = l.fused && l.build == TDEC_S16;
      l.gated   = mid_run && stream != 0;
      l.slot    = slot;
      l.stream  = stream;
      plan.launches.push_back(l);
      return true;
    };
    const TdecBuild cls_build = tdec_pick_build(t, nsb, kmax, cls_cb, layout_sb, false, true);
    if (nsb == 16 && (cls_build == TDEC_S16 || cls_build == TDEC_S16W8)) {
      const uint32_t cut     = std::max(t.w8_max_k, t.w8_fused_max_k);
      const uint32_t large   = std::max(cut, t.mid_cut);
      const int      top_res = kmax > large ? residency(kmax) : 0;
      part(0, 0, [&](uint32_t K) { return K > large && residency(K) == top_res; });
      part(1, 0, [&](uint32_t K) { return K > large && residency(K) != top_res; });
      plan.large_done_at = plan.launches.size();
      mid_run            = part(2, 0, [&](uint32_t K) { return K > cut && K <= large; });
      part(3, 1, [&](uint32_t K) { return K <= cut; });
    } else {
      part(c.slot, c.stream, [](uint32_t) { return true; });
      plan.large_done_at = nsb == 16 ? plan.launches.size() : plan.large_done_at;
    }
  }
  return plan;
}

}  // namespace srsran_amd
#endif
