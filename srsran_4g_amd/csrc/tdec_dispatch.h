// srsran_4g_amd/csrc/tdec_dispatch.h -- the turbo decoder's tuning, its table of builds and the one launch
// entry that picks among them (tdec_plan.h: tdec_pick_build).
#ifndef SRSRAN_AMD_TDEC_DISPATCH_H
#define SRSRAN_AMD_TDEC_DISPATCH_H
#include "tdec_kernel.h"
#include "tdec_plan.h"

namespace srsran_amd {

// The process's tuning: a snapshot, and the store behind the srsran_tdec_gpu_set_* entry points (relaxed atomics:
// a thread may move a threshold between other threads' launches).  mid_cut comes from SRSRAN_AMD_TDEC_MIDCUT once.
TdecTuning tdec_tuning();
void       tdec_tune(uint32_t TdecTuning::*field, uint32_t value);

// What the hosts need of a build; the functions are the ones its .hip file defines.
struct TdecBuildRow {
  const char* api_name;  // srsran_tdec_gpu_kernel_name_batch()
  int (*cpw)();          // code blocks per workgroup
  size_t (*lds_bytes)(const TdecArgs& a);
  hipError_t (*launch)(const TdecArgs& a, hipStream_t stream);
  // ngroups descriptors (device array) in one launch; d_first[g] = first workgroup of group g (ascending);
  // lds = the largest lds_bytes of the groups.
  // Special case, TDEC_S16: its fused kernel keeps the window checkpoints in a device scratch and is launched
  // through tdecs16::multi_launch_ck with tdecs16::multi_lds_bytes / multi_ck_bytes (tdec_kernel.h) instead.
  hipError_t (*multi_launch)(const TdecArgs* d_groups, const uint32_t* d_first, int ngroups, uint32_t nblocks,
                             size_t lds, hipStream_t stream);
};
const TdecBuildRow& tdec_build(TdecBuild b);

// One size on the build that tdec_pick_build chooses for it
hipError_t tdec_launch(int nsb, const TdecArgs& a, hipStream_t stream);

}  // namespace srsran_amd
#endif
