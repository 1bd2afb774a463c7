// srsran_4g_amd/csrc/tdec_dispatch.cpp -- the turbo decoder's tuning, table of builds and launch entry
// (tdec_dispatch.h).
#include "tdec_dispatch.h"

#include <cstdlib>

namespace srsran_amd {

namespace {
TdecTuning& tuning()
{
  static TdecTuning t = [] {
    TdecTuning  d;
    const char* e = getenv("SRSRAN_AMD_TDEC_MIDCUT");
    d.mid_cut     = e ? (uint32_t)atoi(e) : d.mid_cut;
    return d;
  }();
  return t;
}

template <int NSB>
TdecBuildRow quad_row(const char* api_name)
{
  return {api_name,
          [] { return tdec_cpw(NSB); },
          [](const TdecArgs& a) { return tdec_lds_bytes(NSB, a.xyw, a.M); },
          [](const TdecArgs& a, hipStream_t s) { return tdec_quad_launch(NSB, a, s); },
          [](const TdecArgs* d_groups, const uint32_t* d_first, int ngroups, uint32_t nblocks, size_t lds,
             hipStream_t s) { return tdec_multi_launch(NSB, d_groups, d_first, ngroups, nblocks, lds, s); }};
}
}  // namespace

TdecTuning tdec_tuning()
{
  const TdecTuning& g = tuning();
  TdecTuning        t;
  for (uint32_t TdecTuning::*f :
       {&TdecTuning::pair_min_cb, &TdecTuning::single16_min_cb, &TdecTuning::single8_min_cb,
        &TdecTuning::single1_min_cb, &TdecTuning::w8_max_k, &TdecTuning::w8_fused_max_k, &TdecTuning::mid_cut}) {
    t.*f = __atomic_load_n(&(g.*f), __ATOMIC_RELAXED);
  }
  return t;
}

void tdec_tune(uint32_t TdecTuning::*field, uint32_t value)
{
  __atomic_store_n(&(tuning().*field), value, __ATOMIC_RELAXED);
}

const TdecBuildRow& tdec_build(TdecBuild b)
{
  static const TdecBuildRow rows[TDEC_NOF_BUILDS] = {
      quad_row<16>("tdec_kernel<16>"),
      quad_row<8>("tdec_kernel<8>"),
      quad_row<1>("tdec_kernel<1>"),
      {"tdec16_kernel", tdec16_cpw, tdec16_lds_bytes, tdec16_launch, tdec16_multi_launch},
      {"tdec16s_kernel", tdecs16::cpw, tdecs16::lds_bytes, tdecs16::launch, tdecs16::multi_launch},  // fused: _ck
      {"tdec16s_kernel", tdecs16w8::cpw, tdecs16w8::lds_bytes, tdecs16w8::launch, tdecs16w8::multi_launch},
      {"tdec8s_kernel", tdecs8::cpw, tdecs8::lds_bytes, tdecs8::launch, tdecs8::multi_launch},
      {"tdec8s_kernel", tdecs8w8::cpw, tdecs8w8::lds_bytes, tdecs8w8::launch, tdecs8w8::multi_launch},
      {"tdec1s_kernel", tdecs1::cpw, tdecs1::lds_bytes, tdecs1::launch, tdecs1::multi_launch},
  };
  return rows[b];
}

hipError_t tdec_launch(int nsb, const TdecArgs& a, hipStream_t stream)
{
  if (a.ncb == 0) {
    return hipSuccess;
  }
  if (nsb != 16 && nsb != 8 && nsb != 1) {
    return hipErrorInvalidValue;
  }
  const bool resumable = a.n_start != 0 || a.state != nullptr;
  return tdec_build(tdec_pick_build(tdec_tuning(), nsb, a.K, a.ncb, a.layout_sb, resumable, false)).launch(a, stream);
}

}  // namespace srsran_amd
