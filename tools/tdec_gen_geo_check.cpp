// tools/tdec_gen_geo_check.cpp -- prints the workgroup LDS of the generic turbo decoder (K <= 400, the NSB = 1
// kernels of tdec_kernel.hip) from the header its launch sizes it from (csrc/tdec_gen_geo.h), one line a size:
//   K=<K> M=<checkpoints> s=<B> ck=<B> bits=<B> lds=<B> wg_per_cu=<n> state=<int16 a block>
// Host only: g++ -std=c++17 tools/tdec_gen_geo_check.cpp (tests/test_tdec_gen_occupancy_host.py builds it under
// the address and undefined-behaviour sanitizers).
#include <cstdio>

#include "../srsran_4g_amd/csrc/tdec_gen_geo.h"

int main()
{
  using namespace srsran_amd;
  for (uint32_t K = 40; K <= (uint32_t)TDEC_GEN_KMAX; K += 8) {
    const uint32_t   M   = tdec_gen_M(K);
    const TdecGenGeo g   = tdec_gen_geo(K, M);
    const size_t     lds = tdec_gen_lds_bytes(K);
    if (lds != (size_t)g.total_dw * 4) {
      return 1;
    }
    printf("K=%u M=%u s=%u ck=%u bits=%u lds=%zu wg_per_cu=%zu state=%zu\n", K, M, g.s_dw * 4, g.ck_dw * 4,
           TDEC_GEN_CPW * g.bits_dw * 4, lds, (size_t)TDEC_LDS_PER_CU / lds, tdec_gen_state_len(K));
  }
  return 0;
}
