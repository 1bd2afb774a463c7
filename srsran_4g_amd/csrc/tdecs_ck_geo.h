// srsran_4g_amd/csrc/tdecs_ck_geo.h -- geometry of the window-checkpoint scratch of the fused 16-step launches
// (tdecs_kernel.hip, GCK), shared by the kernel, the host (tdec_api.cpp) and tools/tdec_ck_walk.cpp.
//
// The scratch is one device buffer.  Every workgroup of a launch owns one region of it:
//   [M windows][64 lanes][16 B]     M = ceil(L / 16), lane = block of the workgroup * NSB + sub-block
// so a wave's store of one checkpoint is a contiguous kilobyte.  Both waves of a workgroup use the same lane
// index (the forward wave writes windows [0, h), the backward wave [h, M)).  The regions of a group (one K) follow
// each other from the group's base; the groups of a launch follow each other in launch order.  The kernel reaches
// its region through a buffer resource of exactly the region's bytes (clipped to what the group was given), so
// nothing a workgroup does can touch another's region: out-of-range stores are dropped, loads return zero.
#ifndef SRSRAN_AMD_TDECS_CK_GEO_H
#define SRSRAN_AMD_TDECS_CK_GEO_H
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TDECS_CK_HD __host__ __device__
#else
#define TDECS_CK_HD
#endif

namespace srsran_amd {

static constexpr uint32_t TDECS_CK_W     = 16;    // window of the builds that use the scratch
static constexpr uint32_t TDECS_CK_LANES = 64;    // lanes of a wave
static constexpr uint32_t TDECS_CK_STATE = 16;    // bytes of one checkpoint (8 int16 states)
static constexpr uint32_t TDECS_CK_ROW   = TDECS_CK_LANES * TDECS_CK_STATE;  // one window of a workgroup

// windows (checkpoint slots) of a sub-block of L positions
TDECS_CK_HD inline uint32_t tdecs_ck_windows(uint32_t L) { return (L + TDECS_CK_W - 1) / TDECS_CK_W; }
// bytes of one workgroup's region
TDECS_CK_HD inline uint32_t tdecs_ck_wg_bytes(uint32_t L) { return tdecs_ck_windows(L) * TDECS_CK_ROW; }
// bytes of a group of nwg workgroups
TDECS_CK_HD inline uint64_t tdecs_ck_group_bytes(uint32_t L, uint32_t nwg) { return (uint64_t)nwg * tdecs_ck_wg_bytes(L); }
// bytes from the group's base to workgroup wg's region
TDECS_CK_HD inline uint64_t tdecs_ck_wg_off(uint32_t L, uint32_t wg) { return (uint64_t)wg * tdecs_ck_wg_bytes(L); }
// bytes of workgroup wg's region that lie inside the group_bytes the group was given (the buffer resource's size)
TDECS_CK_HD inline uint32_t tdecs_ck_wg_avail(uint32_t L, uint32_t wg, uint64_t group_bytes)
{
  const uint64_t off = tdecs_ck_wg_off(L, wg);
  const uint64_t len = tdecs_ck_wg_bytes(L);
  return off >= group_bytes ? 0u : (uint32_t)(group_bytes - off < len ? group_bytes - off : len);
}
// within a region: bytes to window m's row (wave-uniform) and to a lane's checkpoint in a row
TDECS_CK_HD inline uint32_t tdecs_ck_row(int m) { return (uint32_t)m * TDECS_CK_ROW; }
TDECS_CK_HD inline uint32_t tdecs_ck_lane(uint32_t lane) { return lane * TDECS_CK_STATE; }

}  // namespace srsran_amd
#endif
