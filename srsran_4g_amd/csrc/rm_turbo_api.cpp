// srsran_4g_amd/csrc/rm_turbo_api.cpp -- turbo rate matching, host side (include/srsran_sch.h; rm_turbo.c):
//   rate de-matching tables            rm_turbo.c:175-317 (read by rm_rx_kernel, sch_kernel.hip)
//   the transmitter's read-out tables  rm_turbo.c:345-388 (read by enc_kernel.hip)
//   srsran_rm_turbo_rx_lut*            rm_turbo.c:276-483, host-synchronous
// The tables are built per (device, K, rv, layout) on first use and kept for the process.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/srsran_sch.h"
#include "dev_buf.h"
#include "devkey.h"
#include "sch_internal.h"
#include "sch_kernel.h"
#include "sch_units.h"
#include "tdec8bit_kernel.h"

using namespace srsran_amd;

namespace {

// Sub-block interleaver inter-column permutation, 36.212 Table 5.1.4-1.
const uint8_t kColPerm[32] = {0, 16, 8,  24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30,
                              1, 17, 9,  25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31};

std::mutex                   g_tab_mu;  // the two table caches below
std::map<uint64_t, InvTable> g_inv;     // (device, cb_idx, rv, layout)

uint32_t rx_subblocks(uint32_t K, bool tdec_layout)
{
  return tdec_layout ? srsran_tdec_autoimp_get_subblocks(K) : 0;
}

}  // namespace

namespace srsran_amd {

bool inv_table_nsb(uint32_t cb_idx, uint32_t rv, uint32_t nsb, InvTable* out)
{
  const uint32_t              K   = (uint32_t)srsran_cbsegm_cbsize(cb_idx);
  const uint64_t              key = ((uint64_t)cur_dev() << 32) | ((cb_idx * 4 + rv) * 64 + nsb);
  std::lock_guard<std::mutex> lk(g_tab_mu);
  auto                        it = g_inv.find(key);
  if (it != g_inv.end()) {
    *out = it->second;
    return true;
  }
  if (!have_gpu()) {
    return false;
  }
  const uint32_t D = K + 4, R = (D + 31) / 32, Kp = 32 * R, ND = Kp - D, Kw = 3 * Kp;
  const uint32_t k0 = R * (2 * ((Kw + 8 * R - 1) / (8 * R)) * rv + 2);  // 36.212 5.1.4.1.2
  InvTable       t;
  t.N   = 3 * K + 12;
  t.len = nsb ? 3 * (K + 32) + 12 : t.N;
  std::vector<uint16_t> inv(t.len, 0xFFFF);
  const uint32_t        L = nsb ? K / nsb : K;
  for (uint32_t k = 0, j = 0; k < t.N; j++) {
    const uint32_t w = (k0 + j) % Kw;
    uint32_t       stream, col;
    if (w < Kp) {
      stream = 0;
      col    = w;
    } else {
      stream = 1 + ((w - Kp) & 1);
      col    = (w - Kp) >> 1;
    }
    uint32_t y = kColPerm[col / R] + 32 * (col % R);  // position in the padded stream
    if (stream == 2) {
      y = (y + 1) % Kp;  // pi(k) for the second parity stream
    }
    if (y < ND) {
      continue;  // dummy bit, not transmitted
    }
    const uint32_t i = y - ND;        // bit index in d^(stream)
    uint32_t       n = 3 * i + stream;  // encoder output order (natural 3K+12 layout)
    if (nsb) {  // turbo decoder sub-block layout (rm_turbo.c:260-273)
      n = n < 3 * K ? (n % 3) * (K + 32) + ((n / 3) % L) * nsb + (n / 3) / L : n - 3 * K + 3 * (K + 32);
    }
    inv[n] = (uint16_t)k++;
  }
  if (hipMalloc(&t.d, t.len * sizeof(uint16_t)) != hipSuccess ||
      hipMemcpy(t.d, inv.data(), t.len * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) {
    return false;
  }
  g_inv[key] = t;
  *out       = t;
  return true;
}

bool inv_table(uint32_t cb_idx, uint32_t rv, bool tdec_layout, InvTable* out)
{
  return inv_table_nsb(cb_idx, rv, rx_subblocks((uint32_t)srsran_cbsegm_cbsize(cb_idx), tdec_layout), out);
}

// Rate-matching read-out for the transmitter (rm_turbo.c:345-388): fwd[k] = the natural-layout
// encoder output index (3 i + stream, tail 3K..3K+11) of the k-th transmitted bit of the rv's
// circular buffer, period 3K + 12 along the E bits.  The inverse of the receive table.
bool rm_fwd_table(uint32_t cb_idx, uint32_t rv, const uint16_t** d_fwd, uint32_t* N)
{
  static std::map<uint64_t, uint16_t*> cache;
  const uint32_t                       K   = (uint32_t)srsran_cbsegm_cbsize(cb_idx);
  const uint64_t                       key = ((uint64_t)cur_dev() << 32) | (cb_idx * 4 + rv);
  *N                                       = 3 * K + 12;
  {
    std::lock_guard<std::mutex> lk(g_tab_mu);
    auto                        it = cache.find(key);
    if (it != cache.end()) {
      *d_fwd = it->second;
      return true;
    }
  }
  InvTable t;
  if (!inv_table(cb_idx, rv, false, &t)) {
    return false;
  }
  std::vector<uint16_t> inv(t.len), fwd(t.N);
  if (hipMemcpy(inv.data(), t.d, t.len * sizeof(uint16_t), hipMemcpyDeviceToHost) != hipSuccess) {
    return false;
  }
  for (uint32_t n = 0; n < t.len; n++) {
    fwd[inv[n]] = (uint16_t)n;
  }
  uint16_t* d = nullptr;
  if (hipMalloc((void**)&d, t.N * sizeof(uint16_t)) != hipSuccess ||
      hipMemcpy(d, fwd.data(), t.N * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) {
    return false;
  }
  std::lock_guard<std::mutex> lk(g_tab_mu);
  cache[key] = d;
  *d_fwd     = d;
  return true;
}

}  // namespace srsran_amd

namespace {
std::mutex g_rm_mu;
struct RmCtx {  // one per device: the host-synchronous srsran_rm_turbo_rx_lut_ scratch
  hipStream_t stream = nullptr;
  DevBuf<int16_t> d_in;  // int8 values in srsran_rm_turbo_rx_lut_8bit
  DevBuf<int16_t> d_out;
  DevBuf<RmSlot>  d_slot;
  DevBuf<uint8_t> d_zero;
};

// the current device's context with `in_bytes` of input scratch, or nullptr.  The contexts live for the process:
// the map is never destroyed, so no hipFree runs after the runtime is gone.
RmCtx* rm_ctx(size_t in_bytes)
{
  static auto& ctxs = *new std::map<int, RmCtx>;
  RmCtx&       c    = ctxs[cur_dev()];
  if (!c.stream) {
    if (hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking) != hipSuccess ||
        !c.d_out.reserve(SOFTBUFFER_SIZE) || !c.d_slot.reserve(1) || !c.d_zero.reserve(8) ||
        hipMemset(c.d_zero, 0, 8) != hipSuccess) {
      return nullptr;
    }
  }
  return c.d_in.reserve((std::max<size_t>(in_bytes, 1) + 1) / 2) ? &c : nullptr;
}
}  // namespace

extern "C" {

// ---------------- rm_turbo.c:276-483 ----------------
void srsran_rm_turbo_gentables(void)
{
  // device tables are built lazily per (K, rv, layout) on first use and kept for the process
}

void srsran_rm_turbo_free_tables(void) {}

int srsran_rm_turbo_rx_lut_(int16_t* input,
                            int16_t* output,
                            uint32_t in_len,
                            uint32_t cb_idx,
                            uint32_t rv_idx,
                            bool     enable_input_tdec)
{
  if (rv_idx >= 4 || cb_idx >= SRSRAN_NOF_TC_CB_SIZES) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (!input || !output) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  InvTable t;
  if (!inv_table(cb_idx, rv_idx, enable_input_tdec, &t)) {
    fprintf(stderr, "[srsran_rm_turbo] no HIP device available\n");
    return SRSRAN_ERROR;
  }
  std::lock_guard<std::mutex> lk(g_rm_mu);
  RmCtx*                      cp = rm_ctx((size_t)in_len * sizeof(int16_t));
  if (!cp) {
    return SRSRAN_ERROR;
  }
  RmCtx& c = *cp;
  RmSlot s;
  s.e    = c.d_in;
  s.sb   = c.d_out;
  s.skip = c.d_zero;
  s.inv  = t.d;
  s.E    = in_len;
  s.len  = t.len;
  s.N    = t.N;
  s.overwrite = 0;
  hipMemcpyAsync(c.d_in, input, (size_t)in_len * sizeof(int16_t), hipMemcpyHostToDevice, c.stream);
  hipMemcpyAsync(c.d_out, output, t.len * sizeof(int16_t), hipMemcpyHostToDevice, c.stream);
  hipMemcpyAsync(c.d_slot, &s, sizeof(s), hipMemcpyHostToDevice, c.stream);
  if (rm_rx_launch(c.d_slot, 1, t.len, in_len, c.stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  hipMemcpyAsync(output, c.d_out, t.len * sizeof(int16_t), hipMemcpyDeviceToHost, c.stream);
  return hipStreamSynchronize(c.stream) == hipSuccess ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

int srsran_rm_turbo_rx_lut(int16_t* input, int16_t* output, uint32_t in_len, uint32_t cb_idx, uint32_t rv_idx)
{
  return srsran_rm_turbo_rx_lut_(input, output, in_len, cb_idx, rv_idx, true);
}

// rm_turbo.c:447-483 (the SSE 8-bit path of an AVX2 build, :586-687): output[deinter[i % (3K + 12)]] += input[i]
// with int8 wrap-around, on the sub-block layout of the 8-bit decoder that takes K
// (srsran_tdec_autoimp_get_subblocks_8bit: 32 / 16 / 8 sub-blocks, natural below K = 408)
int srsran_rm_turbo_rx_lut_8bit(int8_t* input, int8_t* output, uint32_t in_len, uint32_t cb_idx, uint32_t rv_idx)
{
  if (rv_idx >= 4 || cb_idx >= SRSRAN_NOF_TC_CB_SIZES || !input || !output) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t K = (uint32_t)srsran_cbsegm_cbsize(cb_idx);
  InvTable       t;
  if (!inv_table_nsb(cb_idx, rv_idx, srsran_tdec_autoimp_get_subblocks_8bit(K), &t)) {
    fprintf(stderr, "[srsran_rm_turbo] no HIP device available\n");
    return SRSRAN_ERROR;
  }
  std::lock_guard<std::mutex> lk(g_rm_mu);
  RmCtx*                      cp = rm_ctx(in_len);
  if (!cp) {
    return SRSRAN_ERROR;
  }
  RmCtx&  c     = *cp;
  int8_t* d_in  = (int8_t*)c.d_in.get();
  int8_t* d_out = (int8_t*)c.d_out.get();
  hipMemcpyAsync(d_in, input, in_len, hipMemcpyHostToDevice, c.stream);
  hipMemcpyAsync(d_out, output, t.len, hipMemcpyHostToDevice, c.stream);
  if (srsran_amd::rm8_rx_launch(d_in, d_out, t.d, in_len, t.len, t.N, c.stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  hipMemcpyAsync(output, d_out, t.len, hipMemcpyDeviceToHost, c.stream);
  return hipStreamSynchronize(c.stream) == hipSuccess ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

}  // extern "C"
