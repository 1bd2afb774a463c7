// srsran_4g_amd/csrc/softbuffer_api.cpp -- the HARQ soft buffers of include/srsran_sch.h, resident in HBM
// (softbuffer.c:36-178), their device arena, the capacity-only transmit soft buffers (softbuffer.c:180-265) and the
// device views other units take of a receive soft buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../include/srsran_sch.h"
#include "dev_buf.h"
#include "devkey.h"
#include "sch_internal.h"
#include "sch_units.h"

using namespace srsran_amd;

namespace {

// 36.213 Table 7.1.7.2.1-1, I_TBS = 33 (the largest index, 256QAM table), N_PRB = 1..110:
// srsran_softbuffer_rx_init sizes max_cb from it (softbuffer.c:38-46).
const int kTbsMaxIdx[SRSRAN_MAX_PRB] = {
       968,   1992,   2984,   4008,   4968,   5992,   6968,   7992,   8760,   9912,  10680,
     11832,  12960,  13536,  14688,  15840,  16992,  17568,  19080,  19848,  20616,  21384,
     22920,  23688,  24496,  25456,  26416,  27376,  28336,  29296,  30576,  31704,  32856,
     34008,  35160,  35160,  36696,  37888,  39232,  39232,  40576,  40576,  42368,  43816,
     43816,  45352,  46888,  46888,  48936,  48936,  51024,  51024,  52752,  52752,  55056,
     55056,  57336,  57336,  59256,  59256,  59256,  61664,  61664,  63776,  63776,  63776,
     66592,  66592,  68808,  68808,  71112,  71112,  71112,  73712,  75376,  76208,  76208,
     76208,  78704,  78704,  81176,  81176,  81176,  81176,  84760,  84760,  84760,  87936,
     87936,  87936,  90816,  90816,  90816,  93800,  93800,  93800,  93800,  97896,  97896,
     97896,  97896,  97896,  97896,  97896,  97896,  97896,  97896,  97896,  97896,  97896,
};

// the code blocks of the largest TB on nof_prb PRB (softbuffer.c:38-46, 182-190), or 0 for a width outside 1..110
uint32_t max_cb_of_prb(uint32_t nof_prb)
{
  if (nof_prb == 0 || nof_prb > SRSRAN_MAX_PRB) {
    return 0;
  }
  return (uint32_t)kTbsMaxIdx[nof_prb - 1] / (SRSRAN_TCOD_MAX_LEN_CB - 24) + 1;
}

// Makes `dev` current for a scope and restores the caller's device: soft buffers are synchronised
// and released on the device they live on, whatever device the caller has selected.
struct DevScope {
  int prev = -1;
  explicit DevScope(int dev)
  {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
      hipSetDevice(dev);
    } else {
      prev = -1;
    }
  }
  ~DevScope()
  {
    if (prev >= 0) {
      hipSetDevice(prev);
    }
  }
};

// Soft-buffer arena: the int16 soft buffers of every srsran_softbuffer_rx_t of a device come from one
// allocation (1 GiB by default, srsran_softbuffer_rx_gpu_arena), which keeps the per-object
// hipMalloc off the HARQ setup path and the blocks of a batch close together in L2 / TLB terms.
// Decoder selection does not depend on it: the turbo descriptor list is padded wherever two
// blocks of a lane-pair workgroup lie far apart (tdec_pair_cbs).  Freed buffers are kept per size
// for reuse; when the arena is full, buffers fall back to hipMalloc (reported once).
struct SbArena {
  uint8_t*                       base = nullptr;
  size_t                         cap = 0, top = 0;
  bool                           tried = false;
  std::multimap<size_t, size_t>  free_by_size;  // size -> offset
};
std::mutex                       g_arena_mu;
std::unordered_map<int, SbArena> g_arenas;
size_t                           g_arena_bytes = (size_t)1 << 30;  // capacity of arenas created from now on
bool                             g_arena_on    = true;             // false: every buffer its own hipMalloc
bool                             g_arena_warned = false;

void* sb_arena_alloc(size_t bytes, int* dev_out)
{
  bytes   = (bytes + 255) & ~(size_t)255;
  int dev = 0;
  hipGetDevice(&dev);
  if (g_arena_on) {
    std::lock_guard<std::mutex> lk(g_arena_mu);
    SbArena&                    a = g_arenas[dev];
    if (!a.tried) {
      a.tried = true;
      if (hipMalloc((void**)&a.base, g_arena_bytes) == hipSuccess) {
        a.cap = g_arena_bytes;
      } else {
        a.base = nullptr;
      }
    }
    auto it = a.free_by_size.find(bytes);
    if (it != a.free_by_size.end()) {
      const size_t off = it->second;
      a.free_by_size.erase(it);
      *dev_out = dev;
      return a.base + off;
    }
    if (a.base && a.top + bytes <= a.cap) {
      const size_t off = a.top;
      a.top += bytes;
      *dev_out = dev;
      return a.base + off;
    }
    if (!g_arena_warned) {
      g_arena_warned = true;
      fprintf(stderr, "[srsran_softbuffer] soft-buffer arena of device %d full (%zu MiB): further buffers use hipMalloc\n",
              dev, a.cap >> 20);
    }
  }
  void* p  = nullptr;
  *dev_out = -1;
  return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}

void sb_arena_free(void* p, size_t bytes, int dev)
{
  if (!p) {
    return;
  }
  if (dev < 0) {
    hipFree(p);
    return;
  }
  bytes = (bytes + 255) & ~(size_t)255;
  std::lock_guard<std::mutex> lk(g_arena_mu);
  SbArena&                    a = g_arenas[dev];
  a.free_by_size.emplace(bytes, (size_t)((uint8_t*)p - a.base));
}

}  // namespace

namespace srsran_amd {
// device views of a soft buffer for other modules of the library (NR SCH)
uint8_t* softbuffer_dflags(srsran_softbuffer_rx_t* q) { return q && q->gpu ? ((SbGpu*)q->gpu)->d_flags : nullptr; }
uint8_t* softbuffer_ddata(srsran_softbuffer_rx_t* q) { return q && q->gpu ? ((SbGpu*)q->gpu)->d_data : nullptr; }
uint32_t softbuffer_data_stride(srsran_softbuffer_rx_t* q) { return q && q->gpu ? ((SbGpu*)q->gpu)->data_stride : 0; }
}  // namespace srsran_amd

extern "C" {

// ---------------- softbuffer.c:36-178 ----------------
int srsran_softbuffer_rx_init(srsran_softbuffer_rx_t* q, uint32_t nof_prb)
{
  const uint32_t max_cb = max_cb_of_prb(nof_prb);
  return max_cb ? srsran_softbuffer_rx_init_guru(q, max_cb, SOFTBUFFER_SIZE) : SRSRAN_ERROR;
}

// ---------------- softbuffer.c:180-265: capacities only (include/srsran_sch.h) ----------------
int srsran_softbuffer_tx_init(srsran_softbuffer_tx_t* q, uint32_t nof_prb)
{
  const uint32_t max_cb = max_cb_of_prb(nof_prb);
  return max_cb ? srsran_softbuffer_tx_init_guru(q, max_cb, SOFTBUFFER_SIZE) : SRSRAN_ERROR;
}

int srsran_softbuffer_tx_init_guru(srsran_softbuffer_tx_t* q, uint32_t max_cb, uint32_t max_cb_size)
{
  if (!q) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  memset(q, 0, sizeof(*q));
  q->max_cb      = max_cb;
  q->max_cb_size = max_cb_size;
  q->buffer_b    = (uint8_t**)calloc(max_cb ? max_cb : 1, sizeof(uint8_t*));
  if (!q->buffer_b) {
    memset(q, 0, sizeof(*q));
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < max_cb; i++) {
    q->buffer_b[i] = reinterpret_cast<uint8_t*>(q->buffer_b);  // placeholder: non-NULL, never dereferenced
  }
  return SRSRAN_SUCCESS;
}

void srsran_softbuffer_tx_free(srsran_softbuffer_tx_t* q)
{
  if (q) {
    free(q->buffer_b);
    memset(q, 0, sizeof(*q));
  }
}

void srsran_softbuffer_tx_reset(srsran_softbuffer_tx_t* q) { (void)q; }

int srsran_softbuffer_rx_init_guru(srsran_softbuffer_rx_t* q, uint32_t max_cb, uint32_t max_cb_size)
{
  if (!q) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  memset(q, 0, sizeof(*q));
  if (!have_gpu()) {
    fprintf(stderr, "[srsran_softbuffer] no HIP device available\n");
    return SRSRAN_ERROR;
  }
  SbGpu* g       = new SbGpu();
  g->stride      = (max_cb_size + 3) & ~3u;  // keeps every buffer 8-byte aligned
  g->data_stride = max_cb_size / 8;
  hipGetDevice(&g->dev);
  q->max_cb      = max_cb;
  q->max_cb_size = max_cb_size;
  q->gpu         = g;
  q->buffer_f    = (int16_t**)calloc(max_cb ? max_cb : 1, sizeof(int16_t*));
  q->data        = (uint8_t**)calloc(max_cb ? max_cb : 1, sizeof(uint8_t*));
  q->cb_crc      = (bool*)calloc(max_cb ? max_cb : 1, sizeof(bool));
  if (!q->buffer_f || !q->data || !q->cb_crc ||
      !(g->buf_bytes = std::max<size_t>((size_t)max_cb * g->stride * sizeof(int16_t), 8),
        g->d_buf     = (short*)sb_arena_alloc(g->buf_bytes, &g->buf_dev)) ||
      !g->d_data.reserve(std::max<size_t>((size_t)max_cb * g->data_stride, 8)) || !g->d_flags.reserve(max_cb + 1)) {
    srsran_softbuffer_rx_free(q);
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < max_cb; i++) {
    q->buffer_f[i] = g->d_buf + (size_t)i * g->stride;
    q->data[i]     = g->d_data + (size_t)i * g->data_stride;
  }
  srsran_softbuffer_rx_reset(q);
  return SRSRAN_SUCCESS;
}

void srsran_softbuffer_rx_reset_cb(srsran_softbuffer_rx_t* q, uint32_t nof_cb)
{
  if (!q || !q->gpu) {
    return;
  }
  SbGpu*   g = (SbGpu*)q->gpu;
  DevScope ds(g->dev);
  nof_cb   = std::min(nof_cb, q->max_cb);
  hipDeviceSynchronize();  // the buffers may still be in use by an asynchronous batch
  if (nof_cb) {
    hipMemset(g->d_buf, 0, (size_t)nof_cb * g->stride * sizeof(int16_t));
    hipMemset(g->d_data, 0, (size_t)nof_cb * g->data_stride);
  }
  hipMemset(g->d_flags, 0, q->max_cb + 1);
  hipDeviceSynchronize();
  memset(q->cb_crc, 0, q->max_cb * sizeof(bool));
  q->tb_crc = false;
}

void srsran_softbuffer_rx_reset(srsran_softbuffer_rx_t* q)
{
  if (q) {
    srsran_softbuffer_rx_reset_cb(q, q->max_cb);
  }
}

void srsran_softbuffer_rx_reset_tbs(srsran_softbuffer_rx_t* q, uint32_t tbs)
{
  if (q) {
    const uint32_t nof_cb = (tbs + 24) / (SRSRAN_TCOD_MAX_LEN_CB - 24) + 1;
    srsran_softbuffer_rx_reset_cb(q, std::min(nof_cb, q->max_cb));
  }
}

void srsran_softbuffer_rx_reset_cb_crc(srsran_softbuffer_rx_t* q, uint32_t nof_cb)
{
  if (!q || nof_cb == 0 || !q->gpu) {
    return;
  }
  nof_cb = std::min(nof_cb, q->max_cb);
  DevScope ds(((SbGpu*)q->gpu)->dev);
  hipDeviceSynchronize();
  hipMemset(((SbGpu*)q->gpu)->d_flags, 0, nof_cb);
  hipDeviceSynchronize();
  memset(q->cb_crc, 0, nof_cb * sizeof(bool));
}

int srsran_softbuffer_rx_sync(srsran_softbuffer_rx_t* q)
{
  if (!q || !q->gpu) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  std::vector<uint8_t> f(q->max_cb + 1);
  DevScope             ds(((SbGpu*)q->gpu)->dev);
  hipDeviceSynchronize();
  if (hipMemcpy(f.data(), ((SbGpu*)q->gpu)->d_flags, f.size(), hipMemcpyDeviceToHost) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < q->max_cb; i++) {
    q->cb_crc[i] = f[i] != 0;
  }
  q->tb_crc = f[q->max_cb] != 0;
  return SRSRAN_SUCCESS;
}

void srsran_softbuffer_rx_free(srsran_softbuffer_rx_t* q)
{
  if (!q) {
    return;
  }
  SbGpu* g = (SbGpu*)q->gpu;
  if (g) {
    // the owning device must be idle before the arena slot can be handed out again
    DevScope ds(g->dev);
    hipDeviceSynchronize();
    sb_arena_free(g->d_buf, g->buf_bytes, g->buf_dev);
    delete g;  // d_data, d_flags: released with their own device current
  }
  free(q->buffer_f);
  free(q->data);
  free(q->cb_crc);
  memset(q, 0, sizeof(*q));
}

int srsran_softbuffer_rx_gpu_arena(int enable, size_t bytes)
{
  std::lock_guard<std::mutex> lk(g_arena_mu);
  g_arena_on = enable != 0;
  if (bytes) {
    g_arena_bytes = bytes;
  }
  return SRSRAN_SUCCESS;
}

const void* srsran_softbuffer_rx_gpu_ptr(const srsran_softbuffer_rx_t* q)
{
  return q && q->gpu ? ((const SbGpu*)q->gpu)->d_buf : nullptr;
}

}  // extern "C"
