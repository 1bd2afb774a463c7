// srsran_4g_amd/csrc/phich_api.cpp -- PHICH object (include/srsran_phich.h; phich.c).
//
// Host: resource arithmetic (36.213 9.1.2), validation as phich.c:198-212 / 326-340, the 12 scrambling bits of every
// subframe (srsran_sequence_phich, sequences.c:46-49), grouping of a batch's items by (subframe, mapping unit) in
// put order.  GPU (phich_kernel.hip): everything between the ACK bit and the grid, and back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/srsran_phich.h"
#include "dev_buf.h"
#include "devkey.h"
#include "lte_seq_host.h"
#include "phich_kernel.h"

using namespace srsran_amd;

namespace {

constexpr uint32_t kRows = 3;  // PHICH REs lie in symbols 0..2 (36.211 6.9.3)

struct PhichGpu {
  hipStream_t stream = nullptr;
  DevBuf<uint32_t> d_re;         // 12 indices per mapping unit of q->regs
  uint32_t    seq[10] = {};      // 12 scrambling bits per subframe
  // batches: items and (subframe, unit) groups on the device
  DevBuf<PhichItem> d_items;
  DevBuf<PhichUnit> d_units;     // same capacity
  // host-synchronous calls: control rows of the grids / estimates, noise, result
  DevBuf<float2>   d_grid;  // max(ports, rx) x kRows x nre
  DevBuf<float2>   d_ce;    // ports x rx x kRows x nre
  DevBuf<float>    d_noise;
  DevBuf<PhichOut> d_out;
  uint32_t  nre    = 0;  // of the cell the scratch was sized for
};

bool is_ext(const srsran_phich_t* q) { return q->cell.cp == SRSRAN_CP_EXT; }

// the reference's ngroups_phich: mapping units, x 2 with the extended CP (regs.c:351-353)
uint32_t ref_ngroups(const srsran_phich_t* q)
{
  return q->regs ? q->regs->ngroups_phich * (is_ext(q) ? 2u : 1u) : 0u;
}

int check_resource(const srsran_phich_t* q, srsran_phich_resource_t n)
{
  const uint32_t nseq_max = is_ext(q) ? SRSRAN_PHICH_EXT_NSEQUENCES : SRSRAN_PHICH_NORM_NSEQUENCES;
  if (n.nseq >= nseq_max) {
    fprintf(stderr, "[srsran_phich] Invalid nseq %u\n", n.nseq);
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (n.ngroup >= ref_ngroups(q)) {
    fprintf(stderr, "[srsran_phich] Invalid ngroup %u\n", n.ngroup);
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  return SRSRAN_SUCCESS;
}

void phich_free_gpu(PhichGpu* g)
{
  if (!g) {
    return;
  }
  if (g->stream) {
    hipStreamSynchronize(g->stream);
    hipStreamDestroy(g->stream);
  }
  delete g;
}

bool upload_regs(PhichGpu* g, const srsran_regs_t* regs)
{
  const uint32_t units = regs->ngroups_phich;
  if (12 * (size_t)units > g->d_re.cap()) {
    hipStreamSynchronize(g->stream);
    if (!g->d_re.reserve(12 * (size_t)units)) {
      return false;
    }
  }
  return units == 0 || (hipMemcpyAsync(g->d_re, regs->phich_re, 12 * (size_t)units * sizeof(uint32_t),
                                       hipMemcpyHostToDevice, g->stream) == hipSuccess &&
                        hipStreamSynchronize(g->stream) == hipSuccess);
}

// validates the items and turns them into device items; with `units`, also groups them by (subframe, unit) in put
// order.  The device copies are enqueued on `st`.
int stage_items(srsran_phich_t* q, uint32_t n, const srsran_phich_gpu_item_t* items, uint32_t nof_sf,
                std::vector<PhichUnit>* units, hipStream_t st)
{
  PhichGpu*              g = (PhichGpu*)q->gpu;
  std::vector<PhichItem> it(n);
  for (uint32_t i = 0; i < n; i++) {
    if (items[i].sf >= nof_sf) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (int r = check_resource(q, items[i].n_phich)) {
      return r;
    }
    const uint32_t ng = items[i].n_phich.ngroup;
    it[i] = {items[i].sf, is_ext(q) ? ng / 2 : ng, is_ext(q) ? ng % 2 : 0u, items[i].n_phich.nseq,
             g->seq[items[i].tti % 10], items[i].ack ? 1u : 0u};
  }
  if (units) {  // stable: a unit's items keep the order in which they were put
    std::stable_sort(it.begin(), it.end(), [](const PhichItem& a, const PhichItem& b) {
      return a.sf != b.sf ? a.sf < b.sf : a.unit < b.unit;
    });
    for (uint32_t i = 0; i < n; i++) {
      if (units->empty() || units->back().sf != it[i].sf || units->back().unit != it[i].unit) {
        units->push_back({it[i].sf, it[i].unit, i, 0});
      }
      units->back().count++;
    }
  }
  if (n > g->d_items.cap() || n > g->d_units.cap()) {
    hipDeviceSynchronize();  // an earlier batch on another stream may still read the buffers
    if (!g->d_items.reserve(n) || !g->d_units.reserve(n)) {
      return SRSRAN_ERROR;
    }
  }
  if (hipMemcpyAsync(g->d_items, it.data(), n * sizeof(PhichItem), hipMemcpyHostToDevice, st) != hipSuccess ||
      (units && hipMemcpyAsync(g->d_units, units->data(), units->size() * sizeof(PhichUnit), hipMemcpyHostToDevice,
                               st) != hipSuccess)) {
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

// scratch of the host-synchronous calls, sized for the cell
bool scratch(srsran_phich_t* q)
{
  PhichGpu*      g   = (PhichGpu*)q->gpu;
  const uint32_t nre = 12 * q->cell.nof_prb;
  if (g->nre == nre && g->d_grid) {
    return true;
  }
  hipStreamSynchronize(g->stream);
  g->d_grid.reset(), g->d_ce.reset();  // sized for the cell
  g->nre             = 0;
  const size_t plane = (size_t)kRows * nre;
  if (!g->d_grid.reserve(4 * plane) || !g->d_ce.reserve(16 * plane) || !g->d_noise.reserve(1) || !g->d_out.reserve(1)) {
    return false;
  }
  g->nre = nre;
  return true;
}

bool ready(const srsran_phich_t* q)
{
  return q && q->gpu && q->regs && q->cell.nof_prb &&
         (q->cell.nof_ports == 1 || q->cell.nof_ports == 2 || q->cell.nof_ports == 4);
}

}  // namespace

extern "C" {

int srsran_phich_init(srsran_phich_t* q, uint32_t nof_rx_antennas)
{
  if (!q || nof_rx_antennas == 0 || nof_rx_antennas > SRSRAN_MAX_PORTS) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  memset(q, 0, sizeof(*q));
  q->nof_rx_antennas = nof_rx_antennas;
  if (!have_gpu()) {
    fprintf(stderr, "[srsran_phich] no HIP device\n");
    return SRSRAN_ERROR;
  }
  PhichGpu* g = new PhichGpu();
  if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) {
    g->stream = nullptr;
    phich_free_gpu(g);
    return SRSRAN_ERROR;
  }
  q->gpu = g;
  return SRSRAN_SUCCESS;
}

void srsran_phich_free(srsran_phich_t* q)
{
  if (q) {
    phich_free_gpu((PhichGpu*)q->gpu);
    memset(q, 0, sizeof(*q));
  }
}

void srsran_phich_set_regs(srsran_phich_t* q, srsran_regs_t* regs)
{
  if (!q || !q->gpu || !regs) {
    return;
  }
  q->regs = upload_regs((PhichGpu*)q->gpu, regs) ? regs : nullptr;
}

int srsran_phich_set_cell(srsran_phich_t* q, srsran_regs_t* regs, srsran_cell_t cell)
{
  if (!q || !q->gpu || !regs || cell.nof_prb < 6 || cell.nof_prb > SRSRAN_MAX_PRB || cell.id >= 504 ||
      (cell.nof_ports != 1 && cell.nof_ports != 2 && cell.nof_ports != 4) ||
      (cell.cp != SRSRAN_CP_NORM && cell.cp != SRSRAN_CP_EXT)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PhichGpu* g = (PhichGpu*)q->gpu;
  q->cell     = cell;
  for (uint32_t sf = 0; sf < 10; sf++) {  // srsran_sequence_phich(2 * sf, cell.id)
    gold_words((sf + 1) * (2 * cell.id + 1) * 512 + cell.id, &g->seq[sf], 12);
  }
  srsran_phich_set_regs(q, regs);
  return q->regs ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

void srsran_phich_calc(srsran_phich_t* q, srsran_phich_grant_t* grant, srsran_phich_resource_t* n_phich)
{
  const uint32_t ngroups = q && q->regs ? q->regs->ngroups_phich_m1 : 0;
  if (!ngroups || !grant) {
    fprintf(stderr, "[srsran_phich] Error computing PHICH groups. Ngroups is zero\n");
    return;
  }
  if (n_phich) {
    n_phich->ngroup = (grant->n_prb_lowest + grant->n_dmrs) % ngroups + grant->I_phich * ngroups;
    n_phich->nseq   = ((grant->n_prb_lowest / ngroups) + grant->n_dmrs) % (2 * srsran_phich_nsf(q));
  }
}

uint32_t srsran_phich_ngroups(srsran_phich_t* q) { return q ? ref_ngroups(q) : 0; }

uint32_t srsran_phich_nsf(srsran_phich_t* q)
{
  return q && is_ext(q) ? SRSRAN_PHICH_EXT_NSF : SRSRAN_PHICH_NORM_NSF;
}

void srsran_phich_reset(srsran_phich_t* q, cf_t* slot_symbols[SRSRAN_MAX_PORTS])
{
  if (!q || !q->regs || !slot_symbols) {
    return;
  }
  for (int p = 0; p < SRSRAN_MAX_PORTS; p++) {
    for (uint32_t i = 0; slot_symbols[p] && i < 12 * q->regs->ngroups_phich; i++) {
      slot_symbols[p][q->regs->phich_re[i]] = 0;
    }
  }
}

void srsran_phich_ack_encode(uint8_t ack, uint8_t bits[SRSRAN_PHICH_NBITS])
{
  memset(bits, ack, SRSRAN_PHICH_NBITS);
}

uint8_t srsran_phich_ack_decode(float bits[SRSRAN_PHICH_NBITS], float* distance)
{
  const float c1 = ((bits[0] + bits[1]) + bits[2]) / SRSRAN_PHICH_NBITS, c0 = -c1;
  if (distance) {
    *distance = c1 > c0 ? c1 : c0;
  }
  return c1 > c0 ? 1 : 0;
}

int srsran_phich_gpu_encode_batch(srsran_phich_t* q, uint32_t nof_items, const srsran_phich_gpu_item_t* items,
                                  uint32_t nof_sf, cf_t* d_grids, void* stream)
{
  if (!ready(q) || (nof_items && (!items || !d_grids))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (nof_items == 0) {
    return SRSRAN_SUCCESS;
  }
  PhichGpu*              g = (PhichGpu*)q->gpu;
  std::vector<PhichUnit> units;
  if (int r = stage_items(q, nof_items, items, nof_sf, &units, (hipStream_t)stream)) {
    return r;
  }
  PhichTxArgs a{};
  a.items  = g->d_items;
  a.units  = g->d_units;
  a.re     = g->d_re;
  a.grids  = (float2*)d_grids;
  a.nports = q->cell.nof_ports;
  a.sf_re  = SRSRAN_SF_LEN_RE(q->cell.nof_prb, q->cell.cp);
  a.ext_cp = is_ext(q) ? 1u : 0u;
  return phich_tx_launch(a, (uint32_t)units.size(), (hipStream_t)stream) == hipSuccess ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

int srsran_phich_gpu_decode_batch(srsran_phich_t* q, uint32_t nof_items, const srsran_phich_gpu_item_t* items,
                                  uint32_t nof_sf, const cf_t* d_grids, const cf_t* d_ce, uint32_t ce_row_len,
                                  const float* d_noise, uint32_t noise_stride, srsran_phich_gpu_res_t* d_out,
                                  void* stream)
{
  if (!ready(q) || (nof_items && (!items || !d_grids || !d_ce || !d_noise || !d_out || ce_row_len == 0))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (nof_items == 0) {
    return SRSRAN_SUCCESS;
  }
  PhichGpu* g = (PhichGpu*)q->gpu;
  if (int r = stage_items(q, nof_items, items, nof_sf, nullptr, (hipStream_t)stream)) {
    return r;
  }
  PhichRxArgs a{};
  a.items        = g->d_items;
  a.re           = g->d_re;
  a.grids        = (const float2*)d_grids;
  a.ce           = (const float2*)d_ce;
  a.noise        = d_noise;
  a.out          = (PhichOut*)d_out;
  a.nports       = q->cell.nof_ports;
  a.nrx          = q->nof_rx_antennas;
  a.sf_re        = SRSRAN_SF_LEN_RE(q->cell.nof_prb, q->cell.cp);
  a.ce_row       = ce_row_len;
  a.noise_stride = noise_stride;
  a.ext_cp       = is_ext(q) ? 1u : 0u;
  return phich_rx_launch(a, nof_items, (hipStream_t)stream) == hipSuccess ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

int srsran_phich_encode(srsran_phich_t* q, srsran_dl_sf_cfg_t* sf, srsran_phich_resource_t n_phich, uint8_t ack,
                        cf_t* sf_symbols[SRSRAN_MAX_PORTS])
{
  if (!ready(q) || !sf || !sf_symbols) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (int r = check_resource(q, n_phich)) {
    return r;
  }
  PhichGpu*      g = (PhichGpu*)q->gpu;
  const uint32_t P = q->cell.nof_ports, unit = is_ext(q) ? n_phich.ngroup / 2 : n_phich.ngroup;
  for (uint32_t p = 0; p < P; p++) {
    if (!sf_symbols[p]) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  if (!scratch(q)) {
    return SRSRAN_ERROR;
  }
  // one item on a scratch "subframe" of kRows symbols a port; its 12 REs a port are then added on the host
  const srsran_phich_gpu_item_t it = {0, sf->tti, n_phich, ack};
  std::vector<PhichUnit>        units;
  const size_t                  plane = (size_t)kRows * g->nre;
  if (int r = stage_items(q, 1, &it, 1, &units, g->stream)) {
    return r;
  }
  PhichTxArgs a{};
  a.items  = g->d_items;
  a.units  = g->d_units;
  a.re     = g->d_re;
  a.grids  = g->d_grid;
  a.nports = P;
  a.sf_re  = (uint32_t)plane;
  a.ext_cp = is_ext(q) ? 1u : 0u;
  std::vector<float2> host(P * plane);
  if (phich_tx_launch(a, 1, g->stream) != hipSuccess ||
      hipMemcpyAsync(host.data(), g->d_grid, P * plane * sizeof(float2), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  for (uint32_t p = 0; p < P; p++) {  // srsran_regs_phich_add
    float2* dst = (float2*)sf_symbols[p];
    for (uint32_t e = 0; e < 12; e++) {
      const uint32_t idx = q->regs->phich_re[12 * unit + e];
      dst[idx].x += host[p * plane + idx].x;
      dst[idx].y += host[p * plane + idx].y;
    }
  }
  return SRSRAN_SUCCESS;
}

int srsran_phich_decode(srsran_phich_t* q, srsran_dl_sf_cfg_t* sf, srsran_chest_dl_res_t* channel,
                        srsran_phich_resource_t n_phich, cf_t* sf_symbols[SRSRAN_MAX_PORTS], srsran_phich_res_t* result)
{
  if (!ready(q) || !sf || !channel || !sf_symbols) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (int r = check_resource(q, n_phich)) {
    return r;
  }
  PhichGpu*      g = (PhichGpu*)q->gpu;
  const uint32_t P = q->cell.nof_ports, R = q->nof_rx_antennas;
  if (!scratch(q)) {
    return SRSRAN_ERROR;
  }
  const size_t plane = (size_t)kRows * g->nre;
  for (uint32_t r = 0; r < R; r++) {  // the control rows of the host grids and full-grid estimates
    if (!sf_symbols[r] || hipMemcpyAsync(g->d_grid + r * plane, sf_symbols[r], plane * sizeof(float2),
                                         hipMemcpyHostToDevice, g->stream) != hipSuccess) {
      return SRSRAN_ERROR;
    }
    for (uint32_t p = 0; p < P; p++) {
      if (!channel->ce[p][r] || hipMemcpyAsync(g->d_ce + (p * R + r) * plane, channel->ce[p][r], plane * sizeof(float2),
                                               hipMemcpyHostToDevice, g->stream) != hipSuccess) {
        return SRSRAN_ERROR;
      }
    }
  }
  const srsran_phich_gpu_item_t it = {0, sf->tti, n_phich, 0};
  PhichOut                      o{};
  if (hipMemcpyAsync(g->d_noise, &channel->noise_estimate, sizeof(float), hipMemcpyHostToDevice, g->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  if (int r = stage_items(q, 1, &it, 1, nullptr, g->stream)) {
    return r;
  }
  PhichRxArgs a{};
  a.items        = g->d_items;
  a.re           = g->d_re;
  a.grids        = g->d_grid;
  a.ce           = g->d_ce;
  a.noise        = g->d_noise;
  a.out          = g->d_out;
  a.nports       = P;
  a.nrx          = R;
  a.sf_re        = (uint32_t)plane;
  a.ce_row       = (uint32_t)plane;
  a.noise_stride = 0;
  a.ext_cp       = is_ext(q) ? 1u : 0u;
  if (phich_rx_launch(a, 1, g->stream) != hipSuccess ||
      hipMemcpyAsync(&o, g->d_out, sizeof(o), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  if (result) {
    result->ack_value = o.ack != 0;
    result->distance  = o.distance;
  }
  return SRSRAN_SUCCESS;
}

}  // extern "C"
