// srsran_4g_amd/csrc/chest_ul_api.cpp -- the UL channel estimator object (include/srsran_pusch.h; chest_ul.c:53-433,
// 612-647): srsran_chest_ul_t / srsran_chest_ul_res_t, the PUSCH estimator over pusch_kernel.hip and the SRS estimator
// over srs_kernel.hip.  srsran_chest_ul_estimate_pucch is in pucch_api.cpp, with its kernel's descriptors.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "srs_kernel.h"
#include "ul_internal.h"

using namespace srsran_amd;

namespace srsran_amd {

void fill_chest_desc(PuschUe& u, const srsran_chest_ul_t* q, const srsran_pusch_cfg_t* cfg, uint32_t M)
{
  u.ncell_re   = q->cell.nof_prb * SRSRAN_NRE;
  u.M          = M;
  u.nsym_slot  = nsymb_slot(q->cell.cp);
  u.n_tilde[0] = cfg->grant.n_prb_tilde[0];
  u.n_tilde[1] = cfg->grant.n_prb_tilde[1];
  u.n_prb[0]   = cfg->grant.n_prb[0];
  u.n_prb[1]   = cfg->grant.n_prb[1];
  u.smooth     = q->smooth_filter_len == 3;
  u.filt[0] = u.smooth ? q->smooth_filter[0] : 0.f;
  u.filt[1] = u.smooth ? q->smooth_filter[1] : 0.f;
  u.filt[2] = u.smooth ? q->smooth_filter[2] : 0.f;
  u.meas_ta    = cfg->meas_ta_en;
  // estimate_noise_pilots' calibration for the 3-tap filter (chest_ul.c:220-225)
  u.noise_div   = chest_ul_noise_div(q->smooth_filter[0]);
  u.noise_dev   = 1;
  u.dft_norm    = 1.0f / sqrtf((float)M);
}

void finish_chest_res(srsran_chest_ul_res_t* res, const ChestUlOut& o)
{
  res->noise_estimate      = o.noise;
  res->cfo_hz              = o.cfo_hz;
  res->ta_us               = o.ta_us;
  res->rsrp                = o.rsrp;
  res->epre                = o.epre;
  res->snr                 = isnormal(o.noise) ? o.epre / o.noise : NAN;
  res->epre_dBfs           = 10.0f * log10f(res->epre);
  res->rsrp_dBfs           = 10.0f * log10f(res->rsrp);
  res->snr_db              = 10.0f * log10f(res->snr);
  res->noise_estimate_dbFs = 10.0f * log10f(res->noise_estimate) + 30.0f;
}

hipStream_t chest_ul_stream(srsran_chest_ul_t* q) { return q && q->gpu ? ((ChestUlGpu*)q->gpu)->stream : nullptr; }

void* chest_ul_scratch(srsran_chest_ul_t* q, size_t bytes)
{
  ChestUlGpu* g = (ChestUlGpu*)q->gpu;
  return g->d_grid.reserve((bytes + sizeof(float2) - 1) / sizeof(float2)) ? (void*)g->d_grid.get() : nullptr;
}

void chest_ul_res_host_changed(srsran_chest_ul_res_t* res)
{
  if (res && res->gpu) {
    ((ChestUlResGpu*)res->gpu)->valid = false;
  }
}

}  // namespace srsran_amd

extern "C" {

// ---------------- chest_ul.c:53-204 ----------------
int srsran_chest_ul_init(srsran_chest_ul_t* q, uint32_t max_prb)
{
  if (!q || max_prb > SRSRAN_MAX_PRB) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  memset(q, 0, sizeof(*q));
  q->smooth_filter_len = 3;
  q->smooth_filter[0]  = 0.3333f;  // srsran_chest_set_smooth_filter3_coeff(.., 0.3333)
  q->smooth_filter[2]  = 0.3333f;
  q->smooth_filter[1]  = 1 - 2 * 0.3333f;
  ChestUlGpu* g        = new ChestUlGpu();
  g->max_prb           = max_prb;
  q->gpu               = g;
  if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) {
    srsran_chest_ul_free(q);
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

void srsran_chest_ul_free(srsran_chest_ul_t* q)
{
  if (!q) {
    return;
  }
  ChestUlGpu* g = (ChestUlGpu*)q->gpu;
  if (g) {
    if (g->stream) {
      hipStreamSynchronize(g->stream);
      hipStreamDestroy(g->stream);
    }
    delete g;
  }
  memset(q, 0, sizeof(*q));
}

int srsran_chest_ul_res_init(srsran_chest_ul_res_t* q, uint32_t max_prb)
{
  if (!q) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  memset(q, 0, sizeof(*q));
  q->nof_re = max_prb * SRSRAN_NRE * 2 * SRSRAN_CP_NORM_NSYMB;  // SRSRAN_SF_LEN_RE(max_prb, NORM)
  q->ce     = (cf_t*)calloc(q->nof_re ? q->nof_re : 1, sizeof(cf_t));
  if (!q->ce) {
    return SRSRAN_ERROR;
  }
  ChestUlResGpu* g = new ChestUlResGpu();
  g->nof_re        = q->nof_re;
  q->gpu           = g;
  if (!g->d_ce.reserve(std::max<uint32_t>(q->nof_re, 1)) ||
      hipMemset(g->d_ce, 0, (size_t)std::max<uint32_t>(q->nof_re, 1) * sizeof(float2)) != hipSuccess ||
      !g->d_out.reserve(1)) {
    srsran_chest_ul_res_free(q);
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

void srsran_chest_ul_res_set_identity(srsran_chest_ul_res_t* q)
{
  if (!q) {
    return;
  }
  for (uint32_t i = 0; i < q->nof_re; i++) {
    q->ce[i] = 1.0f;
  }
  ChestUlResGpu* g = (ChestUlResGpu*)q->gpu;
  if (g) {
    g->valid = false;  // the host copy is the current one
  }
}

void srsran_chest_ul_res_free(srsran_chest_ul_res_t* q)
{
  if (!q) {
    return;
  }
  free(q->ce);
  delete (ChestUlResGpu*)q->gpu;
  memset(q, 0, sizeof(*q));
}

int srsran_chest_ul_set_cell(srsran_chest_ul_t* q, srsran_cell_t cell)
{
  if (!q || !q->gpu || !cell_valid(cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChestUlGpu* g = (ChestUlGpu*)q->gpu;
  if (cell.id != q->cell.id || q->cell.nof_prb == 0 || !g->hop_ok || cell.cp != q->cell.cp) {
    q->cell = cell;
    hopping_tables(cell, g->hop);
    g->hop_ok = true;
  }
  q->cell = cell;
  return SRSRAN_SUCCESS;
}

void srsran_chest_ul_pregen(srsran_chest_ul_t* q, srsran_refsignal_dmrs_pusch_cfg_t* cfg, void* srs_cfg)
{
  if (!q || !q->gpu || !cfg || !((ChestUlGpu*)q->gpu)->hop_ok) {
    return;
  }
  ChestUlGpu* g = (ChestUlGpu*)q->gpu;
  if (srs_cfg) {  // chest_ul.c:200-203; the sequences themselves are formed by the estimator's kernel
    const srsran_refsignal_srs_cfg_t& sc = *(const srsran_refsignal_srs_cfg_t*)srs_cfg;
    if (srs_cfg_valid(sc, q->cell.nof_prb) && cfg->delta_ss < SRSRAN_NOF_DELTA_SS) {
      g->srs_cfg        = sc;
      g->srs_dmrs_cfg   = *cfg;
      g->srs_configured = true;
    } else {
      fprintf(stderr, "[srsran_chest_ul] Invalid SRS configuration: not recorded\n");
    }
  }
  // every (n_dmrs, subframe, valid L_prb <= cell PRB) sequence, as srsran_refsignal_dmrs_pusch_pregen
  const uint32_t nmax = std::min(q->cell.nof_prb, g->max_prb ? g->max_prb : q->cell.nof_prb);
  g->dmrs_off.assign(dmrs_index(SRSRAN_NOF_CSHIFT, 0, 0), (size_t)-1);
  size_t total = 0;
  for (uint32_t cs = 0; cs < SRSRAN_NOF_CSHIFT; cs++) {
    for (uint32_t sf = 0; sf < SRSRAN_NOF_SF_X_FRAME; sf++) {
      for (uint32_t n = 1; n <= nmax; n++) {
        if (srsran_dft_precoding_valid_prb(n)) {
          g->dmrs_off[dmrs_index(cs, sf, n)] = total;
          total += 2 * SRSRAN_NRE * n;
        }
      }
    }
  }
  std::vector<cf_t> h(std::max<size_t>(total, 1));
  for (uint32_t cs = 0; cs < SRSRAN_NOF_CSHIFT; cs++) {
    for (uint32_t sf = 0; sf < SRSRAN_NOF_SF_X_FRAME; sf++) {
      for (uint32_t n = 1; n <= nmax; n++) {
        const size_t o = g->dmrs_off[dmrs_index(cs, sf, n)];
        if (o != (size_t)-1) {
          dmrs_gen(q->cell, g->hop, *cfg, n, sf, cs, &h[o]);
        }
      }
    }
  }
  if (!g->d_dmrs.reserve(h.size()) ||
      hipMemcpy(g->d_dmrs, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) {
    fprintf(stderr, "[srsran_chest_ul] DMRS upload failed\n");
    return;
  }
  q->dmrs_cfg               = *cfg;
  q->dmrs_signal_configured = true;
}

int srsran_chest_ul_estimate_pusch(srsran_chest_ul_t*     q,
                                   srsran_ul_sf_cfg_t*    sf,
                                   srsran_pusch_cfg_t*    cfg,
                                   cf_t*                  input,
                                   srsran_chest_ul_res_t* res)
{
  if (!q || !q->gpu || !sf || !cfg || !input || !res || !res->gpu) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (!q->dmrs_signal_configured) {
    fprintf(stderr, "[srsran_chest_ul] Error must call srsran_chest_ul_set_cfg() before using the UL estimator\n");
    return SRSRAN_ERROR;
  }
  if (cfg->meas_ta_en && cfg->use_cedron_alg) {
    fprintf(stderr, "[srsran_chest_ul] the Cedron TA estimator is not provided\n");
    return SRSRAN_ERROR;
  }
  const uint32_t L = cfg->grant.L_prb;
  if (check_alloc(q->cell, cfg) != SRSRAN_SUCCESS) {
    fprintf(stderr, "[srsran_chest_ul] Error invalid nof_prb=%u\n", L);
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChestUlGpu*    g  = (ChestUlGpu*)q->gpu;
  ChestUlResGpu* rg = (ChestUlResGpu*)res->gpu;
  const uint32_t M = L * SRSRAN_NRE, ncell = q->cell.nof_prb * SRSRAN_NRE, nsf = 2 * nsymb_slot(q->cell.cp);
  const size_t   sf_re = (size_t)ncell * nsf;
  const size_t   off   = g->dmrs_off.empty() ? (size_t)-1 : g->dmrs_off[dmrs_index(cfg->grant.n_dmrs, sf->tti % 10, L)];
  if (off == (size_t)-1 || sf_re > rg->nof_re) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PuschUe u;
  memset(&u, 0, sizeof(u));
  fill_chest_desc(u, q, cfg, M);
  u.grid = g->d_grid;
  u.dmrs = g->d_dmrs + off;
  u.ce   = rg->d_ce;
  u.out  = rg->d_out;
  // the estimator writes the whole-slot rows of the allocation; bring the device copy in line with
  // the host's ce first when the host copy was changed (set_identity) so the rest matches on return
  if (!rg->valid) {
    if (hipMemcpyAsync(rg->d_ce, res->ce, sf_re * sizeof(float2), hipMemcpyHostToDevice, g->stream) != hipSuccess) {
      return SRSRAN_ERROR;
    }
  }
  if (!g->d_grid.reserve(sf_re) ||
      !g->d_desc.reserve(1)) {
    return SRSRAN_ERROR;
  }
  u.grid = g->d_grid;
  ChestUlOut o;
  if (hipMemcpyAsync(g->d_grid, input, sf_re * sizeof(float2), hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemcpyAsync(g->d_desc, &u, sizeof(u), hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      chest_ul_launch(g->d_desc, 1, g->stream) != hipSuccess ||
      hipMemcpyAsync(&o, rg->d_out, sizeof(o), hipMemcpyDeviceToHost, g->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  // the written rows back to the host estimate (other REs keep their contents, as in the reference)
  for (uint32_t s = 0; s < 2; s++) {
    const size_t o0 = (size_t)s * nsymb_slot(q->cell.cp) * ncell + cfg->grant.n_prb[s] * SRSRAN_NRE;
    if (hipMemcpy2DAsync(res->ce + o0, ncell * sizeof(float2), rg->d_ce + o0, ncell * sizeof(float2),
                         M * sizeof(float2), nsymb_slot(q->cell.cp), hipMemcpyDeviceToHost, g->stream) != hipSuccess) {
      return SRSRAN_ERROR;
    }
  }
  if (hipStreamSynchronize(g->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  rg->valid = true;
  finish_chest_res(res, o);
  return SRSRAN_SUCCESS;
}

// ---------------- chest_ul.c:612-647 ----------------
int srsran_chest_ul_gpu_estimate_srs_batch(uint32_t nof_ue, const srsran_chest_ul_gpu_srs_t* ues, void* stream)
{
  if (nof_ue == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!ues) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  hipStream_t          st = (hipStream_t)stream;
  std::vector<SrsRxUe> desc(nof_ue);
  for (uint32_t i = 0; i < nof_ue; i++) {
    const srsran_chest_ul_gpu_srs_t& e = ues[i];
    if (!e.q || !e.q->gpu || !e.sf || !e.cfg || !e.pusch_cfg || !e.d_sf_symbols || !e.res || !e.res->gpu ||
        !((ChestUlGpu*)e.q->gpu)->hop_ok) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    for (uint32_t k = 0; k < i; k++) {
      if (ues[k].res == e.res) {
        return SRSRAN_ERROR_INVALID_INPUTS;
      }
    }
    const srsran_chest_ul_t* q  = e.q;
    ChestUlGpu*              g  = (ChestUlGpu*)q->gpu;
    ChestUlResGpu*           rg = (ChestUlResGpu*)e.res->gpu;
    const srsran_cell_t&     cell = q->cell;
    if (!srs_cfg_valid(*e.cfg, cell.nof_prb) || e.pusch_cfg->delta_ss >= SRSRAN_NOF_DELTA_SS) {
      fprintf(stderr, "[srsran_chest_ul] Invalid SRS configuration\n");
      return SRSRAN_ERROR;
    }
    const uint32_t ncell = cell.nof_prb * SRSRAN_NRE, nsym = 2 * nsymb_slot(cell.cp);
    const uint32_t M_sc = srs_M_sc(*e.cfg, cell.nof_prb), k0 = srs_k0(*e.cfg, cell.nof_prb, e.sf->tti);
    const size_t   off  = (size_t)SRSRAN_REFSIGNAL_UL_L(0, cell.cp) * ncell;
    if (M_sc > SRS_MAX_M_SC || k0 + 2 * (M_sc - 1) >= ncell || off + M_sc > rg->nof_re || (size_t)ncell * nsym > rg->nof_re) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    // the known pilots: generated from the call's configurations, or those srsran_chest_ul_pregen recorded
    const srsran_refsignal_srs_cfg_t&        kc = g->srs_configured ? g->srs_cfg : *e.cfg;
    const srsran_refsignal_dmrs_pusch_cfg_t& kd = g->srs_configured ? g->srs_dmrs_cfg : *e.pusch_cfg;
    if (g->srs_configured && srs_M_sc(kc, cell.nof_prb) != M_sc) {
      fprintf(stderr, "[srsran_chest_ul] SRS of %u subcarriers against pregenerated sequences of %u\n", M_sc,
              srs_M_sc(kc, cell.nof_prb));
      return SRSRAN_ERROR;
    }
    SrsRxUe& u = desc[i];
    memset(&u, 0, sizeof(u));
    u.grid     = (const float2*)e.d_sf_symbols;
    u.ce       = rg->d_ce + off;
    u.out      = rg->d_out;
    u.ncell_re = ncell;
    u.nsym     = nsym;
    u.k0       = k0;
    u.m_sc     = M_sc;
    u.smooth   = q->smooth_filter_len == 3;
    for (int k = 0; k < 3; k++) {
      u.filt[k] = u.smooth ? q->smooth_filter[k] : 0.f;
    }
    u.noise_div   = chest_ul_noise_div(q->smooth_filter[0]);
    u.seq         = srs_seq(cell, g->hop, kc.n_srs, kd, M_sc, e.sf->tti % SRSRAN_NOF_SF_X_FRAME);
  }
  ChestUlGpu* g0 = (ChestUlGpu*)ues[0].q->gpu;
  if (!g0->d_srs_desc.reserve(desc.size() * sizeof(SrsRxUe))) {
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < nof_ue; i++) {  // the device estimate in line with the host's where the host's is newer
    ChestUlResGpu* rg = (ChestUlResGpu*)ues[i].res->gpu;
    if (!rg->valid && hipMemcpyAsync(rg->d_ce, ues[i].res->ce, (size_t)rg->nof_re * sizeof(float2), hipMemcpyHostToDevice,
                                     st) != hipSuccess) {
      return SRSRAN_ERROR;
    }
  }
  if (hipMemcpyAsync(g0->d_srs_desc, desc.data(), desc.size() * sizeof(SrsRxUe), hipMemcpyHostToDevice, st) != hipSuccess ||
      srs_chest_launch((const SrsRxUe*)g0->d_srs_desc.get(), nof_ue, st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < nof_ue; i++) {
    ChestUlResGpu* rg = (ChestUlResGpu*)ues[i].res->gpu;
    rg->srs_pending   = true;
    rg->srs_off       = (size_t)(desc[i].ce - rg->d_ce.get());
    rg->srs_n         = desc[i].m_sc;
    rg->valid         = true;
  }
  return SRSRAN_SUCCESS;
}

int srsran_chest_ul_gpu_srs_result(srsran_chest_ul_res_t* res)
{
  if (!res || !res->gpu || !res->ce) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChestUlResGpu* rg = (ChestUlResGpu*)res->gpu;
  if (!rg->srs_pending) {
    return SRSRAN_ERROR;
  }
  ChestUlOut o;
  if (hipMemcpy(&o, rg->d_out, sizeof(o), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(res->ce + rg->srs_off, rg->d_ce + rg->srs_off, rg->srs_n * sizeof(float2), hipMemcpyDeviceToHost) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  rg->srs_pending = false;
  finish_chest_res(res, o);
  return SRSRAN_SUCCESS;
}

int srsran_chest_ul_estimate_srs(srsran_chest_ul_t*                 q,
                                 srsran_ul_sf_cfg_t*                sf,
                                 srsran_refsignal_srs_cfg_t*        cfg,
                                 srsran_refsignal_dmrs_pusch_cfg_t* pusch_cfg,
                                 cf_t*                              input,
                                 srsran_chest_ul_res_t*             res)
{
  if (!q || !q->gpu || !sf || !cfg || !pusch_cfg || !input || !res || !res->gpu) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  ChestUlGpu*  g     = (ChestUlGpu*)q->gpu;
  const size_t sf_re = (size_t)q->cell.nof_prb * SRSRAN_NRE * 2 * nsymb_slot(q->cell.cp);
  if (sf_re == 0 || !g->d_grid.reserve(sf_re) ||
      hipMemcpyAsync(g->d_grid, input, sf_re * sizeof(float2), hipMemcpyHostToDevice, g->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  srsran_chest_ul_gpu_srs_t e = {q, sf, cfg, pusch_cfg, (const cf_t*)g->d_grid.get(), res};
  int                       ret = srsran_chest_ul_gpu_estimate_srs_batch(1, &e, g->stream);
  if (hipStreamSynchronize(g->stream) != hipSuccess) {
    ret = SRSRAN_ERROR;
  }
  if (ret != SRSRAN_SUCCESS) {
    return ret == SRSRAN_ERROR_INVALID_INPUTS ? ret : SRSRAN_ERROR;
  }
  return srsran_chest_ul_gpu_srs_result(res);
}

}  // extern "C"
