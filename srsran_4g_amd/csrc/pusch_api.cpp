// srsran_4g_amd/csrc/pusch_api.cpp -- srsran_pusch_t (include/srsran_pusch.h; pusch.c:108-471): PUSCH receive, its
// batch, and srsran_pusch_encode, over the kernels of pusch_kernel.hip, llr_kernel.hip, pusch_tx_kernel.hip and the
// UL-SCH coder of ulsch_api.cpp; and the transform precoder's entry points (dft_precoding.c).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "llr_kernel.h"
#include "sch_internal.h"
#include "ul_internal.h"

using namespace srsran_amd;

namespace {

// inverse-DFT plan: radices 4, 2, 3, 5 (M = 12 L, L = 2^a 3^b 5^c)
bool dft_plan(uint32_t M, PuschUe& u)
{
  u.nstages = 0;
  uint32_t n = M;
  for (uint32_t R : {4u, 2u, 3u, 5u}) {
    while (n % R == 0) {
      if (u.nstages == PUSCH_MAX_STAGES) {
        return false;
      }
      u.radix[u.nstages++] = (uint8_t)R;
      n /= R;
    }
  }
  return n == 1;
}

// the PUSCH data symbols of the subframe (pusch_cp, pusch.c:48-95)
uint32_t data_symbols(srsran_cp_t cp, bool shortened, uint8_t* out)
{
  const uint32_t ns = nsymb_slot(cp), L_ref = cp == SRSRAN_CP_NORM ? 3 : 2;
  uint32_t       n  = 0;
  for (uint32_t slot = 0; slot < 2; slot++) {
    const uint32_t n_srs = (shortened && slot == 1) ? 1 : 0;
    for (uint32_t l = 0; l < ns - n_srs; l++) {
      if (l != L_ref) {
        out[n++] = (uint8_t)(l + slot * ns);
      }
    }
  }
  return n;
}

// ---------------- PUSCH device state ----------------
struct PuschGpu {
  DevBuf<float2>     d_grid;  // subframe grid (sync API)
  DevBuf<float2>     d_ce;    // estimate grid uploaded from the host (sync API, channel->gpu absent)
  DevBuf<float2>     d_sym;   // de-precoded symbols
  DevBuf<int16_t>    d_q;     // LLRs
  DevBuf<uint8_t>    d_c;     // unpacked scrambling sequence
  DevBuf<PuschUe>    d_desc;
  DevBuf<LlrItem>    d_llr;
  DevBuf<ChestUlOut> d_out;   // per-UE outputs (sync API: one; batch: nof_ue)
  DevBuf<float2>     d_bce;   // batch: per-UE estimate grids
  DevBuf<int16_t>    d_g;     // batch: de-interleaved LLRs of the UEs without UCI
  DevBuf<uint8_t>    d_data;  // batch: decoded TBs of the UEs without UCI
  uint32_t    last_nsym = 0, last_nllr = 0;  // the last host-sync decode's counts (srsran_pusch_gpu_last_soft)
  DevBuf<uint8_t>    d_tx;      // transmit: descriptors and DMRS values of a batch
  DevBuf<uint8_t>    d_txdata;  // transmit (sync API): the payload
};

uint32_t pusch_seed(uint16_t rnti, uint32_t nslot, uint32_t cell_id)  // sequences.c:119-122
{
  return ((uint32_t)rnti << 14) + ((nslot / 2) << 9) + cell_id;
}

// pusch.c:374-380
void limit_64qam(srsran_pusch_cfg_t* cfg)
{
  if (!cfg->enable_64qam && cfg->grant.tb.mod >= SRSRAN_MOD_64QAM) {
    cfg->grant.tb.mod      = SRSRAN_MOD_16QAM;
    cfg->grant.tb.nof_bits = cfg->grant.nof_re * 4;
  }
}

bool any_uci(const srsran_pusch_cfg_t* cfg)
{
  return srsran_uci_cfg_total_ack(&cfg->uci_cfg) > 0 || cfg->uci_cfg.cqi.ri_len > 0 || cfg->uci_cfg.cqi.data_enable;
}

}  // namespace

namespace srsran_amd {

int check_alloc(const srsran_cell_t& cell, const srsran_pusch_cfg_t* cfg)
{
  const uint32_t L = cfg->grant.L_prb;
  if (!srsran_dft_precoding_valid_prb(L) || L > cell.nof_prb) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  for (int s = 0; s < 2; s++) {
    if (cfg->grant.n_prb_tilde[s] + L > cell.nof_prb || cfg->grant.n_prb[s] + L > cell.nof_prb) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  if (cfg->grant.n_dmrs >= SRSRAN_NOF_CSHIFT) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  return SRSRAN_SUCCESS;
}

// ---------------- PUSCH transmit (pusch.c:178-181, 259-354) ----------------
// srsran_pusch_encode for n transmissions up to the grids: checks, the UL-SCH step, then one multiplexing launch and
// one transform-precoding launch over the batch.  desc / *d_desc: the descriptors (host copy, device array in
// owner's scratch) for the caller's later stages.  Nothing is launched when a transmission is refused.  extra:
// descriptors of the batch's other transmissions (PUCCH), appended after the n of PUSCH for the normalisation launch.
int pusch_tx_run(srsran_pusch_t* owner, uint32_t n, const TxReq* r, std::vector<PuschTxUe>& desc,
                 const PuschTxUe** d_desc, hipStream_t st, const std::vector<PuschTxUe>& extra)
{
  PuschGpu* g = (PuschGpu*)owner->gpu;
  desc.assign(n, PuschTxUe{});
  std::vector<UlschTxJob> jobs(n);
  std::vector<cf_t>       dmrs;
  std::vector<size_t>     dmrs_off(n, 0);
  uint32_t                max_H = 0;
  for (uint32_t i = 0; i < n; i++) {
    srsran_pusch_t*     q   = r[i].pusch;
    srsran_pusch_cfg_t* cfg = r[i].cfg;
    if (!q || !q->gpu || !cfg || !r[i].sf || !r[i].d_grid) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    limit_64qam(cfg);
    if (cfg->grant.nof_re > q->max_re) {
      fprintf(stderr, "[srsran_pusch] Error too many RE per subframe (%u). PUSCH configured for %u RE (%u PRB)\n",
              cfg->grant.nof_re, q->max_re, q->cell.nof_prb);
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    const int err = srsran_pusch_assert_grant(&cfg->grant);
    if (err != SRSRAN_SUCCESS) {
      return err;
    }
    if (check_alloc(q->cell, cfg) != SRSRAN_SUCCESS) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    PuschTxUe&     u = desc[i];
    const uint32_t L = cfg->grant.L_prb, M = L * SRSRAN_NRE;
    u.nof_symb       = data_symbols(q->cell.cp, r[i].sf->shortened, u.data_sym);
    if (u.nof_symb * M != cfg->grant.nof_re) {
      fprintf(stderr, "[srsran_pusch] Error trying to allocate %u symbols but %u were allocated (tti=%u, short=%d, L=%u)\n",
              cfg->grant.nof_re, u.nof_symb * M, r[i].sf->tti, (int)r[i].sf->shortened, L);
      return SRSRAN_ERROR;
    }
    const uint32_t Qm = srsran_mod_bits_x_symbol(cfg->grant.tb.mod);
    PuschUe        plan;
    if (Qm == 0 || cfg->grant.tb.nof_bits != cfg->grant.nof_re * Qm || cfg->grant.nof_symb != u.nof_symb ||
        !dft_plan(M, plan)) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    memcpy(u.radix, plan.radix, sizeof(u.radix));
    u.nstages    = plan.nstages;
    u.grid       = r[i].d_grid;
    u.ncell_re   = q->cell.nof_prb * SRSRAN_NRE;
    u.M          = M;
    u.nsym_slot  = nsymb_slot(q->cell.cp);
    u.n_tilde[0] = cfg->grant.n_prb_tilde[0];
    u.n_tilde[1] = cfg->grant.n_prb_tilde[1];
    u.dft_norm   = 1.0f / sqrtf((float)M);
    u.zero_rest  = r[i].zero_rest;
    u.seed       = pusch_seed(cfg->rnti, 2 * (r[i].sf->tti % SRSRAN_NOF_SF_X_FRAME), q->cell.id);
    u.samples_in  = r[i].samples_in;
    u.samples_out = r[i].samples_out;
    u.sf_len      = r[i].sf_len;
    u.norm_mode   = r[i].norm_mode;
    u.norm_factor = r[i].norm_factor;
    u.force_peak  = r[i].force_peak;
    if (r[i].hop) {
      u.put_dmrs  = 1;
      dmrs_off[i] = dmrs.size();
      dmrs.resize(dmrs.size() + 2 * M);
      if (dmrs_gen(q->cell, *r[i].hop, *r[i].dmrs_cfg, L, r[i].sf->tti % SRSRAN_NOF_SF_X_FRAME, cfg->grant.n_dmrs,
                   dmrs.data() + dmrs_off[i]) != SRSRAN_SUCCESS) {
        fprintf(stderr, "[srsran_ue_ul] Error generating PUSCH DMRS signals\n");
        return SRSRAN_ERROR_INVALID_INPUTS;
      }
    }
    jobs[i] = {cfg, r[i].uci, r[i].d_data, false, false, 0};
    max_H   = std::max(max_H, cfg->grant.nof_re);
  }
  if (n && ulsch_tx_prepare(&owner->ul_sch, n, jobs.data(), desc.data(), st) != SRSRAN_SUCCESS) {
    fprintf(stderr, "[srsran_pusch] Error encoding TB\n");
    return SRSRAN_ERROR;
  }
  desc.insert(desc.end(), extra.begin(), extra.end());
  const size_t o_dmrs = (desc.size() * sizeof(PuschTxUe) + 15) & ~(size_t)15;
  if (!g->d_tx.reserve(o_dmrs + dmrs.size() * sizeof(cf_t))) {
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < n; i++) {
    desc[i].dmrs = (const float2*)(g->d_tx + o_dmrs) + dmrs_off[i];
  }
  *d_desc = (const PuschTxUe*)g->d_tx.get();
  if (hipMemcpyAsync(g->d_tx, desc.data(), desc.size() * sizeof(PuschTxUe), hipMemcpyHostToDevice, st) != hipSuccess ||
      (!dmrs.empty() && hipMemcpyAsync(g->d_tx + o_dmrs, dmrs.data(), dmrs.size() * sizeof(cf_t), hipMemcpyHostToDevice,
                                       st) != hipSuccess) ||
      pusch_tx_mux_launch(*d_desc, n, max_H, st) != hipSuccess || pusch_tx_grid_launch(*d_desc, n, st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

}  // namespace srsran_amd

extern "C" {

bool srsran_dft_precoding_valid_prb(uint32_t nof_prb)
{
  // 36.213 14.1.1.4C: L_prb = 2^a 3^b 5^c (dft_precoding.c:88-103)
  if (nof_prb == 0 || nof_prb > 100) {
    return nof_prb == 0;
  }
  uint32_t n = nof_prb;
  for (uint32_t p : {2u, 3u, 5u}) {
    while (n % p == 0) {
      n /= p;
    }
  }
  return n == 1;
}

uint32_t srsran_dft_precoding_get_valid_prb(uint32_t nof_prb)
{
  while (!srsran_dft_precoding_valid_prb(nof_prb)) {
    nof_prb--;
  }
  return nof_prb;
}

int srsran_dft_precoding_gpu(const cf_t* d_input, cf_t* d_output, uint32_t nof_prb, uint32_t nof_symbols, void* stream)
{
  if (!d_input || !d_output || nof_prb == 0 || !srsran_dft_precoding_valid_prb(nof_prb) || nof_symbols == 0 ||
      nof_symbols > 14) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PuschUe u;
  memset(&u, 0, sizeof(u));
  const uint32_t M = nof_prb * SRSRAN_NRE;
  if (!dft_plan(M, u)) {
    return SRSRAN_ERROR;
  }
  u.grid      = (const float2*)d_input;
  u.sym       = (float2*)d_output;
  u.ncell_re  = M;
  u.M         = M;
  u.nsym_slot = 14;
  u.nof_symb  = nof_symbols;
  for (uint32_t l = 0; l < nof_symbols; l++) {
    u.data_sym[l] = (uint8_t)l;
  }
  u.dft_norm     = 1.0f / sqrtf((float)M);
  hipStream_t st = (hipStream_t)stream;
  PuschUe*    d  = nullptr;
  // the descriptor travels as a kernel-visible copy: one small allocation per call, freed in order
  if (hipMallocAsync((void**)&d, sizeof(u), st) != hipSuccess ||
      hipMemcpyAsync(d, &u, sizeof(u), hipMemcpyHostToDevice, st) != hipSuccess ||
      pusch_eq_idft_launch(d, 1, st) != hipSuccess || hipFreeAsync(d, st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

// ---------------- pusch.c:108-471 ----------------
int srsran_pusch_init_enb(srsran_pusch_t* q, uint32_t max_prb)
{
  if (!q || max_prb > SRSRAN_MAX_PRB) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  memset(q, 0, sizeof(*q));
  q->is_ue  = false;
  q->max_re = max_prb * 2 * SRSRAN_CP_NORM_NSYMB * SRSRAN_NRE;  // MAX_PUSCH_RE(NORM) * max_prb
  if (srsran_sch_init(&q->ul_sch)) {
    return SRSRAN_ERROR;
  }
  q->gpu = new PuschGpu();
  if (sch_own_queue(&q->ul_sch)) {  // one hardware queue per PUSCH object (= per PHY worker)
    srsran_pusch_free(q);
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

void srsran_pusch_free(srsran_pusch_t* q)
{
  if (!q) {
    return;
  }
  PuschGpu* g = (PuschGpu*)q->gpu;
  if (g) {
    hipStream_t st = sch_stream(&q->ul_sch);
    if (st) {
      hipStreamSynchronize(st);
    }
    delete g;
  }
  srsran_sch_free(&q->ul_sch);
  memset(q, 0, sizeof(*q));
}

int srsran_pusch_set_cell(srsran_pusch_t* q, srsran_cell_t cell)
{
  if (!q || !cell_valid(cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  q->cell   = cell;
  q->max_re = cell.nof_prb * 2 * nsymb_slot(cell.cp) * SRSRAN_NRE;
  return SRSRAN_SUCCESS;
}

int srsran_pusch_assert_grant(const srsran_pusch_grant_t* grant)
{
  if (!srsran_dft_precoding_valid_prb(grant->L_prb)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (grant->tb.rv < -1 || grant->tb.rv > 3) {
    return SRSRAN_ERROR_OUT_OF_BOUNDS;
  }
  if (grant->tb.tbs < 0) {
    return SRSRAN_ERROR_OUT_OF_BOUNDS;
  }
  return SRSRAN_SUCCESS;
}

int srsran_pusch_decode(srsran_pusch_t*        q,
                        srsran_ul_sf_cfg_t*    sf,
                        srsran_pusch_cfg_t*    cfg,
                        srsran_chest_ul_res_t* channel,
                        cf_t*                  sf_symbols,
                        srsran_pusch_res_t*    out)
{
  if (!q || !q->gpu || !sf || !sf_symbols || !out || !cfg || !channel) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (q->llr_is_8bit) {
    fprintf(stderr, "[srsran_pusch] the 8-bit LLR path is not provided\n");
    return SRSRAN_ERROR;
  }
  ((PuschGpu*)q->gpu)->last_nsym = ((PuschGpu*)q->gpu)->last_nllr = 0;  // set again when this decode has run
  limit_64qam(cfg);
  const uint32_t L = cfg->grant.L_prb, M = L * SRSRAN_NRE;
  if (check_alloc(q->cell, cfg) != SRSRAN_SUCCESS) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PuschUe u;
  memset(&u, 0, sizeof(u));
  u.nof_symb = data_symbols(q->cell.cp, sf->shortened, u.data_sym);
  if (u.nof_symb * M != cfg->grant.nof_re) {
    fprintf(stderr, "[srsran_pusch] Error expecting %u symbols but got %u\n", cfg->grant.nof_re, u.nof_symb * M);
    return SRSRAN_ERROR;
  }
  const uint32_t Qm = srsran_mod_bits_x_symbol(cfg->grant.tb.mod);
  if (Qm == 0 || cfg->grant.tb.nof_bits != cfg->grant.nof_re * Qm || !dft_plan(M, u)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PuschGpu*      g     = (PuschGpu*)q->gpu;
  hipStream_t    st    = sch_stream(&q->ul_sch);
  const uint32_t ncell = q->cell.nof_prb * SRSRAN_NRE, nsf = 2 * nsymb_slot(q->cell.cp);
  const size_t   sf_re = (size_t)ncell * nsf;
  const uint32_t nb    = cfg->grant.tb.nof_bits;
  if (!g->d_grid.reserve(sf_re) ||
      !g->d_sym.reserve((size_t)cfg->grant.nof_re) ||
      !g->d_q.reserve((size_t)nb) ||
      !g->d_c.reserve((size_t)nb) || !g->d_desc.reserve(1) ||
      !g->d_out.reserve(1)) {
    return SRSRAN_ERROR;
  }
  // the estimate: the estimator's device copy when it is current, else the host's ce
  ChestUlResGpu* rg = (ChestUlResGpu*)channel->gpu;
  const float2*  d_ce;
  if (rg && rg->valid && rg->nof_re >= sf_re) {
    d_ce = rg->d_ce;
  } else {
    if (!channel->ce || !g->d_ce.reserve(sf_re) ||
        hipMemcpyAsync(g->d_ce, channel->ce, sf_re * sizeof(float2), hipMemcpyHostToDevice, st) != hipSuccess) {
      return SRSRAN_ERROR;
    }
    d_ce = g->d_ce;
  }
  u.grid       = g->d_grid;
  u.ce         = (float2*)d_ce;
  u.sym        = g->d_sym;
  u.out        = g->d_out;
  u.ncell_re   = ncell;
  u.M          = M;
  u.nsym_slot  = nsymb_slot(q->cell.cp);
  u.n_tilde[0] = cfg->grant.n_prb_tilde[0];
  u.n_tilde[1] = cfg->grant.n_prb_tilde[1];
  u.noise      = channel->noise_estimate;
  u.dft_norm = 1.0f / sqrtf((float)M);
  LlrItem it{};
  memset(&it, 0, sizeof(it));
  it.sym         = (const float*)g->d_sym.get();
  it.llr         = g->d_q;
  it.n           = cfg->grant.nof_re;
  it.seed        = pusch_seed(cfg->rnti, 2 * (sf->tti % SRSRAN_NOF_SF_X_FRAME), q->cell.id);
  it.scramble    = 1;
  const bool uci = any_uci(cfg);
  if (!g->d_llr.reserve(1) ||
      hipMemcpyAsync(g->d_grid, sf_symbols, sf_re * sizeof(float2), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(g->d_desc, &u, sizeof(u), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(g->d_llr, &it, sizeof(it), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(g->d_out, 0, sizeof(ChestUlOut), st) != hipSuccess ||
      pusch_eq_idft_launch(g->d_desc, 1, st) != hipSuccess ||
      llr_batch_launch((int)cfg->grant.tb.mod, g->d_llr, 1, it.n, 1, st) != hipSuccess ||
      (uci && seq_unpack_launch(g->d_c, nb, it.seed, st) != hipSuccess)) {
    return SRSRAN_ERROR;
  }
  srsran_sch_set_max_noi(&q->ul_sch, cfg->max_nof_iterations);
  const int ret = ulsch_decode_dev(&q->ul_sch, cfg, g->d_q, uci ? g->d_c : nullptr, out->data, &out->uci);
  ChestUlOut o;
  if (hipMemcpyAsync(&o, g->d_out, sizeof(o), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  out->epre_dbfs            = cfg->meas_epre_en ? 10.0f * log10f(o.data_pow / (float)cfg->grant.nof_re) : NAN;
  out->evm                  = NAN;
  out->crc                  = ret == 0;
  out->avg_iterations_block = q->ul_sch.avg_iterations;
  cfg->last_O_cqi           = (uint32_t)srsran_cqi_size(&cfg->uci_cfg.cqi);
  g->last_nsym              = cfg->grant.nof_re;
  g->last_nllr              = nb;
  return SRSRAN_SUCCESS;
}

int srsran_pusch_gpu_last_soft(srsran_pusch_t* q, const cf_t** d_sym, uint32_t* nof_sym, const int16_t** d_llr,
                               uint32_t* nof_llr)
{
  if (!q || !q->gpu || !d_sym || !nof_sym || !d_llr || !nof_llr) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PuschGpu* g = (PuschGpu*)q->gpu;
  if (g->last_nsym == 0) {  // no host-sync decode yet, or a batch has reused the buffers since
    return SRSRAN_ERROR;
  }
  *d_sym   = (const cf_t*)g->d_sym.get();
  *nof_sym = g->last_nsym;
  *d_llr   = g->d_q;
  *nof_llr = g->last_nllr;
  return SRSRAN_SUCCESS;
}

int srsran_pusch_gpu_decode_batch(srsran_pusch_t*              q,
                                  uint32_t                     nof_ue,
                                  const srsran_pusch_gpu_ue_t* ues,
                                  srsran_chest_ul_res_t*       chest_res,
                                  srsran_pusch_res_t*          res)
{
  if (!q || !q->gpu || (nof_ue && (!ues || !res))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (nof_ue == 0) {
    return SRSRAN_SUCCESS;
  }
  if (q->llr_is_8bit) {
    return SRSRAN_ERROR;
  }
  PuschGpu*   g  = (PuschGpu*)q->gpu;
  hipStream_t st = sch_stream(&q->ul_sch);
  g->last_nsym = g->last_nllr = 0;  // the symbol / LLR buffers are laid out per UE from here on

  // ---- host: descriptors and the device layout of every UE's buffers ----
  std::vector<PuschUe> desc(nof_ue);
  std::vector<size_t>  ce_off(nof_ue), sym_off(nof_ue), q_off(nof_ue), c_off(nof_ue);
  size_t               ce_tot = 0, sym_tot = 0, q_tot = 0, c_tot = 0;
  for (uint32_t i = 0; i < nof_ue; i++) {
    const srsran_pusch_gpu_ue_t& e = ues[i];
    if (!e.chest || !e.chest->gpu || !e.sf || !e.cfg || !e.d_sf_symbols || !e.chest->dmrs_signal_configured) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    srsran_pusch_cfg_t* cfg = e.cfg;
    const srsran_cell_t& cell = e.chest->cell;
    ChestUlGpu*          cg   = (ChestUlGpu*)e.chest->gpu;
    limit_64qam(cfg);
    if (check_alloc(cell, cfg) != SRSRAN_SUCCESS || (cfg->meas_ta_en && cfg->use_cedron_alg)) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    const uint32_t L = cfg->grant.L_prb, M = L * SRSRAN_NRE;
    PuschUe&       u = desc[i];
    memset(&u, 0, sizeof(u));
    fill_chest_desc(u, e.chest, cfg, M);
    u.nof_symb = data_symbols(cell.cp, e.sf->shortened, u.data_sym);
    const uint32_t Qm = srsran_mod_bits_x_symbol(cfg->grant.tb.mod);
    const size_t   off = cg->dmrs_off.empty() ? (size_t)-1 : cg->dmrs_off[dmrs_index(cfg->grant.n_dmrs, e.sf->tti % 10, L)];
    if (u.nof_symb * M != cfg->grant.nof_re || Qm == 0 || cfg->grant.tb.nof_bits != cfg->grant.nof_re * Qm ||
        !dft_plan(M, u) || off == (size_t)-1) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    u.grid     = (const float2*)e.d_sf_symbols;
    u.dmrs     = cg->d_dmrs + off;
    ce_off[i]  = ce_tot;
    ce_tot += (size_t)u.ncell_re * 2 * u.nsym_slot;
    sym_off[i] = sym_tot;
    sym_tot += cfg->grant.nof_re;
    q_off[i] = q_tot;
    q_tot += (cfg->grant.tb.nof_bits + 7) & ~7u;
    c_off[i] = c_tot;
    c_tot += any_uci(cfg) ? ((cfg->grant.tb.nof_bits + 15) & ~15u) : 0;
  }
  if (!g->d_desc.reserve(nof_ue) ||
      !g->d_out.reserve(nof_ue) ||
      !g->d_bce.reserve(ce_tot) ||
      !g->d_sym.reserve(sym_tot) ||
      !g->d_q.reserve(q_tot) || !g->d_c.reserve(c_tot + 16) ||
      !g->d_llr.reserve(nof_ue)) {
    return SRSRAN_ERROR;
  }
  std::vector<LlrItem> items(nof_ue);
  for (uint32_t i = 0; i < nof_ue; i++) {
    desc[i].ce  = g->d_bce + ce_off[i];
    desc[i].sym = g->d_sym + sym_off[i];
    desc[i].out = g->d_out + i;
    LlrItem& it = items[i];
    memset(&it, 0, sizeof(it));
    it.sym      = (const float*)desc[i].sym;
    it.llr      = g->d_q + q_off[i];
    it.n        = ues[i].cfg->grant.nof_re;
    it.seed     = pusch_seed(ues[i].cfg->rnti, 2 * (ues[i].sf->tti % SRSRAN_NOF_SF_X_FRAME), ues[i].chest->cell.id);
    it.scramble = 1;
  }
  // the LLR launch takes one modulation: order the items by it
  std::vector<uint32_t> order(nof_ue);
  for (uint32_t i = 0; i < nof_ue; i++) {
    order[i] = i;
  }
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return ues[a].cfg->grant.tb.mod < ues[b].cfg->grant.tb.mod; });
  std::vector<LlrItem> sorted(nof_ue);
  for (uint32_t k = 0; k < nof_ue; k++) {
    sorted[k] = items[order[k]];
  }
  if (hipMemcpyAsync(g->d_desc, desc.data(), nof_ue * sizeof(PuschUe), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(g->d_llr, sorted.data(), nof_ue * sizeof(LlrItem), hipMemcpyHostToDevice, st) != hipSuccess ||
      chest_ul_launch(g->d_desc, nof_ue, st) != hipSuccess || pusch_eq_idft_launch(g->d_desc, nof_ue, st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  for (uint32_t k = 0; k < nof_ue;) {
    const int mod = (int)ues[order[k]].cfg->grant.tb.mod;
    uint32_t  k1 = k, max_n = 0;
    while (k1 < nof_ue && (int)ues[order[k1]].cfg->grant.tb.mod == mod) {
      max_n = std::max(max_n, sorted[k1].n);
      k1++;
    }
    if (llr_batch_launch(mod, g->d_llr + k, k1 - k, max_n, 1, st) != hipSuccess) {
      return SRSRAN_ERROR;
    }
    k = k1;
  }
  for (uint32_t i = 0; i < nof_ue; i++) {
    if (any_uci(ues[i].cfg) &&
        seq_unpack_launch(g->d_c + c_off[i], ues[i].cfg->grant.tb.nof_bits, items[i].seed, st) != hipSuccess) {
      return SRSRAN_ERROR;
    }
  }

  // ---- UL-SCH: every UE, with or without UCI, through the batched srsran_ulsch_decode (sch_internal.h):
  // one ACK/RI launch, one de-interleaver launch, one CQI launch and one decode_tb batch ----
  int                       rc = SRSRAN_SUCCESS;
  size_t                    g_tot = 0, data_tot = 0;
  std::vector<size_t>       g_off(nof_ue), data_off(nof_ue);
  for (uint32_t i = 0; i < nof_ue; i++) {
    const srsran_pusch_cfg_t* cfg = ues[i].cfg;
    g_off[i]                      = g_tot;
    data_off[i]                   = data_tot;
    g_tot += (cfg->grant.tb.nof_bits + 7) & ~7u;
    data_tot += cfg->grant.tb.tbs > 0 ? (((uint32_t)cfg->grant.tb.tbs / 8 + 64 + 15) & ~15u) : 0;
  }
  if (!g->d_g.reserve(g_tot) || !g->d_data.reserve(data_tot + 16)) {
    return SRSRAN_ERROR;
  }
  std::vector<UlschBatchUe> ub(nof_ue);
  for (uint32_t i = 0; i < nof_ue; i++) {
    UlschBatchUe& u = ub[i];
    memset(&u, 0, sizeof(u));
    u.cfg      = ues[i].cfg;
    u.d_q      = g->d_q + q_off[i];
    u.d_c      = any_uci(ues[i].cfg) ? g->d_c + c_off[i] : nullptr;
    u.d_g      = g->d_g + g_off[i];
    u.d_data   = g->d_data + data_off[i];
    u.new_data = ues[i].new_data;
    u.data     = res[i].data;
    u.uci      = &res[i].uci;
    if (!any_uci(ues[i].cfg) && ues[i].cfg->grant.tb.tbs > 0) {
      memset(&res[i].uci, 0, sizeof(res[i].uci));
    }
  }
  if (ulsch_decode_batch_dev(&q->ul_sch, nof_ue, ub.data(), g->d_data, data_tot, st) != SRSRAN_SUCCESS) {
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < nof_ue; i++) {
    res[i].crc                  = ub[i].ret == 0;
    res[i].avg_iterations_block = ub[i].avg;
    res[i].evm                  = NAN;
    ues[i].cfg->last_O_cqi      = (uint32_t)srsran_cqi_size(&ues[i].cfg->uci_cfg.cqi);
    if (ub[i].ret < 0 && ub[i].ret != SRSRAN_ERROR) {
      rc = ub[i].ret;
    }
  }
  std::vector<ChestUlOut> outs(nof_ue);
  if (hipMemcpyAsync(outs.data(), g->d_out, nof_ue * sizeof(ChestUlOut), hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < nof_ue; i++) {
    res[i].epre_dbfs = ues[i].cfg->meas_epre_en ? 10.0f * log10f(outs[i].data_pow / (float)ues[i].cfg->grant.nof_re)
                                                : NAN;
    if (chest_res) {
      finish_chest_res(&chest_res[i], outs[i]);
      if (chest_res[i].ce) {  // the estimate rows, as srsran_chest_ul_estimate_pusch writes them
        const PuschUe& u = desc[i];
        for (uint32_t s = 0; s < 2; s++) {
          const size_t o0 = (size_t)s * u.nsym_slot * u.ncell_re + u.n_prb[s] * SRSRAN_NRE;
          if (hipMemcpy2D(chest_res[i].ce + o0, u.ncell_re * sizeof(float2), desc[i].ce + o0, u.ncell_re * sizeof(float2),
                          u.M * sizeof(float2), u.nsym_slot, hipMemcpyDeviceToHost) != hipSuccess) {
            return SRSRAN_ERROR;
          }
        }
        ChestUlResGpu* rg = (ChestUlResGpu*)chest_res[i].gpu;
        if (rg) {
          rg->valid = false;  // the host copy is now the current one
        }
      }
    }
  }
  return rc;
}

int srsran_pusch_init_ue(srsran_pusch_t* q, uint32_t max_prb)
{
  const int ret = srsran_pusch_init_enb(q, max_prb);
  if (ret == SRSRAN_SUCCESS) {
    q->is_ue = true;
  }
  return ret;
}

int srsran_pusch_encode(srsran_pusch_t*      q,
                        srsran_ul_sf_cfg_t*  sf,
                        srsran_pusch_cfg_t*  cfg,
                        srsran_pusch_data_t* data,
                        cf_t*                sf_symbols)
{
  if (!q || !q->gpu || !cfg || !sf || !data || !sf_symbols) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PuschGpu*      g      = (PuschGpu*)q->gpu;
  hipStream_t    st     = sch_stream(&q->ul_sch);
  const size_t   sf_re  = (size_t)q->cell.nof_prb * SRSRAN_NRE * 2 * nsymb_slot(q->cell.cp);
  const uint32_t nbytes = cfg->grant.tb.tbs > 0 ? (uint32_t)cfg->grant.tb.tbs / 8 : 0;
  if (nbytes && !data->ptr) {
    fprintf(stderr, "[srsran_pusch] encoding from the soft buffer (data == NULL) is not provided\n");
    return SRSRAN_ERROR;
  }
  if (sf_re == 0 || !g->d_grid.reserve(sf_re) ||
      !g->d_txdata.reserve((size_t)nbytes + 16) ||
      hipMemcpyAsync(g->d_grid, sf_symbols, sf_re * sizeof(float2), hipMemcpyHostToDevice, st) != hipSuccess ||
      (nbytes && hipMemcpyAsync(g->d_txdata, data->ptr, nbytes, hipMemcpyHostToDevice, st) != hipSuccess)) {
    return SRSRAN_ERROR;
  }
  TxReq r;
  memset(&r, 0, sizeof(r));
  r.pusch  = q;
  r.sf     = sf;
  r.cfg    = cfg;
  r.uci    = &data->uci;
  r.d_data = nbytes ? g->d_txdata : nullptr;
  r.d_grid = g->d_grid;
  std::vector<PuschTxUe> desc;
  const PuschTxUe*       d_desc = nullptr;
  int                    ret    = pusch_tx_run(q, 1, &r, desc, &d_desc, st);
  if (ret == SRSRAN_SUCCESS &&
      hipMemcpyAsync(sf_symbols, g->d_grid, sf_re * sizeof(float2), hipMemcpyDeviceToHost, st) != hipSuccess) {
    ret = SRSRAN_ERROR;
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    ret = SRSRAN_ERROR;
  }
  return ret;
}

}  // extern "C"
