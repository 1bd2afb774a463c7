// srsran_4g_amd/csrc/ue_ul_api.cpp -- the UE's uplink object (include/srsran_ue_ul.h; ue_ul.c): srsran_ue_ul_encode
// and srsran_ue_ul_gpu_tx_batch with the PUSCH branch (pusch_tx_run of pusch_api.cpp), the PUCCH branch
// (pucch_tx_prepare of pucch_api.cpp, pucch_tx_kernel.hip) and the SRS (srs_kernel.hip), SC-FDMA and normalisation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/srsran_ue_ul.h"
#include "ofdm_kernel.h"
#include "sch_internal.h"
#include "srs_kernel.h"
#include "ul_internal.h"

using namespace srsran_amd;

namespace {

// ---------------- ue_ul device state ----------------
struct UeUlGpu {
  UlHopping hop;
  bool      hop_ok = false;
  DevBuf<float2>  d_grid;  // the grids of this object's entries of a batch
  DevBuf<float2>  d_samp;  // their samples before the normalisation
  DevBuf<float2>  d_cfo;   // srsran_vec_apply_cfo's phasors of cfo_freq (cfo_len samples)
  float     cfo_freq = 0.0f;
  uint32_t  cfo_len = 0;
  DevBuf<uint8_t> d_io;    // sync API: payload, then the output samples
  DevBuf<uint8_t> d_ptx;   // the PUCCH descriptors of a batch this object's scratch serves
  DevBuf<uint8_t> d_stx;   // its SRS descriptors
  // srsran_ue_ul_gpu_last
  const uint8_t* last_s = nullptr;
  const float2*  last_d = nullptr;
  const float2*  last_grid = nullptr;
  uint32_t       last_bits = 0, last_re = 0, last_ngrid = 0;
  bool           last_ok = false;  // an encode has run (a PUCCH subframe leaves last_bits = last_re = 0)
};

}  // namespace

extern "C" {

// ---------------- ue_ul.c:41-175 ----------------
int srsran_ue_ul_init(srsran_ue_ul_t* q, cf_t* out_buffer, uint32_t max_prb)
{
  if (!q) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  memset(q, 0, sizeof(*q));
  srsran_ofdm_cfg_t ofdm_cfg;
  memset(&ofdm_cfg, 0, sizeof(ofdm_cfg));
  ofdm_cfg.nof_prb      = max_prb;
  ofdm_cfg.cp           = SRSRAN_CP_NORM;
  ofdm_cfg.freq_shift_f = 0.5f;
  ofdm_cfg.normalize    = true;
  if (srsran_ofdm_tx_init_cfg(&q->fft, &ofdm_cfg)) {
    fprintf(stderr, "[srsran_ue_ul] Error initiating FFT\n");
    return SRSRAN_ERROR;
  }
  if (srsran_pusch_init_ue(&q->pusch, max_prb)) {
    fprintf(stderr, "[srsran_ue_ul] Error creating PUSCH object\n");
    srsran_ofdm_tx_free(&q->fft);
    return SRSRAN_ERROR;
  }
  q->gpu        = new UeUlGpu();
  q->out_buffer = out_buffer;
  return SRSRAN_SUCCESS;
}

void srsran_ue_ul_free(srsran_ue_ul_t* q)
{
  if (!q) {
    return;
  }
  UeUlGpu* g = (UeUlGpu*)q->gpu;
  if (g) {
    hipStream_t st = sch_stream(&q->pusch.ul_sch);
    if (st) {
      hipStreamSynchronize(st);
    }
    delete g;
  }
  srsran_ofdm_tx_free(&q->fft);
  srsran_pusch_free(&q->pusch);
  memset(q, 0, sizeof(*q));
}

int srsran_ue_ul_set_cell(srsran_ue_ul_t* q, srsran_cell_t cell)
{
  if (!q || !q->gpu || !cell_valid(cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (q->cell.id != cell.id || q->cell.nof_prb == 0) {
    UeUlGpu* g = (UeUlGpu*)q->gpu;
    g->hop_ok  = false;
    g->last_bits = 0;
    g->last_ok   = false;
    if (srsran_ofdm_rx_set_prb(&q->fft, cell.cp, cell.nof_prb)) {  // srsran_ofdm_tx_set_prb: the same object
      fprintf(stderr, "[srsran_ue_ul] Error resizing FFT\n");
      return SRSRAN_ERROR;
    }
    if (srsran_pusch_set_cell(&q->pusch, cell)) {
      return SRSRAN_ERROR;
    }
    q->cell = cell;
    hopping_tables(cell, g->hop);
    g->hop_ok = true;
  }
  return SRSRAN_SUCCESS;
}

int srsran_ue_ul_set_cfr(srsran_ue_ul_t*, const void*)
{
  fprintf(stderr, "[srsran_ue_ul] crest factor reduction is not provided\n");
  return SRSRAN_ERROR;
}

int srsran_ue_ul_pregen_signals(srsran_ue_ul_t*, srsran_ue_ul_cfg_t*)
{
  fprintf(stderr, "[srsran_ue_ul] pregenerated signals are not provided: every subframe generates its DMRS\n");
  return SRSRAN_ERROR;
}

// ue_ul.c:497-506
void srsran_ue_ul_pucch_resource_selection(const srsran_cell_t*      cell,
                                           srsran_pucch_cfg_t*       cfg,
                                           const srsran_uci_cfg_t*   uci_cfg,
                                           const srsran_uci_value_t* uci_value,
                                           uint8_t                   b[SRSRAN_UCI_MAX_ACK_BITS])
{
  cfg->format  = srsran_pucch_proc_select_format(cell, cfg, uci_cfg, uci_value);
  cfg->n_pucch = (uint16_t)srsran_pucch_proc_get_npucch(cell, cfg, uci_cfg, uci_value, b);
}

// ue_ul.c:561-600, 36.213 Table 10.1.5-1
int srsran_ue_ul_sr_send_tti(const srsran_pucch_cfg_t* cfg, uint32_t current_tti)
{
  if (!cfg->sr_configured) {
    return SRSRAN_SUCCESS;
  }
  static const uint32_t first[8] = {0, 5, 15, 35, 75, 155, 157, 158}, period[7] = {5, 10, 20, 40, 80, 2, 1};
  const uint32_t        I_sr     = cfg->I_sr;
  if (I_sr >= first[7]) {
    return SRSRAN_ERROR;
  }
  uint32_t k = 0;
  while (I_sr >= first[k + 1]) {
    k++;
  }
  const uint32_t offset = I_sr - first[k];
  return current_tti >= offset && (current_tti - offset) % period[k] == 0 ? 1 : SRSRAN_SUCCESS;
}

// ue_ul.c:602-614
bool srsran_ue_ul_gen_sr(srsran_ue_ul_cfg_t* cfg, srsran_ul_sf_cfg_t* sf, srsran_uci_data_t* uci_data, bool sr_request)
{
  uci_data->value.scheduling_request = false;
  if (srsran_ue_ul_sr_send_tti(&cfg->ul_cfg.pucch, sf->tti)) {
    if (sr_request) {
      uci_data->value.scheduling_request = true;
    }
    uci_data->cfg.is_scheduling_request_tti = true;
    return true;
  }
  return false;
}

int srsran_ue_ul_gpu_tx_batch(uint32_t nof_ue, const srsran_ue_ul_gpu_entry_t* entries, void* stream)
{
  if (nof_ue == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!entries) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  enum { K_PUSCH, K_PUCCH, K_SRS, K_NONE };  // the branch order of ue_ul.c:640-656
  hipStream_t                  st = (hipStream_t)stream;
  std::vector<srsran_ue_ul_t*> objs;            // the distinct cell objects, in order of first use
  std::vector<uint32_t>        slot(nof_ue);    // the entry's index among its object's transmissions
  std::vector<uint32_t>        count, samples;  // per object: transmissions, transmissions that want samples
  std::vector<uint32_t>        obj_of(nof_ue), kind(nof_ue), idx(nof_ue);  // idx: among the entries of its kind
  std::vector<PucchTxUe>       pdesc;
  std::vector<SrsTxUe>         sdesc;           // the SRS of every entry whose subframe carries it, with or without a channel
  std::vector<int>             srs_of(nof_ue, -1);
  uint32_t                     npusch = 0, nsrs_only = 0;
  for (uint32_t i = 0; i < nof_ue; i++) {
    const srsran_ue_ul_gpu_entry_t& e = entries[i];
    if (!e.q || !e.q->gpu || !e.sf || !e.cfg || !((UeUlGpu*)e.q->gpu)->hop_ok) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    // add_srs (ue_ul.c:301-311) or srs_encode (435-451); checked before anything of the caller's is written
    const bool with_srs = srs_tx_enabled(e.cfg->ul_cfg.srs, e.sf->tti);
    SrsTxUe    srs_d;
    if (with_srs && srs_tx_prepare(e.q->cell, ((UeUlGpu*)e.q->gpu)->hop, e.cfg->ul_cfg.srs, e.cfg->ul_cfg.dmrs, e.sf->tti,
                                   &srs_d) != SRSRAN_SUCCESS) {
      fprintf(stderr, "[srsran_ue_ul] Invalid SRS configuration (tti %u carries this UE's SRS)\n", e.sf->tti);
      return SRSRAN_ERROR;
    }
    if (e.cfg->grant_available) {
      kind[i] = K_PUSCH;
      idx[i]  = npusch++;
    } else {
      // the PUCCH branch of ue_ul.c:642-648 and pucch_encode (510-541) up to the kernel
      srsran_pucch_cfg_t*     pc = &e.cfg->ul_cfg.pucch;
      const srsran_uci_cfg_t& pu = pc->uci_cfg;
      srsran_uci_value_t      value;
      if (e.uci) {
        value = *e.uci;
      } else {
        memset(&value, 0, sizeof(value));
      }
      const bool pending = srsran_uci_cfg_total_ack(&pu) > 0 || pu.cqi.data_enable || pu.cqi.ri_len > 0;
      kind[i]            = (pending || value.scheduling_request) && e.cfg->cc_idx == 0 ? K_PUCCH : K_NONE;
      if (kind[i] == K_PUCCH) {
        if (!pc->rnti) {
          fprintf(stderr, "[srsran_ue_ul] Encoding PUCCH: rnti not set in ul_cfg\n");
          return SRSRAN_ERROR;
        }
        if (!srsran_pucch_cfg_isvalid(pc, e.q->cell.nof_prb)) {
          fprintf(stderr, "[srsran_ue_ul] Invalid PUCCH configuration\n");
          return SRSRAN_ERROR;
        }
      }
      if (kind[i] == K_PUCCH) {
        srsran_uci_value_t value2 = value;  // the value that is encoded: b(0) b(1) of the selection go here
        srsran_ue_ul_pucch_resource_selection(&e.q->cell, pc, &pc->uci_cfg, &value, value2.ack.ack_value);
        if (pc->format == SRSRAN_PUCCH_FORMAT_ERROR) {
          return SRSRAN_ERROR;
        }
        srsran_refsignal_srs_pucch_shortened_cfg(e.sf, &e.cfg->ul_cfg.srs, pc);
        PucchTxUe d;
        if (pucch_tx_prepare(e.q->cell, e.sf, pc, &value2, &d) != SRSRAN_SUCCESS) {
          fprintf(stderr, "[srsran_ue_ul] Error encoding PUCCH\n");
          return SRSRAN_ERROR;
        }
        idx[i] = (uint32_t)pdesc.size();
        pdesc.push_back(d);
      }
    }
    if (with_srs) {
      if (kind[i] == K_NONE) {
        kind[i] = K_SRS;
        idx[i]  = nsrs_only++;
      }
      srs_of[i] = (int)sdesc.size();
      sdesc.push_back(srs_d);
    }
    size_t o = std::find(objs.begin(), objs.end(), e.q) - objs.begin();
    if (o == objs.size()) {
      objs.push_back(e.q);
      count.push_back(0);
      samples.push_back(0);
    }
    obj_of[i] = (uint32_t)o;
    if (kind[i] != K_NONE) {
      slot[i] = count[o]++;
      samples[o] += e.d_out ? 1 : 0;
    }
  }
  for (size_t o = 0; o < objs.size(); o++) {
    srsran_ue_ul_t* q = objs[o];
    UeUlGpu*        g = (UeUlGpu*)q->gpu;
    const size_t sf_re = (size_t)q->cell.nof_prb * SRSRAN_NRE * 2 * nsymb_slot(q->cell.cp);
    if (!g->d_grid.reserve(count[o] * sf_re) ||
        !g->d_samp.reserve((size_t)count[o] * q->fft.sf_sz)) {
      return SRSRAN_ERROR;
    }
  }
  std::vector<TxReq>     r(npusch);
  // the normalisation stage of the PUCCH entries, then of the SRS-only entries
  std::vector<PuschTxUe> pnorm(pdesc.size() + nsrs_only, PuschTxUe{});
  for (uint32_t i = 0; i < nof_ue; i++) {
    const srsran_ue_ul_gpu_entry_t& e = entries[i];
    srsran_ue_ul_t*                 q = e.q;
    UeUlGpu*                        g = (UeUlGpu*)q->gpu;
    const size_t sf_re = (size_t)q->cell.nof_prb * SRSRAN_NRE * 2 * nsymb_slot(q->cell.cp);
    if (kind[i] == K_NONE) {  // nothing to send: zero outputs
      if ((e.d_out && hipMemsetAsync(e.d_out, 0, q->fft.sf_sz * sizeof(float2), st) != hipSuccess) ||
          (e.d_grid && hipMemsetAsync(e.d_grid, 0, sf_re * sizeof(float2), st) != hipSuccess)) {
        return SRSRAN_ERROR;
      }
      continue;
    }
    const float2* samples_in = g->d_samp + (size_t)slot[i] * q->fft.sf_sz;
    const uint32_t norm_mode = e.cfg->normalize_mode == SRSRAN_UE_UL_NORMALIZE_MODE_FORCE_AMPLITUDE ? 1 : 0;
    const float   force_peak = e.cfg->force_peak_amplitude > 0 ? e.cfg->force_peak_amplitude : 1.0f;
    if (srs_of[i] >= 0) {
      SrsTxUe& d  = sdesc[srs_of[i]];
      d.grid      = g->d_grid + slot[i] * sf_re;
      d.zero_rest = kind[i] == K_SRS ? 1 : 0;
    }
    if (kind[i] == K_PUCCH || kind[i] == K_SRS) {
      const bool pucch = kind[i] == K_PUCCH;
      if (pucch) {
        PucchTxUe& d = pdesc[idx[i]];
        d.grid       = g->d_grid + slot[i] * sf_re;
        d.zero_rest  = 1;
      }
      if (e.d_out) {
        PuschTxUe& u  = pnorm[pucch ? idx[i] : pdesc.size() + idx[i]];
        u.samples_in  = samples_in;
        u.samples_out = (float2*)e.d_out;
        u.sf_len      = q->fft.sf_sz;
        u.norm_mode   = norm_mode;
        // ue_ul.c:548 / 446: a float quotient here
        u.norm_factor = pucch ? (float)q->cell.nof_prb / 15 / 10
                              : (float)q->cell.nof_prb / 15 / sqrtf((float)sdesc[srs_of[i]].m_sc);
        u.force_peak  = force_peak;
      }
      continue;
    }
    TxReq& t = r[idx[i]];
    memset(&t, 0, sizeof(t));
    t.pusch     = &q->pusch;
    t.hop       = &g->hop;
    t.dmrs_cfg  = &e.cfg->ul_cfg.dmrs;
    t.sf        = e.sf;
    t.cfg       = &e.cfg->ul_cfg.pusch;
    t.uci       = e.uci;
    t.d_data    = e.d_data;
    t.d_grid    = g->d_grid + slot[i] * sf_re;
    t.zero_rest = true;
    if (e.d_out) {
      t.samples_in  = samples_in;
      t.samples_out = (float2*)e.d_out;
      t.sf_len      = q->fft.sf_sz;
      t.norm_mode   = norm_mode;
      // ue_ul.c:345: the integer quotient nof_prb / 15 first
      t.norm_factor = (float)(q->cell.nof_prb / 15) / sqrtf((float)e.cfg->ul_cfg.pusch.grant.L_prb) / 2;
      t.force_peak  = force_peak;
    }
  }
  if (npusch == 0 && pdesc.empty() && sdesc.empty()) {
    return SRSRAN_SUCCESS;
  }
  std::vector<PuschTxUe> desc;
  const PuschTxUe*       d_desc = nullptr;
  const int              ret    = pusch_tx_run(&entries[0].q->pusch, npusch, r.data(), desc, &d_desc, st, pnorm);
  if (ret != SRSRAN_SUCCESS) {
    return ret == SRSRAN_ERROR_INVALID_INPUTS ? ret : SRSRAN_ERROR;
  }
  if (!pdesc.empty()) {  // every PUCCH entry of every cell in one launch
    UeUlGpu* g0 = (UeUlGpu*)entries[0].q->gpu;
    if (!g0->d_ptx.reserve(pdesc.size() * sizeof(PucchTxUe)) ||
        hipMemcpyAsync(g0->d_ptx, pdesc.data(), pdesc.size() * sizeof(PucchTxUe), hipMemcpyHostToDevice, st) != hipSuccess ||
        pucch_tx_launch((const PucchTxUe*)g0->d_ptx.get(), (uint32_t)pdesc.size(), st) != hipSuccess) {
      return SRSRAN_ERROR;
    }
  }
  if (!sdesc.empty()) {  // every SRS of every cell in one launch, after the channels it shares a grid with
    UeUlGpu* g0 = (UeUlGpu*)entries[0].q->gpu;
    if (!g0->d_stx.reserve(sdesc.size() * sizeof(SrsTxUe)) ||
        hipMemcpyAsync(g0->d_stx, sdesc.data(), sdesc.size() * sizeof(SrsTxUe), hipMemcpyHostToDevice, st) != hipSuccess ||
        srs_tx_launch((const SrsTxUe*)g0->d_stx.get(), (uint32_t)sdesc.size(), st) != hipSuccess) {
      return SRSRAN_ERROR;
    }
  }
  for (size_t o = 0; o < objs.size(); o++) {
    UeUlGpu* g = (UeUlGpu*)objs[o]->gpu;
    if (samples[o] && srsran_ofdm_tx_gpu(&objs[o]->fft, (const cf_t*)g->d_grid.get(), (cf_t*)g->d_samp.get(), 1, count[o], 1.0f, st) !=
                          SRSRAN_SUCCESS) {
      return SRSRAN_ERROR;
    }
  }
  for (uint32_t i = 0; i < nof_ue; i++) {
    const srsran_ue_ul_gpu_entry_t& e = entries[i];
    srsran_ue_ul_t*                 q = e.q;
    UeUlGpu*                        g = (UeUlGpu*)q->gpu;
    const size_t sf_re = (size_t)q->cell.nof_prb * SRSRAN_NRE * 2 * nsymb_slot(q->cell.cp);
    if (kind[i] == K_NONE) {
      continue;
    }
    const float2* grid = g->d_grid + slot[i] * sf_re;
    if (e.d_grid && hipMemcpyAsync(e.d_grid, grid, sf_re * sizeof(float2), hipMemcpyDeviceToDevice, st) != hipSuccess) {
      return SRSRAN_ERROR;
    }
    // apply_cfo (ue_ul.c:260-266): the samples times srsran_vec_apply_cfo's phasors of cfo_value / symbol_sz
    const float f = e.cfg->cfo_value / (float)srsran_symbol_sz(q->cell.nof_prb);
    if (e.d_out && e.cfg->cfo_en && f != 0.0f) {  // a zero frequency multiplies every sample by exactly 1
      const uint32_t len = q->fft.sf_sz;
      if (g->cfo_len != len || g->cfo_freq != f) {
        float c, s;
        cfo_phasor(f, &c, &s);
        if (!g->d_cfo.reserve(len) ||
            cfo_table_launch(c, s, g->d_cfo, len, st) != hipSuccess) {
          return SRSRAN_ERROR;
        }
        g->cfo_len  = len;
        g->cfo_freq = f;
      }
      float2* x = g->d_samp + (size_t)slot[i] * len;
      if (cfo_launch(x, x, g->d_cfo, len, st) != hipSuccess) {
        return SRSRAN_ERROR;
      }
    }
    const bool pusch = kind[i] == K_PUSCH;
    g->last_s        = pusch ? desc[idx[i]].s_pack : nullptr;
    g->last_bits     = pusch ? e.cfg->ul_cfg.pusch.grant.tb.nof_bits : 0;
    g->last_d        = pusch ? desc[idx[i]].d : nullptr;
    g->last_re       = pusch ? e.cfg->ul_cfg.pusch.grant.nof_re : 0;
    g->last_grid     = grid;
    g->last_ngrid    = (uint32_t)sf_re;
    g->last_ok       = true;
  }
  return pusch_tx_norm_launch(d_desc, (uint32_t)desc.size(), st) == hipSuccess ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

int srsran_ue_ul_gpu_last(srsran_ue_ul_t* q,
                          const uint8_t** d_scrambled,
                          uint32_t*       nof_bits,
                          const cf_t**    d_symbols,
                          uint32_t*       nof_re,
                          const cf_t**    d_grid,
                          uint32_t*       nof_grid)
{
  if (!q || !q->gpu || !d_scrambled || !nof_bits || !d_symbols || !nof_re || !d_grid || !nof_grid) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  UeUlGpu* g = (UeUlGpu*)q->gpu;
  if (!g->last_ok) {
    return SRSRAN_ERROR;
  }
  *d_scrambled = g->last_s;
  *nof_bits    = g->last_bits;
  *d_symbols   = (const cf_t*)g->last_d;
  *nof_re      = g->last_re;
  *d_grid      = (const cf_t*)g->last_grid;
  *nof_grid    = g->last_ngrid;
  return SRSRAN_SUCCESS;
}

// ue_ul.c:618-659
int srsran_ue_ul_encode(srsran_ue_ul_t* q, srsran_ul_sf_cfg_t* sf, srsran_ue_ul_cfg_t* cfg, srsran_pusch_data_t* data)
{
  if (!q || !q->gpu || !sf || !cfg || !data) {
    return SRSRAN_ERROR;
  }
  // DTX to NACK in channel-selection mode; all DTX: no HARQ-ACK
  if (cfg->ul_cfg.pucch.ack_nack_feedback_mode != SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_NORMAL) {
    const uint32_t nack      = srsran_uci_cfg_total_ack(&cfg->ul_cfg.pusch.uci_cfg);
    uint32_t       dtx_count = 0;
    for (uint32_t a = 0; a < nack && a < SRSRAN_UCI_MAX_ACK_BITS; a++) {
      if (data->uci.ack.ack_value[a] == 2) {
        data->uci.ack.ack_value[a] = 0;
        dtx_count++;
      }
    }
    if (dtx_count == nack) {
      for (int i = 0; i < SRSRAN_MAX_CARRIERS; i++) {
        cfg->ul_cfg.pusch.uci_cfg.ack[i].nof_acks = 0;
      }
    }
  }
  UeUlGpu*     g      = (UeUlGpu*)q->gpu;
  const size_t sf_len = q->cell.nof_prb ? q->fft.sf_sz : 0;
  if (!cfg->grant_available) {
    const srsran_uci_cfg_t& pu = cfg->ul_cfg.pucch.uci_cfg;
    const bool pucch = (srsran_uci_cfg_total_ack(&pu) > 0 || pu.cqi.data_enable || pu.cqi.ri_len > 0 ||
                        data->uci.scheduling_request) &&
                       cfg->cc_idx == 0;
    // PUCCH, over the PCell only (ue_ul.c:642-648), else the SRS alone (649-651): a batch of one
    if (pucch || srs_tx_enabled(cfg->ul_cfg.srs, sf->tti)) {
      hipStream_t st = sch_stream(&q->pusch.ul_sch);
      if (!g->hop_ok || !q->out_buffer || !g->d_io.reserve(sf_len * sizeof(cf_t))) {
        return SRSRAN_ERROR;
      }
      srsran_ue_ul_gpu_entry_t e   = {q, sf, cfg, &data->uci, nullptr, (cf_t*)g->d_io.get(), nullptr};
      int                      ret = srsran_ue_ul_gpu_tx_batch(1, &e, st);
      if (ret == SRSRAN_SUCCESS &&
          hipMemcpyAsync(q->out_buffer, g->d_io, sf_len * sizeof(cf_t), hipMemcpyDeviceToHost, st) != hipSuccess) {
        ret = SRSRAN_ERROR;
      }
      if (hipStreamSynchronize(st) != hipSuccess) {
        ret = SRSRAN_ERROR;
      }
      return ret == SRSRAN_SUCCESS ? 1 : SRSRAN_ERROR;
    }
    if (sf_len && q->out_buffer) {
      memset(q->out_buffer, 0, sf_len * sizeof(cf_t));
    }
    return SRSRAN_SUCCESS;
  }
  if (!g->hop_ok || !q->out_buffer) {
    return SRSRAN_ERROR;
  }
  hipStream_t    st     = sch_stream(&q->pusch.ul_sch);
  const int      tbs    = cfg->ul_cfg.pusch.grant.tb.tbs;
  const uint32_t nbytes = tbs > 0 ? (uint32_t)tbs / 8 : 0;
  const size_t   o_out  = ((size_t)nbytes + 31) & ~(size_t)15;
  if (nbytes && !data->ptr) {
    fprintf(stderr, "[srsran_ue_ul] encoding from the soft buffer (data == NULL) is not provided\n");
    return SRSRAN_ERROR;
  }
  if (!g->d_io.reserve(o_out + sf_len * sizeof(cf_t)) ||
      (nbytes && hipMemcpyAsync(g->d_io, data->ptr, nbytes, hipMemcpyHostToDevice, st) != hipSuccess)) {
    return SRSRAN_ERROR;
  }
  srsran_ue_ul_gpu_entry_t e = {q, sf, cfg, &data->uci, nbytes ? g->d_io : nullptr, (cf_t*)(g->d_io + o_out), nullptr};
  int                      ret = srsran_ue_ul_gpu_tx_batch(1, &e, st);
  if (ret == SRSRAN_SUCCESS &&
      hipMemcpyAsync(q->out_buffer, g->d_io + o_out, sf_len * sizeof(cf_t), hipMemcpyDeviceToHost, st) != hipSuccess) {
    ret = SRSRAN_ERROR;
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    ret = SRSRAN_ERROR;
  }
  return ret == SRSRAN_SUCCESS ? 1 : SRSRAN_ERROR;
}

}  // extern "C"
