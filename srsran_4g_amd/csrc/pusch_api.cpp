// srsran_4g_amd/csrc/pusch_api.cpp -- C-ABI of the PUSCH receive path (include/srsran_pusch.h) and, at the end, of
// the UE's uplink transmit path (srsran_pusch_encode, include/srsran_ue_ul.h: the PUSCH branch and, over
// pucch_tx_kernel.hip and srs_kernel.hip, the PUCCH and SRS branches of srsran_ue_ul_encode /
// srsran_ue_ul_gpu_tx_batch, with the host helpers of the sounding reference signal):
// PUSCH DMRS generation (refsignal_ul.c:95-358 restated), the UL channel estimator object
// (chest_ul.c:53-433) and srsran_pusch_t (pusch.c:108-471), over the kernels of pusch_kernel.hip,
// llr_kernel.hip and the UL-SCH decoder of sch_api.cpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/srsran_pusch.h"
#include "../../include/srsran_ue_ul.h"
#include "dev_buf.h"
#include "llr_kernel.h"
#include "ofdm_kernel.h"
#include "pusch_kernel.h"
#include "pucch_tx_kernel.h"
#include "pusch_tx_internal.h"
#include "srs_kernel.h"
#include "ulsch_batch.h"

namespace srsran_amd {
// pucch_api.cpp: srsran_pucch_encode up to the kernel
int pucch_tx_prepare(const srsran_cell_t& cell, const srsran_ul_sf_cfg_t* sf, srsran_pucch_cfg_t* cfg,
                     const srsran_uci_value_t* uci, PucchTxUe* d);
int         ulsch_decode_dev(srsran_sch_t* q, srsran_pusch_cfg_t* cfg, int16_t* d_q, const uint8_t* d_c, uint8_t* data,
                             srsran_uci_value_t* uci_data);
hipStream_t sch_stream(srsran_sch_t* q);
int         sch_own_queue(srsran_sch_t* q);
}  // namespace srsran_amd

using namespace srsran_amd;

namespace {

#include "zc_tables.inc"

constexpr uint32_t kNdmrs1[8] = {0, 2, 3, 4, 6, 8, 9, 10};  // 36.211 Table 5.5.2.1.1-2
constexpr uint32_t kNdmrs2[8] = {0, 6, 3, 4, 2, 8, 10, 9};  // 36.211 Table 5.5.2.1.1-1

uint32_t nsymb_slot(srsran_cp_t cp) { return cp == SRSRAN_CP_NORM ? 7u : 6u; }

bool cell_valid(const srsran_cell_t& c) { return c.id < 504 && c.nof_ports >= 1 && c.nof_ports <= 4 && c.nof_prb >= 6 && c.nof_prb <= SRSRAN_MAX_PRB; }

// LTE Gold sequence c(n) (36.211 7.2, Nc = 1600)
void gold(uint32_t c_init, uint8_t* c, uint32_t len)
{
  uint32_t x1 = 1, x2 = c_init & 0x7FFFFFFFu;
  auto     s1 = [](uint32_t s) { return (s >> 1) ^ (((s ^ (s >> 3)) & 1u) << 30); };
  auto     s2 = [](uint32_t s) { return (s >> 1) ^ (((s ^ (s >> 1) ^ (s >> 2) ^ (s >> 3)) & 1u) << 30); };
  for (int n = 0; n < 1600; n++) {
    x1 = s1(x1);
    x2 = s2(x2);
  }
  for (uint32_t n = 0; n < len; n++) {
    c[n] = (uint8_t)((x1 ^ x2) & 1u);
    x1   = s1(x1);
    x2   = s2(x2);
  }
}

// the per-cell hopping tables of srsran_refsignal_ul_set_cell (refsignal_ul.c:95-171)
struct UlHopping {
  uint32_t n_prs[SRSRAN_NOF_DELTA_SS][SRSRAN_NSLOTS_X_FRAME];  // 5.5.2.1.1 n_PN(ns)
  uint32_t f_gh[SRSRAN_NSLOTS_X_FRAME];                       // 5.5.1.3 group hopping
  uint32_t v[SRSRAN_NSLOTS_X_FRAME][SRSRAN_NOF_DELTA_SS];     // 5.5.1.4 sequence hopping
};

void hopping_tables(const srsran_cell_t& cell, UlHopping& h)
{
  const uint32_t       ns_len = 8 * nsymb_slot(cell.cp) * 20;
  std::vector<uint8_t> c(ns_len);
  for (uint32_t dss = 0; dss < SRSRAN_NOF_DELTA_SS; dss++) {
    const uint32_t c_init = ((cell.id / 30) << 5) + (((cell.id % 30) + dss) % 30);
    gold(c_init, c.data(), ns_len);
    for (uint32_t ns = 0; ns < SRSRAN_NSLOTS_X_FRAME; ns++) {
      uint32_t n = 0;
      for (int i = 0; i < 8; i++) {
        n += (uint32_t)c[8 * nsymb_slot(cell.cp) * ns + i] << i;
      }
      h.n_prs[dss][ns] = n;
      h.v[ns][dss]     = c[ns];  // the first 20 bits of the same sequence
    }
  }
  gold(cell.id / 30, c.data(), 160);
  for (uint32_t ns = 0; ns < SRSRAN_NSLOTS_X_FRAME; ns++) {
    h.f_gh[ns] = 0;
    for (int i = 0; i < 8; i++) {
      h.f_gh[ns] += (uint32_t)c[8 * ns + i] << i;
    }
  }
}

uint32_t prime_below(uint32_t n)  // largest prime < n (srsran_prime_lower_than)
{
  for (uint32_t p = n - 1; p > 2; p--) {
    bool is = true;
    for (uint32_t d = 2; d * d <= p; d++) {
      if (p % d == 0) {
        is = false;
        break;
      }
    }
    if (is) {
      return p;
    }
  }
  return 2;
}

// the Zadoff-Chu root q of group u, base sequence v, in the float arithmetic of zc_sequence.c:214-227
float zc_root(uint32_t u, uint32_t v, uint32_t Nzc)
{
  const float q_hat = (float)Nzc * (float)(u + 1) / 31.0f;
  const float qf    = (((uint32_t)(2 * q_hat)) % 2 == 0) ? (float)(q_hat + 0.5 + v) : (float)(q_hat + 0.5 - v);
  return (float)(uint32_t)qf;
}

// base sequence r_uv(n) e^{j alpha n} of 36.211 5.5.1, float arithmetic of zc_sequence.c:214-311
// fused: fl(arg + alpha i) with one rounding, as the reference's -mfma build evaluates it (the SRS, whose fixtures
// record that build); otherwise alpha i is rounded first
void zc_sequence(uint32_t u, uint32_t v, float alpha, uint32_t nof_prb, cf_t* out, bool fused = false)
{
  const uint32_t     Mzc = nof_prb * SRSRAN_NRE;
  std::vector<float> arg(Mzc);
  if (Mzc == 12 || Mzc == 24) {
    const int8_t* phi = Mzc == 12 ? kZcPhi12[u] : kZcPhi24[u];
    for (uint32_t i = 0; i < Mzc; i++) {
      arg[i] = (float)phi[i] * (float)M_PI_4;
    }
  } else {
    const uint32_t Nzc  = prime_below(Mzc);
    const float    n_sz = (float)Nzc;
    const float    q    = zc_root(u, v, Nzc);
    for (uint32_t i = 0; i < Mzc; i++) {
      const float m = (float)(i % Nzc);
      arg[i]        = (float)(-M_PI * q * m * (m + 1) / n_sz);
    }
  }
  for (uint32_t i = 0; i < Mzc; i++) {
    float s, c;
    sincosf(fused ? fmaf(alpha, (float)i, arg[i]) : arg[i] + alpha * (float)i, &s, &c);
    out[i] = cf_t{c, s};
  }
}

int dmrs_gen(const srsran_cell_t& cell, const UlHopping& h, const srsran_refsignal_dmrs_pusch_cfg_t& cfg,
             uint32_t nof_prb, uint32_t sf_idx, uint32_t cs_dmrs, cf_t* r)
{
  if (cfg.cyclic_shift >= SRSRAN_NOF_CSHIFT || cfg.delta_ss >= SRSRAN_NOF_DELTA_SS || nof_prb > cell.nof_prb ||
      cs_dmrs >= SRSRAN_NOF_CSHIFT || sf_idx >= SRSRAN_NOF_SF_X_FRAME || nof_prb == 0) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  for (uint32_t ns = 2 * sf_idx; ns < 2 * (sf_idx + 1); ns++) {
    const uint32_t n_cs  = (kNdmrs1[cfg.cyclic_shift] + kNdmrs2[cs_dmrs] + h.n_prs[cfg.delta_ss][ns]) % 12;
    const float    alpha = (float)(2 * M_PI * n_cs / 12);
    const uint32_t u     = ((cfg.group_hopping_en ? h.f_gh[ns] : 0) + (cell.id % 30) + cfg.delta_ss) % 30;
    const uint32_t v     = (nof_prb >= 6 && cfg.sequence_hopping_en) ? h.v[ns][cfg.delta_ss] : 0;
    zc_sequence(u, v, alpha, nof_prb, r + (ns % 2) * SRSRAN_NRE * nof_prb);
  }
  return SRSRAN_SUCCESS;
}

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

// the sounding reference signal's host side, further down
bool     srs_cfg_valid(const srsran_refsignal_srs_cfg_t& c, uint32_t nof_prb);
uint32_t srs_M_sc(const srsran_refsignal_srs_cfg_t& c, uint32_t nof_prb);

// ---------------- chest_ul device state ----------------
struct ChestUlGpu {
  hipStream_t         stream = nullptr;
  uint32_t            max_prb = 0;
  UlHopping           hop;
  bool                hop_ok = false;
  DevBuf<float2>      d_dmrs;    // [cs][sf][valid n <= cell prb] 2 * 12 n values
  std::vector<size_t> dmrs_off;  // (cs * 10 + sf) * 101 + n -> offset (values)
  DevBuf<float2>      d_grid;    // one subframe grid
  DevBuf<PuschUe>     d_desc;
  // srsran_chest_ul_pregen with an SRS configuration: the known sequence comes from these (chest_ul.c:633-634)
  bool                              srs_configured = false;
  srsran_refsignal_srs_cfg_t        srs_cfg;
  srsran_refsignal_dmrs_pusch_cfg_t srs_dmrs_cfg;
  DevBuf<uint8_t>                   d_srs_desc;  // the SRS descriptors of a batch this object's scratch serves
};

struct ChestUlResGpu {
  DevBuf<float2>     d_ce;  // nof_re values
  DevBuf<ChestUlOut> d_out;
  uint32_t    nof_re = 0;
  bool        valid  = false;   // d_ce holds the last estimate written to ce
  // an SRS estimate enqueued on the device side and not yet fetched: where its ce row lies and how long it is
  bool        srs_pending = false;
  size_t      srs_off = 0;
  uint32_t    srs_n = 0;
};

size_t dmrs_index(uint32_t cs, uint32_t sf, uint32_t n) { return ((size_t)cs * SRSRAN_NOF_SF_X_FRAME + sf) * 101 + n; }

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
  const float w = q->smooth_filter[0];
  const float a = (float)(7.419 * w * w + 0.1117 * w - 0.005387);
  u.noise_div   = (double)a * 0.8;
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

// check a PUSCH allocation against the estimator / cell (chest_ul.c:409-414, pusch.c:392-410)
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

// what the PUCCH estimator (pucch_api.cpp) needs of the chest objects: the stream, a device
// scratch of `bytes` (the grid buffer, grown), and a note that res->ce was rewritten on the host
namespace srsran_amd {
hipStream_t chest_ul_stream(srsran_chest_ul_t* q) { return q && q->gpu ? ((ChestUlGpu*)q->gpu)->stream : nullptr; }
void*       chest_ul_scratch(srsran_chest_ul_t* q, size_t bytes)
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

int srsran_refsignal_dmrs_pusch_gen_cell(const srsran_cell_t*               cell,
                                         srsran_refsignal_dmrs_pusch_cfg_t* cfg,
                                         uint32_t                           nof_prb,
                                         uint32_t                           sf_idx,
                                         uint32_t                           cyclic_shift_for_dmrs,
                                         cf_t*                              r_pusch)
{
  if (!cell || !cfg || !r_pusch || !cell_valid(*cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  UlHopping h;
  hopping_tables(*cell, h);
  return dmrs_gen(*cell, h, *cfg, nof_prb, sf_idx, cyclic_shift_for_dmrs, r_pusch);
}

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

  // ---- UL-SCH: every UE, with or without UCI, through the batched srsran_ulsch_decode (ulsch_batch.h):
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

}  // extern "C"

// ---------------- PUSCH transmit (pusch.c:178-181, 259-354) and the UE uplink (ue_ul.c) ----------------
namespace {

// One transmission of a batch: the PUSCH object of its cell, where its grid goes and, for the UE uplink path, the
// DMRS tables and the normalisation of its samples.
struct TxReq {
  srsran_pusch_t*                          pusch;
  const UlHopping*                         hop;  // DMRS put (null: none)
  const srsran_refsignal_dmrs_pusch_cfg_t* dmrs_cfg;
  srsran_ul_sf_cfg_t*                      sf;
  srsran_pusch_cfg_t*                      cfg;
  const srsran_uci_value_t*                uci;
  const uint8_t*                           d_data;
  float2*                                  d_grid;
  bool                                     zero_rest;
  const float2*                            samples_in;  // null: no normalisation stage
  float2*                                  samples_out;
  uint32_t                                 sf_len, norm_mode;
  float                                    norm_factor, force_peak;
};

// srsran_pusch_encode for n transmissions up to the grids: checks, the UL-SCH step, then one multiplexing launch and
// one transform-precoding launch over the batch.  desc / *d_desc: the descriptors (host copy, device array in
// owner's scratch) for the caller's later stages.  Nothing is launched when a transmission is refused.  extra:
// descriptors of the batch's other transmissions (PUCCH), appended after the n of PUSCH for the normalisation launch.
int pusch_tx_run(srsran_pusch_t* owner, uint32_t n, const TxReq* r, std::vector<PuschTxUe>& desc,
                 const PuschTxUe** d_desc, hipStream_t st, const std::vector<PuschTxUe>& extra = {})
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

// srs_tx_enabled (ue_ul.c:453-462): the subframe carries this UE's SRS when it is a cell-specific SRS subframe
// (srsran_refsignal_srs_send_cs, refsignal_ul.c:703-749, 36.211 Table 5.5.3.3-1) and a UE-specific one
// (srsran_refsignal_srs_send_ue, refsignal_ul.c:560-622, 36.213 Table 8.2-1).
bool srs_send_cs(uint32_t subframe_config, uint32_t sf_idx)
{
  static const uint32_t T_sfc[15] = {1, 2, 2, 5, 5, 5, 5, 5, 5, 10, 10, 10, 10, 10, 10};
  static const uint32_t Delta_sfc1[7] = {0, 0, 1, 0, 1, 2, 3}, Delta_sfc2[4] = {0, 1, 2, 3};
  if (subframe_config >= 15 || sf_idx >= 10) {
    return false;
  }
  const uint32_t m = sf_idx % T_sfc[subframe_config];
  if (subframe_config < 7) {
    return m == Delta_sfc1[subframe_config];
  } else if (subframe_config == 7) {
    return m == 0 || m == 1;
  } else if (subframe_config == 8) {
    return m == 2 || m == 3;
  } else if (subframe_config < 13) {
    return m == Delta_sfc2[subframe_config - 9];
  } else if (subframe_config == 13) {
    return !(m == 5 || m == 7 || m == 9);
  }
  return !(m == 7 || m == 9);
}

bool srs_send_ue(uint32_t I_srs, uint32_t tti)
{
  static const uint32_t first[9] = {0, 2, 7, 17, 37, 77, 157, 317, 637}, T_srs[8] = {2, 5, 10, 20, 40, 80, 160, 320};
  if (I_srs >= 637 || tti >= 10240) {
    return false;
  }
  uint32_t k = 0;
  while (I_srs >= first[k + 1]) {
    k++;
  }
  return (tti - (I_srs - first[k])) % T_srs[k] == 0;  // unsigned, as the reference's (tti - Toffset) % T_srs; tti >= 10240 above: the
                                                      // reference's helper answers an error there, which srs_tx_enabled does not take for 1
}

bool srs_tx_enabled(const srsran_refsignal_srs_cfg_t& srs, uint32_t tti)
{
  return srs.configured && srs_send_cs(srs.subframe_config, tti % 10) && srs_send_ue(srs.I_srs, tti);
}

// 36.211 Tables 5.5.3.2-1 .. -4 as refsignal_ul.c:65-92 holds them: m_SRS,b and N_b by [bandwidth table][b][C_SRS]
constexpr uint32_t kMsrs[4][4][8] = {
    {{36, 32, 24, 20, 16, 12, 8, 4}, {12, 16, 4, 4, 4, 4, 4, 4}, {4, 8, 4, 4, 4, 4, 4, 4}, {4, 4, 4, 4, 4, 4, 4, 4}},
    {{48, 48, 40, 36, 32, 24, 20, 16}, {24, 16, 20, 12, 16, 4, 4, 4}, {12, 8, 4, 4, 8, 4, 4, 4}, {4, 4, 4, 4, 4, 4, 4, 4}},
    {{72, 64, 60, 48, 48, 40, 36, 32}, {24, 32, 20, 24, 16, 20, 12, 16}, {12, 16, 4, 12, 8, 4, 4, 8}, {4, 4, 4, 4, 4, 4, 4, 4}},
    {{96, 96, 80, 72, 64, 60, 48, 48}, {48, 32, 40, 24, 32, 20, 24, 16}, {24, 16, 20, 12, 16, 4, 12, 8}, {4, 4, 4, 4, 4, 4, 4, 4}}};
constexpr uint32_t kNb[4][4][8] = {
    {{1, 1, 1, 1, 1, 1, 1, 1}, {3, 2, 6, 5, 4, 3, 2, 1}, {3, 2, 1, 1, 1, 1, 1, 1}, {1, 2, 1, 1, 1, 1, 1, 1}},
    {{1, 1, 1, 1, 1, 1, 1, 1}, {2, 3, 2, 3, 2, 6, 5, 4}, {2, 2, 5, 3, 2, 1, 1, 1}, {3, 2, 1, 1, 2, 1, 1, 1}},
    {{1, 1, 1, 1, 1, 1, 1, 1}, {3, 2, 3, 2, 3, 2, 3, 2}, {2, 2, 5, 2, 2, 5, 3, 2}, {3, 4, 1, 3, 2, 1, 1, 2}},
    {{1, 1, 1, 1, 1, 1, 1, 1}, {2, 3, 2, 3, 2, 3, 2, 3}, {2, 2, 2, 2, 2, 5, 2, 2}, {6, 4, 5, 3, 4, 1, 3, 2}}};

// refsignal_ul.c:751-762: the table by the cell's bandwidth
uint32_t srs_bw_table(uint32_t nof_prb) { return nof_prb <= 40 ? 0 : nof_prb <= 60 ? 1 : nof_prb <= 80 ? 2 : 3; }

uint32_t srs_T(uint32_t I_srs)  // 36.213 Table 8.2-1 (refsignal_ul.c:560-584), 0 from 637 on
{
  static const uint32_t first[9] = {0, 2, 7, 17, 37, 77, 157, 317, 637}, T_srs[8] = {2, 5, 10, 20, 40, 80, 160, 320};
  for (uint32_t k = 0; k < 8; k++) {
    if (I_srs < first[k + 1]) {
      return T_srs[k];
    }
  }
  return 0;
}

bool srs_cfg_valid(const srsran_refsignal_srs_cfg_t& c, uint32_t nof_prb)
{
  return c.bw_cfg < 8 && c.B < 4 && c.b_hop < 4 && c.k_tc < 2 && c.n_srs < 8 && c.n_rrc < 24 && c.subframe_config < 15 &&
         c.I_srs < 637 && kMsrs[srs_bw_table(nof_prb)][0][c.bw_cfg] <= nof_prb;
}

uint32_t srs_M_sc(const srsran_refsignal_srs_cfg_t& c, uint32_t nof_prb)
{
  return kMsrs[srs_bw_table(nof_prb)][c.B][c.bw_cfg] * SRSRAN_NRE / 2;
}

// srs_Fb (refsignal_ul.c:782-802).  The odd branch keeps the reference's form: floor(N_b / 2) (n_SRS / prod), without
// the outer floor of 36.211 5.5.3.2 (n_SRS / prod is an integer quotient already).
uint32_t srs_Fb(const srsran_refsignal_srs_cfg_t& c, uint32_t b, uint32_t nof_prb, uint32_t tti)
{
  const uint32_t T = srs_T(c.I_srs), t = srs_bw_table(nof_prb);
  if (!T) {
    return 0;
  }
  const uint32_t n_srs = tti / T, N_b = kNb[t][b][c.bw_cfg];
  uint32_t       prod_1 = 1;
  for (uint32_t bp = c.b_hop + 1; bp < b; bp++) {
    prod_1 *= kNb[t][bp][c.bw_cfg];
  }
  const uint32_t prod_2 = prod_1 * N_b;
  if (N_b % 2 == 0) {
    return (N_b / 2) * ((n_srs % prod_2) / prod_1) + ((n_srs % prod_2) / prod_1 / 2);
  }
  return (N_b / 2) * (n_srs / prod_1);
}

// srs_k0_ue (refsignal_ul.c:805-825) of a valid configuration
uint32_t srs_k0(const srsran_refsignal_srs_cfg_t& c, uint32_t nof_prb, uint32_t tti)
{
  const uint32_t t  = srs_bw_table(nof_prb);
  uint32_t       k0 = (nof_prb / 2 - kMsrs[t][0][c.bw_cfg] / 2) * SRSRAN_NRE + c.k_tc;
  for (uint32_t b = 0; b <= c.B; b++) {
    const uint32_t m_srs = kMsrs[t][b][c.bw_cfg], m_sc = m_srs * SRSRAN_NRE / 2;
    uint32_t       nb    = 4 * c.n_rrc / m_srs;
    if (b > c.b_hop) {
      nb += srs_Fb(c, b, nof_prb, tti);
    }
    k0 += 2 * m_sc * (nb % kNb[t][b][c.bw_cfg]);
  }
  return k0;
}

// What compute_r (refsignal_ul.c:229-252) hands to srsran_zc_sequence_generate_lte for the SRS of slot ns
// (refsignal_ul.c:882-883): nof_prb = M_sc / 12, delta_ss = 0 in u, the DMRS configuration's delta_ss in the row of v.
void srs_uv(const srsran_cell_t& cell, const UlHopping& h, const srsran_refsignal_dmrs_pusch_cfg_t& d, uint32_t M_sc,
            uint32_t ns, uint32_t* u, uint32_t* v)
{
  *u = ((d.group_hopping_en ? h.f_gh[ns] : 0) + (cell.id % 30)) % 30;
  *v = (M_sc / SRSRAN_NRE >= 6 && d.sequence_hopping_en) ? h.v[ns][d.delta_ss] : 0;
}

float srs_alpha(uint32_t n_srs) { return (float)(2 * M_PI * n_srs / 8); }

// The sequence of subframe sf_idx for the kernels: that of slot 2 sf_idx
SrsSeq srs_seq(const srsran_cell_t& cell, const UlHopping& h, uint32_t n_srs, const srsran_refsignal_dmrs_pusch_cfg_t& d,
               uint32_t m_sc, uint32_t sf_idx)
{
  SrsSeq q;
  memset(&q, 0, sizeof(q));
  uint32_t u, v;
  srs_uv(cell, h, d, m_sc, 2 * sf_idx, &u, &v);
  q.alpha = srs_alpha(n_srs);
  if (m_sc == 24) {
    memcpy(q.phi, kZcPhi24[u], 24);
  } else {
    q.n_zc = prime_below(m_sc);
    q.q    = zc_root(u, v, q.n_zc);
  }
  return q;
}

// The descriptor of the UE's SRS in subframe tti: the sequence of slot 2 (tti % 10) (srsran_refsignal_srs_put maps the
// first of the two sequences srsran_refsignal_srs_gen writes, also in the last symbol of slot 1).  grid is left null.
int srs_tx_prepare(const srsran_cell_t& cell, const UlHopping& h, const srsran_refsignal_srs_cfg_t& c,
                   const srsran_refsignal_dmrs_pusch_cfg_t& d, uint32_t tti, SrsTxUe* out)
{
  if (!srs_cfg_valid(c, cell.nof_prb) || d.delta_ss >= SRSRAN_NOF_DELTA_SS) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  SrsTxUe s;
  memset(&s, 0, sizeof(s));
  s.ncell_re = cell.nof_prb * SRSRAN_NRE;
  s.nsym     = 2 * nsymb_slot(cell.cp);
  s.m_sc     = srs_M_sc(c, cell.nof_prb);
  s.k0       = srs_k0(c, cell.nof_prb, tti);
  if (s.m_sc == 0 || s.k0 + 2 * (s.m_sc - 1) >= s.ncell_re) {  // the comb stays inside the last symbol's row
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  s.seq = srs_seq(cell, h, c.n_srs, d, s.m_sc, tti % SRSRAN_NOF_SF_X_FRAME);
  *out  = s;
  return SRSRAN_SUCCESS;
}

}  // namespace

extern "C" {

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

int srsran_refsignal_dmrs_pusch_put_cell(const srsran_cell_t* cell,
                                         srsran_pusch_cfg_t*  pusch_cfg,
                                         cf_t*                r_pusch,
                                         cf_t*                sf_symbols)
{
  if (!cell || !pusch_cfg || !r_pusch || !sf_symbols || !cell_valid(*cell) ||
      check_alloc(*cell, pusch_cfg) != SRSRAN_SUCCESS) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t M = pusch_cfg->grant.L_prb * SRSRAN_NRE;
  for (uint32_t ns = 0; ns < 2; ns++) {
    const uint32_t L = SRSRAN_REFSIGNAL_UL_L(ns, cell->cp);
    memcpy(sf_symbols + (size_t)L * cell->nof_prb * SRSRAN_NRE + pusch_cfg->grant.n_prb_tilde[ns] * SRSRAN_NRE,
           r_pusch + ns * M, M * sizeof(cf_t));
  }
  return SRSRAN_SUCCESS;
}

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

// refsignal_ul.c:625-642: format 1x is shortened in the cell's SRS subframes when ACK and SRS may coincide
void srsran_refsignal_srs_pucch_shortened_cfg(srsran_ul_sf_cfg_t*         sf,
                                              srsran_refsignal_srs_cfg_t* srs_cfg,
                                              srsran_pucch_cfg_t*         pucch_cfg)
{
  sf->shortened = srs_cfg->configured && pucch_cfg->format < SRSRAN_PUCCH_FORMAT_2 && srs_cfg->simul_ack &&
                  srs_send_cs(srs_cfg->subframe_config, sf->tti % 10);
}

// ---------------- sounding reference signal, host side (refsignal_ul.c:560-622, 644-830, 870-924) ----------------
bool srsran_refsignal_srs_cfg_isvalid(const srsran_refsignal_srs_cfg_t* cfg, uint32_t nof_prb)
{
  return cfg && nof_prb >= 6 && nof_prb <= SRSRAN_MAX_PRB && srs_cfg_valid(*cfg, nof_prb);
}

int srsran_refsignal_srs_send_cs(uint32_t subframe_config, uint32_t sf_idx)
{
  if (subframe_config >= 15 || sf_idx >= 10) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  return srs_send_cs(subframe_config, sf_idx) ? 1 : 0;
}

int srsran_refsignal_srs_send_ue(uint32_t I_srs, uint32_t tti)
{
  if (I_srs >= 1024 || tti >= 10240) {  // refsignal_ul.c:592: from 637 to 1023 the answer is 0, not an error
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  return srs_send_ue(I_srs, tti) ? 1 : 0;
}

// refsignal_ul.c:765-780; unsigned as there: it wraps where m_SRS,0 > nof_prb, which srs_cfg_isvalid refuses
uint32_t srsran_refsignal_srs_rb_start_cs(uint32_t bw_cfg, uint32_t nof_prb)
{
  return bw_cfg < 8 ? nof_prb / 2 - kMsrs[srs_bw_table(nof_prb)][0][bw_cfg] / 2 : 0;
}

uint32_t srsran_refsignal_srs_rb_L_cs(uint32_t bw_cfg, uint32_t nof_prb)
{
  return bw_cfg < 8 ? kMsrs[srs_bw_table(nof_prb)][0][bw_cfg] : 0;
}

uint32_t srsran_refsignal_srs_M_sc_cell(const srsran_cell_t* cell, const srsran_refsignal_srs_cfg_t* cfg)
{
  return cell && srsran_refsignal_srs_cfg_isvalid(cfg, cell->nof_prb) ? srs_M_sc(*cfg, cell->nof_prb) : 0;
}

uint32_t srsran_refsignal_srs_k0_cell(const srsran_cell_t* cell, const srsran_refsignal_srs_cfg_t* cfg, uint32_t tti)
{
  return cell && srsran_refsignal_srs_cfg_isvalid(cfg, cell->nof_prb) ? srs_k0(*cfg, cell->nof_prb, tti) : 0;
}

// refsignal_ul.c:644-697
void srsran_refsignal_srs_pusch_shortened_cfg(const srsran_cell_t*        cell,
                                              srsran_ul_sf_cfg_t*         sf,
                                              srsran_refsignal_srs_cfg_t* srs_cfg,
                                              srsran_pusch_cfg_t*         pusch_cfg)
{
  bool shortened = false;
  if (pusch_cfg->grant.is_rar) {  // no SRS with a RAR grant or its retransmissions
    sf->shortened = false;
    return;
  }
  if (srs_cfg->configured) {
    const uint32_t k0_srs = srsran_refsignal_srs_rb_start_cs(srs_cfg->bw_cfg, cell->nof_prb);
    const uint32_t nrb    = srsran_refsignal_srs_rb_L_cs(srs_cfg->bw_cfg, cell->nof_prb);
    const uint32_t L      = pusch_cfg->grant.L_prb;
    const bool     cs     = srs_send_cs(srs_cfg->subframe_config, sf->tti % 10);
    if (cs && srs_send_ue(srs_cfg->I_srs, sf->tti)) {
      // the UE's own SRS subframe: shortened, overlapping or not, unless the allocation is contiguous to the region
      shortened = true;
      for (uint32_t ns = 0; ns < 2 && shortened; ns++) {
        const uint32_t n = pusch_cfg->grant.n_prb_tilde[ns];
        if (n == k0_srs + nrb || n + L == k0_srs) {
          shortened = false;
        }
      }
    }
    if (!shortened && cs) {  // a cell SRS subframe: shortened where the allocation meets the cell's SRS region
      for (uint32_t ns = 0; ns < 2 && !shortened; ns++) {
        const uint32_t n = pusch_cfg->grant.n_prb_tilde[ns];
        if ((n >= k0_srs && n < k0_srs + nrb) || (n + L > k0_srs && n + L < k0_srs + nrb) ||
            (n <= k0_srs && n + L >= k0_srs + nrb)) {
          shortened = true;
        }
      }
    }
  }
  sf->shortened = shortened;
}

// refsignal_ul.c:870-888: the sequences of both slots of the subframe, M_sc values each
int srsran_refsignal_srs_gen_cell(const srsran_cell_t*               cell,
                                  srsran_refsignal_srs_cfg_t*        cfg,
                                  srsran_refsignal_dmrs_pusch_cfg_t* pusch_cfg,
                                  uint32_t                           sf_idx,
                                  cf_t*                              r_srs)
{
  if (!cell || !cfg || !pusch_cfg || !r_srs || !cell_valid(*cell) || sf_idx >= SRSRAN_NOF_SF_X_FRAME ||
      !srs_cfg_valid(*cfg, cell->nof_prb) || pusch_cfg->delta_ss >= SRSRAN_NOF_DELTA_SS) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  UlHopping h;
  hopping_tables(*cell, h);
  const uint32_t M_sc = srs_M_sc(*cfg, cell->nof_prb);
  for (uint32_t ns = 2 * sf_idx; ns < 2 * (sf_idx + 1); ns++) {
    uint32_t u, v;
    srs_uv(*cell, h, *pusch_cfg, M_sc, ns, &u, &v);
    zc_sequence(u, v, srs_alpha(cfg->n_srs), M_sc / SRSRAN_NRE, r_srs + (ns % 2) * M_sc, true);
  }
  return SRSRAN_SUCCESS;
}

namespace {
// refsignal_ul.c:890-924: the comb of the last symbol, from or to the first M_sc values of r_srs
int srs_put_get(const srsran_cell_t* cell, srsran_refsignal_srs_cfg_t* cfg, uint32_t tti, cf_t* r_srs, cf_t* sf_symbols,
                bool put)
{
  if (!cell || !cfg || !r_srs || !sf_symbols || !cell_valid(*cell) || !srs_cfg_valid(*cfg, cell->nof_prb)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t M_sc = srs_M_sc(*cfg, cell->nof_prb), k0 = srs_k0(*cfg, cell->nof_prb, tti);
  const uint32_t ncell = cell->nof_prb * SRSRAN_NRE;
  if (k0 + 2 * (M_sc - 1) >= ncell) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  cf_t* row = sf_symbols + (size_t)(2 * nsymb_slot(cell->cp) - 1) * ncell + k0;
  for (uint32_t i = 0; i < M_sc; i++) {
    if (put) {
      row[2 * i] = r_srs[i];
    } else {
      r_srs[i] = row[2 * i];
    }
  }
  return SRSRAN_SUCCESS;
}
}  // namespace

int srsran_refsignal_srs_put_cell(const srsran_cell_t* cell, srsran_refsignal_srs_cfg_t* cfg, uint32_t tti, cf_t* r_srs,
                                  cf_t* sf_symbols)
{
  return srs_put_get(cell, cfg, tti, r_srs, sf_symbols, true);
}

int srsran_refsignal_srs_get_cell(const srsran_cell_t* cell, srsran_refsignal_srs_cfg_t* cfg, uint32_t tti, cf_t* r_srs,
                                  cf_t* sf_symbols)
{
  return srs_put_get(cell, cfg, tti, r_srs, sf_symbols, false);
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
    const float w = q->smooth_filter[0];  // estimate_noise_pilots' calibration (chest_ul.c:220-225)
    u.noise_div   = (double)(float)(7.419 * w * w + 0.1117 * w - 0.005387) * 0.8;
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
