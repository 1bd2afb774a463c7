// srsran_4g_amd/csrc/pucch_api.cpp -- C-ABI of the PUCCH receive path (include/srsran_pucch.h):
// the resource helpers of pucch.c:943-1264, pucch_proc.c and refsignal_ul.c:360-429 restated on the
// host (the per-cell tables are in refsignal_ul_api.cpp), srsran_chest_ul_estimate_pucch (chest_ul.c:462-610), srsran_pucch_decode (pucch.c:797-872)
// and srsran_pucch_gpu_get_batch (the sequence of enb_ul.c:156-273 for many UEs), over the kernel
// of pucch_kernel.hip; and the transmit side of the UE (pucch.c:583-623, 768-794, refsignal_ul.c:432-552):
// srsran_pucch_init_ue, srsran_pucch_encode and the DMRS generation / mapping over pucch_tx_kernel.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/srsran_pucch.h"
#include "dev_buf.h"
#include "lte_seq_host.h"
#include "pucch_kernel.h"
#include "pucch_tx_kernel.h"
#include "ul_internal.h"

using namespace srsran_amd;

namespace {

bool     is_f1(srsran_pucch_format_t f) { return f == SRSRAN_PUCCH_FORMAT_1 || f == SRSRAN_PUCCH_FORMAT_1A || f == SRSRAN_PUCCH_FORMAT_1B; }
bool     is_f2(srsran_pucch_format_t f) { return f == SRSRAN_PUCCH_FORMAT_2 || f == SRSRAN_PUCCH_FORMAT_2A || f == SRSRAN_PUCCH_FORMAT_2B; }

// the first 48 bits of srsran_sequence_pucch (sequences.c:169-172), bit i of the result is c(i)
uint64_t pucch_scrambling(uint16_t rnti, uint32_t tti, uint32_t cell_id)
{
  const uint32_t nslot = 2 * (tti % 10);
  uint32_t       w[2];
  gold_words((((nslot / 2) + 1) * (2 * cell_id + 1) << 16) + rnti, w, 48);
  return (uint64_t)w[1] << 32 | w[0];
}

// ---- cyclic shifts (pucch.c:1149-1234); the public alpha is 2 pi n_cs / 12
uint32_t ncs_format1(const ncs_table_t         n_cs_cell,
                     const srsran_pucch_cfg_t* cfg,
                     srsran_cp_t               cp,
                     bool                      is_dmrs,
                     uint32_t                  ns,
                     uint32_t                  l,
                     uint32_t*                 n_oc_ptr,
                     uint32_t*                 n_prime_ns)
{
  const uint32_t c = cp == SRSRAN_CP_NORM ? 3 : 2, ds = cfg->delta_pucch_shift;
  const uint32_t edge    = c * cfg->N_cs / ds;  // resources of the mixed PRB
  const bool     mixed   = cfg->n_pucch < edge;
  const uint32_t N_prime = mixed ? cfg->N_cs : SRSRAN_NRE;
  uint32_t       n_prime = mixed ? (uint32_t)cfg->n_pucch : (cfg->n_pucch - edge) % (c * SRSRAN_NRE / ds);
  if (ns % 2) {
    if (!mixed) {
      n_prime = (c * (n_prime + 1)) % (c * SRSRAN_NRE / ds + 1) - 1;
    } else {
      const uint32_t dd = cp == SRSRAN_CP_NORM ? 2 : 0;
      const uint32_t h  = (n_prime + dd) % (c * N_prime / ds);
      n_prime           = (h / c) + (h % c) * N_prime / ds;
    }
  }
  if (n_prime_ns) {
    *n_prime_ns = n_prime;
  }
  const bool data_ext = !is_dmrs && cp == SRSRAN_CP_EXT;
  uint32_t   n_oc     = (n_prime * ds) / N_prime;
  if (data_ext) {
    n_oc *= 2;
  }
  if (n_oc_ptr) {
    *n_oc_ptr = n_oc;
  }
  const uint32_t shift = cp == SRSRAN_CP_NORM ? n_oc % ds : n_oc / (data_ext ? 2 : 1);
  return (n_cs_cell[ns][l] + (n_prime * ds + shift) % N_prime) % SRSRAN_NRE;
}

uint32_t ncs_format2(const ncs_table_t n_cs_cell, const srsran_pucch_cfg_t* cfg, uint32_t ns, uint32_t l)
{
  const bool mixed   = cfg->n_pucch >= SRSRAN_NRE * cfg->n_rb_2;
  uint32_t   n_prime = mixed ? (cfg->n_pucch + cfg->N_cs + 1) % SRSRAN_NRE : cfg->n_pucch % SRSRAN_NRE;
  if (ns % 2) {
    n_prime = (SRSRAN_NRE * (n_prime + 1)) % (SRSRAN_NRE + 1) - 1;
    if (mixed) {
      const int x = (SRSRAN_NRE - 2 - (int)cfg->n_pucch) % SRSRAN_NRE;
      n_prime     = x >= 0 ? (uint32_t)x : (uint32_t)(SRSRAN_NRE + x);
    }
  }
  return (n_cs_cell[ns][l] + n_prime) % SRSRAN_NRE;
}

// Table 5.4.3-1 data symbols and N_SF of each slot (pucch.c:206-318)
const uint8_t kDataSymF1[2][4] = {{0, 1, 5, 6}, {0, 1, 4, 5}};
const uint8_t kDataSymF2[2][5] = {{0, 2, 3, 4, 6}, {0, 1, 2, 4, 5}};
// orthogonal cover phases in units of pi / 12: Tables 5.4.1-2 / -3 (data), 5.5.2.2.1-2 (DMRS)
const uint8_t kDataW[2][3][4] = {{{0, 0, 0, 0}, {0, 12, 0, 12}, {0, 12, 12, 0}}, {{0, 0, 0, 0}, {0, 8, 16, 0}, {0, 16, 8, 0}}};
const uint8_t kRsWNorm[3][3]  = {{0, 0, 0}, {0, 8, 16}, {0, 16, 8}};
const uint8_t kRsWExt[3][2]   = {{0, 0}, {0, 12}, {0, 0}};

uint32_t n_sf(srsran_pucch_format_t f, uint32_t slot, bool shortened)
{
  if (is_f1(f)) {
    return slot && shortened ? 3 : 4;
  }
  if (is_f2(f)) {
    return 5;
  }
  if (f == SRSRAN_PUCCH_FORMAT_3) {
    return slot && shortened ? 4 : 5;
  }
  return 0;
}

// Everything the kernel needs of one (cell, subframe, cfg->format, cfg->n_pucch).  Returns the
// reference's error for what it refuses (N_rs == 0, PRB outside the cell).
int build_cand(const srsran_cell_t&      cell,
               const CellTables&         t,
               const srsran_chest_ul_t*  chest,
               const srsran_ul_sf_cfg_t* sf,
               srsran_pucch_cfg_t*       cfg,
               PucchCand&                c)
{
  memset(&c, 0, sizeof(c));
  const srsran_pucch_format_t f = cfg->format;
  if (cfg->delta_pucch_shift == 0) {  // divides the format 1x resource arithmetic
    return SRSRAN_ERROR;
  }
  c.n_rs                        = srsran_refsignal_dmrs_N_rs(f, cell.cp);
  if (!c.n_rs) {
    return SRSRAN_ERROR;
  }
  const uint32_t ext = cell.cp == SRSRAN_CP_NORM ? 0 : 1, sf_idx = sf->tti % 10;
  c.format    = (uint32_t)f;
  c.ncell_re  = cell.nof_prb * SRSRAN_NRE;
  c.nsym_slot = nsymb_slot(cell.cp);
  for (uint32_t m = 0; m < c.n_rs; m++) {
    c.rs_sym[m] = (uint8_t)srsran_refsignal_dmrs_pucch_symbol(m, f, cell.cp);
  }
  for (uint32_t i = 0; i < PUCCH_MAX_SF; i++) {
    c.data_sym[i] = is_f1(f) ? (i < 4 ? kDataSymF1[ext][i] : 0) : kDataSymF2[ext][i];
  }
  for (uint32_t s = 0; s < 2; s++) {
    const uint32_t ns = 2 * sf_idx + s;
    c.n_sf[s]         = n_sf(f, s, sf->shortened);
    c.n_prb[s]        = srsran_pucch_n_prb(&cell, cfg, s);
    if (c.n_prb[s] >= cell.nof_prb) {
      fprintf(stderr, "[srsran_pucch] Invalid PUCCH n_prb=%u\n", c.n_prb[s]);
      return SRSRAN_ERROR;
    }
    const uint32_t u = ((cfg->group_hopping_en ? t.f_gh[ns] : 0) + (cell.id % 30)) % 30;
    memcpy(c.phi[s], zc_phi12(u), 12);
    for (uint32_t m = 0; m < c.n_rs; m++) {
      const uint32_t l = c.rs_sym[m];
      if (is_f1(f)) {
        uint32_t n_oc  = 0;
        c.rs_ncs[s][m] = (uint8_t)ncs_format1(t.n_cs_cell, cfg, cell.cp, true, ns, l, &n_oc, nullptr);
        if (n_oc > 2) {
          return SRSRAN_ERROR;
        }
        c.rs_ph[s][m] = ext ? kRsWExt[n_oc][m] : kRsWNorm[n_oc][m];
      } else {
        c.rs_ncs[s][m] = (uint8_t)ncs_format2(t.n_cs_cell, cfg, ns, l);
      }
    }
    for (uint32_t i = 0; i < c.n_sf[s]; i++) {
      const uint32_t l = c.data_sym[i];
      if (is_f1(f)) {
        // pucch.c:419 asks for the DMRS n_oc here too: with extended CP it is not doubled
        uint32_t n_oc = 0, n_prime = 0;
        c.data_ncs[s][i] = (uint8_t)ncs_format1(t.n_cs_cell, cfg, cell.cp, true, ns, l, &n_oc, &n_prime);
        c.data_ph[s][i]  = (uint8_t)(kDataW[c.n_sf[s] == 3 ? 1 : 0][n_oc % 3][i] + (n_prime % 2 ? 6 : 0));
      } else if (is_f2(f)) {
        c.data_ncs[s][i] = (uint8_t)ncs_format2(t.n_cs_cell, cfg, ns, l);
      } else {
        c.data_ncs[s][i] = (uint8_t)t.n_cs_cell[ns % SRSRAN_NSLOTS_X_FRAME][l];
      }
    }
  }
  if (f == SRSRAN_PUCCH_FORMAT_3) {  // pucch.c:520-524
    const uint32_t N1 = c.n_sf[1];
    c.f3_noc[0]       = (uint8_t)(cfg->n_pucch % N1);
    c.f3_noc[1]       = (uint8_t)(N1 == 5 ? (3 * cfg->n_pucch) % N1 : c.f3_noc[0] % N1);
  }
  if (f >= SRSRAN_PUCCH_FORMAT_2) {
    c.scr = pucch_scrambling(cfg->rnti, sf->tti, cell.id);
  }
  const int nof_cqi = srsran_cqi_size(&cfg->uci_cfg.cqi);
  c.nof_uci_bits    = cfg->uci_cfg.cqi.ri_len ? cfg->uci_cfg.cqi.ri_len : (uint32_t)nof_cqi;
  c.thr_format1     = cfg->threshold_format1;
  c.thr_format3     = cfg->threshold_data_valid_format3;
  c.thr_dmrs        = cfg->threshold_dmrs_detection;
  c.meas_ta         = cfg->meas_ta_en;
  if (chest) {
    c.filt[0]     = chest->smooth_filter[0];
    c.filt[1]     = chest->smooth_filter[1];
    c.filt[2]     = chest->smooth_filter[2];
    c.noise_div   = chest_ul_noise_div(chest->smooth_filter[0]);  // chest_ul.c:452-456
  }
  return SRSRAN_SUCCESS;
}

// what the estimator refuses before any work
int check_estimator(const srsran_chest_ul_t* q, const srsran_pucch_cfg_t* cfg)
{
  if (cfg->meas_ta_en && cfg->use_cedron_alg) {
    fprintf(stderr, "[srsran_chest_ul] the Cedron TA estimator is not provided\n");
    return SRSRAN_ERROR;
  }
  if (q->smooth_filter_len != 3) {
    fprintf(stderr, "[srsran_chest_ul] PUCCH estimation needs the 3-tap smoothing filter (len %u)\n", q->smooth_filter_len);
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

float to_dB(float x) { return 10.0f * log10f(x); }

// decode_bits and the validity rules of srsran_pucch_decode (pucch.c:730-765, 827-866) from the
// kernel's candidate result; drs: the pucch2_drs_bits of this candidate's estimate
void apply_decode(srsran_pucch_cfg_t* cfg, const PucchCandOut& o, const uint8_t* drs, srsran_pucch_res_t* data)
{
  if (o.dmrs_checked) {
    data->dmrs_correlation = o.dmrs_corr;
    if (o.dmrs_failed) {
      data->correlation = 0.0f;
      data->detected    = false;
      return;
    }
  }
  data->correlation = o.corr;
  const bool         found = o.found != 0;
  srsran_uci_value_t* uci  = &data->uci_data;
  uint8_t            pucch_bits[SRSRAN_CQI_MAX_BITS] = {};
  memcpy(pucch_bits, o.bits, sizeof(o.bits));
  if (cfg->format == SRSRAN_PUCCH_FORMAT_3) {
    const uint32_t nof_ack = srsran_uci_cfg_total_ack(&cfg->uci_cfg);
    memcpy(uci->ack.ack_value, pucch_bits, std::min<uint32_t>(nof_ack, SRSRAN_UCI_MAX_ACK_BITS));
    uci->scheduling_request = pucch_bits[nof_ack] == 1;
    uci->ack.valid          = found;
  } else {
    if (cfg->uci_cfg.is_scheduling_request_tti) {
      uci->scheduling_request = found;
    }
    const bool cqi_or_ri = cfg->uci_cfg.cqi.data_enable || cfg->uci_cfg.cqi.ri_len;
    for (uint32_t a = 0; a < srsran_pucch_nof_ack_format(cfg->format); a++) {
      uci->ack.ack_value[a] = cqi_or_ri ? drs[a] : pucch_bits[a];
    }
    if (cfg->uci_cfg.cqi.data_enable) {
      srsran_cqi_value_unpack(&cfg->uci_cfg.cqi, pucch_bits, &uci->cqi);
    }
    if (cfg->uci_cfg.cqi.ri_len) {
      uci->ri = pucch_bits[0];
    }
  }
  data->detected = found;
  if (cfg->format == SRSRAN_PUCCH_FORMAT_1A || cfg->format == SRSRAN_PUCCH_FORMAT_1B) {
    uci->ack.valid = data->correlation > cfg->threshold_data_valid_format1a;
  } else if (is_f2(cfg->format)) {
    data->detected     = data->correlation > cfg->threshold_data_valid_format2;
    uci->ack.valid     = data->detected;
    uci->cqi.data_crc  = data->detected;
  }
}

// the estimator's scalars in the forms chest_ul.c:522-606 leaves in srsran_chest_ul_res_t
struct ChestScalars {
  float epre_dBfs, noise_dbFs, snr_db;
};
ChestScalars chest_scalars(const PucchCandOut& o)
{
  ChestScalars s;
  s.epre_dBfs  = to_dB(o.epre);
  s.noise_dbFs = to_dB(o.noise) + 30.0f;
  s.snr_db     = isnormal(o.noise) ? to_dB(o.epre / o.noise) : NAN;
  return s;
}

// ---------------- device state of srsran_pucch_t ----------------
struct PucchGpu {
  hipStream_t   stream = nullptr;
  PinBuf<PucchCand>    h_cand;  // the four candidate buffers have one capacity (reserve below), d_out.cap()
  PinBuf<PucchCandOut> h_out;
  DevBuf<PucchCand>    d_cand;
  DevBuf<PucchCandOut> d_out;
  DevBuf<float2>       d_re;  // srsran_pucch_decode: gathered data REs and estimates; srsran_pucch_encode: z
  DevBuf<PucchTxUe>    d_tx;  // srsran_pucch_encode: the descriptor (allocated by the first call)
};

bool reserve(PucchGpu* g, uint32_t n)
{
  if (n <= g->d_out.cap()) {
    return true;
  }
  hipStreamSynchronize(g->stream);
  g->h_cand.reset(), g->h_out.reset(), g->d_cand.reset(), g->d_out.reset();
  const uint32_t m = std::max<uint32_t>(64, n + n / 2);
  return g->h_cand.reserve(m) && g->h_out.reserve(m) && g->d_cand.reserve(m) && g->d_out.reserve(m);
}

// one pass of get_pucch (enb_ul.c:156-231) planned on the host: format and candidate resources
struct PassPlan {
  srsran_pucch_format_t format;
  int                   nres;
  uint32_t              n_pucch[SRSRAN_PUCCH_MAX_ALLOC];
};

int plan_pass(const srsran_cell_t& cell, srsran_pucch_cfg_t* cfg, PassPlan& p)
{
  p.format = srsran_pucch_proc_select_format(&cell, cfg, &cfg->uci_cfg, NULL);
  if (p.format == SRSRAN_PUCCH_FORMAT_ERROR) {
    return SRSRAN_ERROR;
  }
  cfg->format = p.format;
  memset(p.n_pucch, 0, sizeof(p.n_pucch));
  p.nres = srsran_pucch_proc_get_resources(&cell, cfg, &cfg->uci_cfg, NULL, p.n_pucch);
  if (p.nres < 1 || p.nres > SRSRAN_PUCCH_CS_MAX_ACK) {
    fprintf(stderr, "[srsran_pucch] No PUCCH resource could be calculated (%d)\n", p.nres);
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

struct EntryPlan {
  uint32_t first;      // first candidate of the entry
  uint32_t npass;      // 2 when SR and ACK are both expected
  PassPlan pass[2];
  bool     cqi_dropped;
};

// get_pucch's loop over the candidates of one pass (enb_ul.c:181-228) from the kernel's results
void finish_pass(srsran_pucch_cfg_t* cfg, const PassPlan& p, const PucchCandOut* o, srsran_pucch_res_t* res)
{
  const uint32_t total_ack = srsran_uci_cfg_total_ack(&cfg->uci_cfg);
  cfg->format              = p.format;
  res->correlation         = 0.0f;
  for (int i = 0; i < p.nres; i++) {
    srsran_pucch_res_t r;
    memset(&r, 0, sizeof(r));
    cfg->n_pucch = (uint16_t)p.n_pucch[i];
    if (cfg->format == SRSRAN_PUCCH_FORMAT_2A || cfg->format == SRSRAN_PUCCH_FORMAT_2B) {
      cfg->pucch2_drs_bits[0] = o[i].drs_bits[0];
      cfg->pucch2_drs_bits[1] = o[i].drs_bits[1];
    }
    const ChestScalars s = chest_scalars(o[i]);
    r.snr_db             = s.snr_db;
    r.rssi_dbFs          = s.epre_dBfs;
    r.ni_dbFs            = s.noise_dbFs;
    apply_decode(cfg, o[i], cfg->pucch2_drs_bits, &r);
    if (total_ack > 0 && cfg->format == SRSRAN_PUCCH_FORMAT_1B &&
        cfg->ack_nack_feedback_mode == SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_CS &&
        !cfg->uci_cfg.is_scheduling_request_tti && r.uci_data.ack.valid) {
      const uint8_t b[2] = {r.uci_data.ack.ack_value[0], r.uci_data.ack.ack_value[1]};
      srsran_pucch_cs_get_ack(cfg, &cfg->uci_cfg, (uint32_t)i, b, &r.uci_data);
    }
    if (i == 0 || r.correlation > res->correlation) {
      if (cfg->meas_ta_en) {
        r.ta_valid = !(isnan(o[i].ta_us) || isinf(o[i].ta_us));
        r.ta_us    = o[i].ta_us;
      }
      *res = r;
    }
  }
}

}  // namespace

extern "C" {

// ---------------- host helpers ----------------
uint32_t srsran_pucch_m(const srsran_pucch_cfg_t* cfg, srsran_cp_t cp)
{
  if (is_f1(cfg->format)) {
    const uint32_t c = cp == SRSRAN_CP_NORM ? 3 : 2, edge = c * cfg->N_cs / cfg->delta_pucch_shift;
    if (cfg->n_pucch < edge) {
      return cfg->n_rb_2;
    }
    return (cfg->n_pucch - edge) / (c * SRSRAN_NRE / cfg->delta_pucch_shift) + cfg->n_rb_2 +
           (uint32_t)ceilf((float)cfg->N_cs / 8);
  }
  if (is_f2(cfg->format)) {
    return cfg->n_pucch / SRSRAN_NRE;
  }
  if (cfg->format == SRSRAN_PUCCH_FORMAT_3) {
    return cfg->n_pucch / 5;
  }
  return 0;
}

uint32_t srsran_pucch_n_prb(const srsran_cell_t* cell, const srsran_pucch_cfg_t* cfg, uint32_t ns)
{
  const uint32_t m = srsran_pucch_m(cfg, cell->cp);
  return (m + ns) % 2 ? cell->nof_prb - 1 - m / 2 : m / 2;
}

int srsran_pucch_n_cs_cell(srsran_cell_t cell, uint32_t n_cs_cell[SRSRAN_NSLOTS_X_FRAME][SRSRAN_CP_NORM_NSYMB])
{
  n_cs_cell_gen(cell, n_cs_cell);
  return SRSRAN_SUCCESS;
}

float srsran_pucch_alpha_format1(const uint32_t            n_cs_cell[SRSRAN_NSLOTS_X_FRAME][SRSRAN_CP_NORM_NSYMB],
                                 const srsran_pucch_cfg_t* cfg,
                                 srsran_cp_t               cp,
                                 bool                      is_dmrs,
                                 uint32_t                  ns,
                                 uint32_t                  l,
                                 uint32_t*                 n_oc,
                                 uint32_t*                 n_prime_ns)
{
  const uint32_t n_cs = ncs_format1(n_cs_cell, cfg, cp, is_dmrs, ns, l, n_oc, n_prime_ns);
  return (float)(2 * M_PI * n_cs / SRSRAN_NRE);
}

float srsran_pucch_alpha_format2(const uint32_t            n_cs_cell[SRSRAN_NSLOTS_X_FRAME][SRSRAN_CP_NORM_NSYMB],
                                 const srsran_pucch_cfg_t* cfg,
                                 uint32_t                  ns,
                                 uint32_t                  l)
{
  return (float)(2 * M_PI * ncs_format2(n_cs_cell, cfg, ns, l) / SRSRAN_NRE);
}

int srsran_pucch_format2ab_mod_bits(srsran_pucch_format_t format, uint8_t bits[2], cf_t* d_10)
{
  if (!d_10) {
    return SRSRAN_ERROR;
  }
  if (format == SRSRAN_PUCCH_FORMAT_2A) {
    *d_10 = cf_t(bits[0] ? -1.0f : 1.0f, 0.0f);
    return SRSRAN_SUCCESS;
  }
  if (format == SRSRAN_PUCCH_FORMAT_2B) {  // Table 5.4.2-1: 00: 1, 01: -j, 10: j, 11: -1
    static const cf_t tab[4] = {cf_t(1, 0), cf_t(0, -1), cf_t(0, 1), cf_t(-1, 0)};
    *d_10                    = tab[(bits[0] ? 2 : 0) + (bits[1] ? 1 : 0)];
    return SRSRAN_SUCCESS;
  }
  return SRSRAN_ERROR;
}

uint32_t srsran_pucch_nof_ack_format(srsran_pucch_format_t format)
{
  switch (format) {
    case SRSRAN_PUCCH_FORMAT_1A:
    case SRSRAN_PUCCH_FORMAT_2A:
      return 1;
    case SRSRAN_PUCCH_FORMAT_1B:
    case SRSRAN_PUCCH_FORMAT_2B:
      return 2;
    default:
      return 0;
  }
}

bool srsran_pucch_cfg_isvalid(srsran_pucch_cfg_t* cfg, uint32_t nof_prb)
{
  return cfg->delta_pucch_shift > 0 && cfg->delta_pucch_shift < 4 && cfg->N_cs < 8 &&
         (cfg->N_cs % cfg->delta_pucch_shift) == 0 && cfg->n_rb_2 <= nof_prb;
}

int srsran_pucch_collision(const srsran_cell_t* cell, const srsran_pucch_cfg_t* cfg1, const srsran_pucch_cfg_t* cfg2)
{
  if (!cell || !cfg1 || !cfg2) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (cfg1->format != cfg2->format) {
    return SRSRAN_SUCCESS;  // different formats cannot be compared
  }
  if (cfg1->n_pucch == cfg2->n_pucch) {
    return SRSRAN_ERROR;
  }
  if (srsran_pucch_m(cfg1, cell->cp) != srsran_pucch_m(cfg2, cell->cp)) {
    return SRSRAN_SUCCESS;  // different PRBs
  }
  const CellTables* t = cell_tables(*cell);
  if (is_f1(cfg1->format)) {
    uint32_t oc1 = 0, oc2 = 0, np1 = 0, np2 = 0;
    ncs_format1(t->n_cs_cell, cfg1, cell->cp, false, 0, 0, &oc1, &np1);
    ncs_format1(t->n_cs_cell, cfg2, cell->cp, false, 0, 0, &oc2, &np2);
    return (oc1 == oc2 && np1 % 2 == np2 % 2) ? SRSRAN_ERROR : SRSRAN_SUCCESS;
  }
  if (is_f2(cfg1->format)) {
    return ncs_format2(t->n_cs_cell, cfg1, 0, 0) == ncs_format2(t->n_cs_cell, cfg2, 0, 0) ? SRSRAN_ERROR : SRSRAN_SUCCESS;
  }
  if (cfg1->format == SRSRAN_PUCCH_FORMAT_3) {
    return cfg1->n_pucch % 5 == cfg2->n_pucch % 5 ? SRSRAN_ERROR : SRSRAN_SUCCESS;
  }
  return SRSRAN_ERROR;
}

int srsran_pucch_cfg_assert(const srsran_cell_t* cell, const srsran_pucch_cfg_t* cfg)
{
  if (!cell || !cfg) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  srsran_pucch_cfg_t a = *cfg, b = *cfg;
  a.format = b.format = SRSRAN_PUCCH_FORMAT_1B;
  a.n_pucch           = (uint16_t)cfg->N_pucch_1;
  b.n_pucch           = (uint16_t)cfg->n_pucch_sr;
  if (srsran_pucch_collision(cell, &a, &b) != SRSRAN_SUCCESS) {
    return SRSRAN_ERROR;
  }
  if (cfg->ack_nack_feedback_mode == SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_CS) {
    // every channel-selection resource against N_pucch_1, n_pucch_sr and its row neighbour
    for (uint32_t i = 0; i < SRSRAN_PUCCH_SIZE_AN_CS; i++) {
      for (uint32_t j = 0; j < SRSRAN_PUCCH_NOF_AN_CS; j++) {
        b.n_pucch               = (uint16_t)cfg->n1_pucch_an_cs[i][j];
        const uint32_t other[3] = {cfg->N_pucch_1, cfg->n_pucch_sr, cfg->n1_pucch_an_cs[i][(j + 1) % SRSRAN_PUCCH_NOF_AN_CS]};
        for (uint32_t k = 0; k < 3; k++) {
          a.n_pucch = (uint16_t)other[k];
          if (srsran_pucch_collision(cell, &a, &b) != SRSRAN_SUCCESS) {
            return SRSRAN_ERROR;
          }
        }
      }
    }
  }
  return SRSRAN_SUCCESS;
}

char* srsran_pucch_format_text(srsran_pucch_format_t format)
{
  static const char* text[] = {"Format 1", "Format 1A", "Format 1B", "Format 2", "Format 2A", "Format 2B", "Format 3"};
  return (char*)((uint32_t)format < 7 ? text[format] : "Format Error");
}

char* srsran_pucch_format_text_short(srsran_pucch_format_t format)
{
  static const char* text[] = {"1", "1a", "1b", "2", "2a", "2b", "3"};
  return (char*)((uint32_t)format < 7 ? text[format] : "Err");
}

srsran_pucch_format_t srsran_pucch_proc_select_format(const srsran_cell_t*      cell,
                                                      const srsran_pucch_cfg_t* cfg,
                                                      const srsran_uci_cfg_t*   uci_cfg,
                                                      const srsran_uci_value_t* uci_value)
{
  srsran_pucch_format_t format    = SRSRAN_PUCCH_FORMAT_ERROR;
  const uint32_t        total_ack = srsran_uci_cfg_total_ack(uci_cfg);
  // with a UCI value the SR bit itself decides, otherwise the SR opportunity
  const bool sr = uci_value ? uci_value->scheduling_request : uci_cfg->is_scheduling_request_tti;
  if (!uci_cfg->cqi.data_enable && uci_cfg->cqi.ri_len == 0) {
    if (cfg->ack_nack_feedback_mode == SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_PUCCH3 && total_ack > uci_cfg->ack[0].nof_acks) {
      format = SRSRAN_PUCCH_FORMAT_3;
    } else if (total_ack == 1) {
      format = SRSRAN_PUCCH_FORMAT_1A;
    } else if (total_ack >= 2 && total_ack <= 4) {
      format = SRSRAN_PUCCH_FORMAT_1B;  // with channel selection above 2
    } else if (sr) {
      format = SRSRAN_PUCCH_FORMAT_1;
    } else {
      fprintf(stderr, "[srsran_pucch] Error selecting PUCCH format: Unsupported number of ACK bits %u\n", total_ack);
    }
  } else if (total_ack == 0) {
    format = SRSRAN_PUCCH_FORMAT_2;
  } else if (total_ack == 1) {
    format = cell->cp == SRSRAN_CP_NORM ? SRSRAN_PUCCH_FORMAT_2A : SRSRAN_PUCCH_FORMAT_2B;
  } else if (total_ack == 2) {
    format = SRSRAN_PUCCH_FORMAT_2B;
  }
  if (format == SRSRAN_PUCCH_FORMAT_ERROR) {
    fprintf(stderr, "[srsran_pucch] Returned Error while selecting PUCCH format\n");
  }
  return format;
}

int srsran_pucch_proc_get_resources(const srsran_cell_t*      cell,
                                    const srsran_pucch_cfg_t* cfg,
                                    const srsran_uci_cfg_t*   uci_cfg,
                                    const srsran_uci_value_t* uci_value,
                                    uint32_t*                 n_pucch_i)
{
  if (!cfg || !cell || !uci_cfg || !n_pucch_i) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t total_ack = srsran_uci_cfg_total_ack(uci_cfg);
  const bool     sr        = uci_value ? uci_value->scheduling_request : uci_cfg->is_scheduling_request_tti;
  if (sr && cfg->format != SRSRAN_PUCCH_FORMAT_3) {
    n_pucch_i[0] = cfg->n_pucch_sr;
    return 1;
  }
  if (cfg->format < SRSRAN_PUCCH_FORMAT_2) {
    const srsran_uci_cfg_ack_t* ack = uci_cfg->ack;
    if (cfg->sps_enabled) {
      n_pucch_i[0] = cfg->n_pucch_1[ack[0].tpc_for_pucch % 4];
      return 1;
    }
    if (cell->frame_type == SRSRAN_TDD) {
      // 36.213 10.1.3: n = (M - m - 1) N_p + m N_p+1 + n_cce + N_pucch_1, N_p = nof_prb (12 p - 4) / 36;
      // the reference returns its invalid-inputs code after filling the list (pucch_proc.c:272-285)
      const uint32_t M = ack[0].tdd_ack_M;
      for (uint32_t m = 0; m < M; m++) {
        const uint32_t ncce = ack[0].ncce[m];
        n_pucch_i[m]        = 0;
        for (uint32_t p = 0; p < 4; p++) {
          const uint32_t Np  = p == 0 ? 0 : cell->nof_prb * (SRSRAN_NRE * p - 4) / 36;
          const uint32_t Np1 = cell->nof_prb * (SRSRAN_NRE * (p + 1) - 4) / 36;
          if (ncce >= Np && ncce < Np1) {
            n_pucch_i[m] = (M - m - 1) * Np + m * Np1 + ncce + cfg->N_pucch_1;
            break;
          }
        }
      }
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (cfg->ack_nack_feedback_mode == SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_CS) {
      // up to 4 resources n_pucch_j associated with HARQ-ACK(j), 36.213 10.1.2.2.1
      int k = 0;
      for (int i = 0; i < SRSRAN_PUCCH_CS_MAX_CARRIERS && k < SRSRAN_PUCCH_CS_MAX_ACK; i++) {
        for (uint32_t j = 0; j < ack[i].nof_acks && k < SRSRAN_PUCCH_CS_MAX_ACK; j++) {
          const uint32_t* row = cfg->n1_pucch_an_cs[ack[i].tpc_for_pucch % SRSRAN_PUCCH_SIZE_AN_CS];
          if (ack[i].grant_cc_idx == 0) {  // PDCCH on the primary cell
            n_pucch_i[k++] = ack[i].ncce[0] + cfg->N_pucch_1 + j;
          } else if (i == 0) {  // primary cell without PDCCH: higher-layer resource
            n_pucch_i[k++] = row[0] + j;
          } else {  // PDCCH on the secondary cell
            n_pucch_i[k++] = row[j % SRSRAN_PUCCH_NOF_AN_CS];
          }
        }
      }
      return k;
    }
    if (cfg->ack_nack_feedback_mode == SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_NORMAL ||
        (cfg->ack_nack_feedback_mode == SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_PUCCH3 && total_ack == ack[0].nof_acks)) {
      n_pucch_i[0] = ack[0].ncce[0] + cfg->N_pucch_1;
      return 1;
    }
    fprintf(stderr, "[srsran_pucch] Unhandled PUCCH format mode %d\n", (int)cfg->ack_nack_feedback_mode);
    return SRSRAN_ERROR;
  }
  if (cfg->format == SRSRAN_PUCCH_FORMAT_3) {
    n_pucch_i[0] = cfg->n3_pucch_an_list[uci_cfg->ack[0].tpc_for_pucch % SRSRAN_PUCCH_SIZE_AN_CS];
    return 1;
  }
  n_pucch_i[0] = cfg->n_pucch_2;
  return 1;
}

// pucch_proc.c:344-437, 589-622: the UE's resource and b(0) b(1) for format 1b with channel selection
// (36.213 Tables 10.1.2.2.1-3 / -4 / -5).  In a TDD cell the reference's resource list comes back with its
// invalid-inputs code (pucch_proc.c:272-285), so this returns 0 there, as the reference does.
uint32_t srsran_pucch_proc_get_npucch(const srsran_cell_t*      cell,
                                      const srsran_pucch_cfg_t* cfg,
                                      const srsran_uci_cfg_t*   uci_cfg,
                                      const srsran_uci_value_t* uci_value,
                                      uint8_t                   b[SRSRAN_UCI_MAX_ACK_BITS])
{
  uint32_t  n[SRSRAN_PUCCH_MAX_ALLOC] = {};
  const int nres                      = srsran_pucch_proc_get_resources(cell, cfg, uci_cfg, uci_value, n);
  memcpy(b, uci_value->ack.ack_value, SRSRAN_UCI_MAX_ACK_BITS);
  if (nres < 1) {
    return 0;
  }
  if (nres == 1) {
    return n[0];
  }
  if (cell->frame_type == SRSRAN_TDD || cfg->ack_nack_feedback_mode != SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_CS) {
    return 0;
  }
  const bool a0 = b[0] == 1, a1 = b[1] == 1, a2 = b[2] == 1, a3 = b[3] == 1;
  uint32_t   r  = 0;
  bool       o0 = false, o1 = false;
  switch (srsran_uci_cfg_total_ack(uci_cfg)) {
    case 1:
      return n[0];
    case 2:
      r  = a1 ? 1 : 0;
      o0 = o1 = a0;
      break;
    case 3:
      r  = (!a0 && !a1) ? 2 : (a2 ? 1 : 0);
      if (!a0 && !a1 && !a2) {
        o0 = o1 = false;
      } else if (a0 != a1) {  // NACK + ACK: (0, 1), ACK + NACK: (1, 0)
        o0 = a0, o1 = a1;
      } else {
        o0 = o1 = true;
      }
      break;
    case 4:
      r = (!a2 && !a3) ? 0 : (a1 && a2) ? 1 : a0 ? 2 : 3;
      if (r == 0) {
        o0 = a0, o1 = a1;
      } else if (r == 1) {
        o0 = a0, o1 = a3;
      } else if (r == 2) {
        o0 = a3 && !a2, o1 = a3 && (a1 != a2);
      } else {
        o0 = a2, o1 = a3 && (a1 != a2);
      }
      break;
    default:
      fprintf(stderr, "[srsran_pucch] Too many (%u) ACK for this CS mode\n", srsran_uci_cfg_total_ack(uci_cfg));
      return 0;
  }
  b[0] = o0 ? 1 : 0;
  b[1] = o1 ? 1 : 0;
  return n[r];
}

int srsran_pucch_cs_get_ack(const srsran_pucch_cfg_t* cfg,
                            const srsran_uci_cfg_t*   uci_cfg,
                            uint32_t                  j,
                            const uint8_t             b[2],
                            srsran_uci_value_t*       uci_value)
{
  if (!cfg || !uci_cfg || !uci_value) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  // 36.213 Tables 10.1.2.2.1-3 / -4 / -5 read backwards: (resource j, b(0), b(1)) -> mask of ACKs
  struct Row {
    uint8_t j, b0, b1, acks;
  };
  static const Row a2[] = {{1, 1, 1, 0x3}, {0, 1, 1, 0x1}, {1, 0, 0, 0x2}};
  static const Row a3[] = {{1, 1, 1, 0x7}, {1, 1, 0, 0x5}, {1, 0, 1, 0x6}, {2, 1, 1, 0x4},
                           {0, 1, 1, 0x3}, {0, 1, 0, 0x1}, {0, 0, 1, 0x2}, {1, 0, 0, 0x0}};
  static const Row a4[] = {{1, 1, 1, 0xF}, {2, 0, 1, 0xD}, {1, 0, 1, 0xE}, {3, 1, 1, 0xC}, {1, 1, 0, 0x7}, {2, 0, 0, 0x5},
                           {1, 0, 0, 0x6}, {3, 1, 0, 0x4}, {2, 1, 1, 0xB}, {2, 1, 0, 0x9}, {3, 0, 1, 0xA}, {3, 0, 0, 0x8},
                           {0, 1, 1, 0x3}, {0, 1, 0, 0x1}, {0, 0, 1, 0x2}, {0, 0, 0, 0x0}};
  memset(uci_value->ack.ack_value, 0, SRSRAN_UCI_MAX_ACK_BITS);
  const uint32_t nof_ack = srsran_uci_cfg_total_ack(uci_cfg);
  const Row*     rows    = nof_ack == 2 ? a2 : nof_ack == 3 ? a3 : a4;
  const uint32_t nrows   = nof_ack == 2 ? 3 : nof_ack == 3 ? 8 : 16;
  if (nof_ack < 2 || nof_ack > 4) {
    fprintf(stderr, "[srsran_pucch] Unexpected number of ACK (%u)\n", nof_ack);
    return SRSRAN_ERROR;
  }
  for (uint32_t r = 0; r < nrows; r++) {
    if (rows[r].j == j && rows[r].b0 == b[0] && rows[r].b1 == b[1]) {
      for (uint32_t a = 0; a < SRSRAN_PUCCH_CS_MAX_ACK; a++) {
        if ((rows[r].acks >> a) & 1u) {
          uci_value->ack.ack_value[a] = 1;
        }
      }
      return SRSRAN_SUCCESS;
    }
  }
  return SRSRAN_ERROR;
}

uint32_t srsran_refsignal_dmrs_N_rs(srsran_pucch_format_t format, srsran_cp_t cp)
{
  if (is_f1(format)) {
    return cp == SRSRAN_CP_NORM ? 3 : 2;
  }
  if (format == SRSRAN_PUCCH_FORMAT_2 || format == SRSRAN_PUCCH_FORMAT_3) {
    return cp == SRSRAN_CP_NORM ? 2 : 1;
  }
  if (format == SRSRAN_PUCCH_FORMAT_2A || format == SRSRAN_PUCCH_FORMAT_2B) {
    return 2;
  }
  fprintf(stderr, "[srsran_refsignal] DMRS Nof RS: Unsupported format %d\n", (int)format);
  return 0;
}

uint32_t srsran_refsignal_dmrs_pucch_symbol(uint32_t m, srsran_pucch_format_t format, srsran_cp_t cp)
{
  // 36.211 Table 5.5.2.2.2-1
  static const uint32_t f1[2][3] = {{2, 3, 4}, {2, 3, 0}}, f2[2][2] = {{1, 5}, {3, 0}};
  const uint32_t        ext      = cp == SRSRAN_CP_NORM ? 0 : 1;
  if (is_f1(format)) {
    return m < (ext ? 2u : 3u) ? f1[ext][m] : 0;
  }
  if (format == SRSRAN_PUCCH_FORMAT_2 || format == SRSRAN_PUCCH_FORMAT_3) {
    return m < (ext ? 1u : 2u) ? f2[ext][m] : 0;
  }
  if (format == SRSRAN_PUCCH_FORMAT_2A || format == SRSRAN_PUCCH_FORMAT_2B) {
    return m < 2 ? f2[0][m] : 0;
  }
  fprintf(stderr, "[srsran_refsignal] DMRS Symbol indexes: Unsupported format %d\n", (int)format);
  return 0;
}

// ---------------- pucch.c:48-132 ----------------
int srsran_pucch_init_enb(srsran_pucch_t* q)
{
  if (!q) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  memset(q, 0, sizeof(*q));
  PucchGpu* g = new PucchGpu();
  q->gpu      = g;
  if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess || !reserve(g, 64) ||
      !g->d_re.reserve(2 * PUCCH_MAX_RE)) {
    srsran_pucch_free(q);
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

void srsran_pucch_free(srsran_pucch_t* q)
{
  if (!q) {
    return;
  }
  PucchGpu* g = (PucchGpu*)q->gpu;
  if (g) {
    if (g->stream) {
      hipStreamSynchronize(g->stream);
      hipStreamDestroy(g->stream);
    }
    delete g;
  }
  memset(q, 0, sizeof(*q));
}

int srsran_pucch_set_cell(srsran_pucch_t* q, srsran_cell_t cell)
{
  if (!q || !cell_valid(cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (cell.id != q->cell.id || q->cell.nof_prb == 0 || cell.cp != q->cell.cp) {
    const CellTables* t = cell_tables(cell);
    memcpy(q->n_cs_cell, t->n_cs_cell, sizeof(q->n_cs_cell));
    memcpy(q->f_gh, t->f_gh, sizeof(q->f_gh));
  }
  q->cell = cell;
  return SRSRAN_SUCCESS;
}

// ---------------- chest_ul.c:462-610 ----------------
int srsran_chest_ul_estimate_pucch(srsran_chest_ul_t*     q,
                                   srsran_ul_sf_cfg_t*    sf,
                                   srsran_pucch_cfg_t*    cfg,
                                   cf_t*                  input,
                                   srsran_chest_ul_res_t* res)
{
  if (!q || !q->gpu || !sf || !cfg || !input || !res || !cell_valid(q->cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (check_estimator(q, cfg) != SRSRAN_SUCCESS) {
    return SRSRAN_ERROR;
  }
  const uint32_t nsym = nsymb_slot(q->cell.cp), ncell = q->cell.nof_prb * SRSRAN_NRE;
  const size_t   sf_re = (size_t)ncell * 2 * nsym;
  if (res->ce && sf_re > res->nof_re) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PucchCand c;
  const int err = build_cand(q->cell, *cell_tables(q->cell), q, sf, cfg, c);
  if (err != SRSRAN_SUCCESS) {
    fprintf(stderr, "[srsran_chest_ul] Error computing N_rs\n");
    return err;
  }
  // scratch: the grid, the estimate grid, the descriptor and its result
  const size_t grid_bytes = sf_re * sizeof(float2), desc_off = 2 * grid_bytes;
  const size_t out_off    = desc_off + ((sizeof(PucchCand) + 15) & ~(size_t)15);
  uint8_t*     d          = (uint8_t*)chest_ul_scratch(q, out_off + sizeof(PucchCandOut));
  hipStream_t  st         = chest_ul_stream(q);
  if (!d) {
    return SRSRAN_ERROR;
  }
  float2* d_ce = (float2*)(d + grid_bytes);
  c.grid       = (const float2*)d;
  c.ce         = res->ce ? d_ce : nullptr;
  PucchCandOut o;
  if (hipMemcpyAsync(d, input, grid_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d + desc_off, &c, sizeof(c), hipMemcpyHostToDevice, st) != hipSuccess ||
      pucch_launch((const PucchCand*)(d + desc_off), (PucchCandOut*)(d + out_off), 1, st) != hipSuccess ||
      hipMemcpyAsync(&o, d + out_off, sizeof(o), hipMemcpyDeviceToHost, st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  if (res->ce) {  // the written PRB of each slot back to the host estimate
    for (uint32_t s = 0; s < 2; s++) {
      const size_t o0 = (size_t)s * nsym * ncell + c.n_prb[s] * SRSRAN_NRE;
      if (hipMemcpy2DAsync(res->ce + o0, ncell * sizeof(float2), d_ce + o0, ncell * sizeof(float2),
                           SRSRAN_NRE * sizeof(float2), nsym, hipMemcpyDeviceToHost, st) != hipSuccess) {
        return SRSRAN_ERROR;
      }
    }
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  if (cfg->format == SRSRAN_PUCCH_FORMAT_2A || cfg->format == SRSRAN_PUCCH_FORMAT_2B) {
    cfg->pucch2_drs_bits[0] = o.drs_bits[0];
    cfg->pucch2_drs_bits[1] = o.drs_bits[1];
  }
  res->epre      = o.epre;
  res->epre_dBfs = to_dB(o.epre);
  res->rsrp      = o.rsrp;
  res->rsrp_dBfs = to_dB(o.rsrp);
  if (cfg->meas_ta_en) {
    res->ta_us = o.ta_us;
  }
  if (res->ce) {
    const ChestScalars s     = chest_scalars(o);
    res->noise_estimate      = o.noise;
    res->noise_estimate_dbFs = s.noise_dbFs;
    res->snr                 = isnormal(o.noise) ? o.epre / o.noise : NAN;
    res->snr_db              = s.snr_db;
    chest_ul_res_host_changed(res);
  }
  return SRSRAN_SUCCESS;
}

// ---------------- pucch.c:797-872 ----------------
int srsran_pucch_decode(srsran_pucch_t*        q,
                        srsran_ul_sf_cfg_t*    sf,
                        srsran_pucch_cfg_t*    cfg,
                        srsran_chest_ul_res_t* channel,
                        cf_t*                  sf_symbols,
                        srsran_pucch_res_t*    data)
{
  if (!q || !q->gpu || !sf || !cfg || !channel || !channel->ce || !sf_symbols || !data || !cell_valid(q->cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PucchGpu* g = (PucchGpu*)q->gpu;
  PucchCand c;
  if (build_cand(q->cell, *cell_tables(q->cell), nullptr, sf, cfg, c) != SRSRAN_SUCCESS) {
    fprintf(stderr, "[srsran_pucch] Error getting PUCCH symbols\n");
    return SRSRAN_ERROR;
  }
  // pucch_get of the symbols and of the estimates (pucch.c:321-362)
  const uint32_t nre = (c.n_sf[0] + c.n_sf[1]) * SRSRAN_NRE, ncell = c.ncell_re;
  cf_t           re[2 * PUCCH_MAX_RE];
  for (uint32_t s = 0, k = 0; s < 2; s++) {
    for (uint32_t i = 0; i < c.n_sf[s]; i++, k += SRSRAN_NRE) {
      const size_t o0 = (size_t)(s * c.nsym_slot + c.data_sym[i]) * ncell + c.n_prb[s] * SRSRAN_NRE;
      memcpy(&re[k], &sf_symbols[o0], SRSRAN_NRE * sizeof(cf_t));
      memcpy(&re[nre + k], &channel->ce[o0], SRSRAN_NRE * sizeof(cf_t));
    }
  }
  c.compact   = 1;
  c.do_decode = 1;
  c.grid      = g->d_re;
  c.ce_in     = g->d_re + nre;
  c.noise_in  = channel->noise_estimate;
  g->h_cand[0] = c;
  if (hipMemcpyAsync(g->d_re, re, 2 * nre * sizeof(float2), hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      hipMemcpyAsync(g->d_cand, g->h_cand, sizeof(PucchCand), hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      pucch_launch(g->d_cand, g->d_out, 1, g->stream) != hipSuccess ||
      hipMemcpyAsync(g->h_out, g->d_out, sizeof(PucchCandOut), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  apply_decode(cfg, g->h_out[0], cfg->pucch2_drs_bits, data);
  return SRSRAN_SUCCESS;
}

// ---------------- added: enb_ul.c:156-273 for many UEs, one launch ----------------
int srsran_pucch_gpu_get_batch(srsran_pucch_t*              q,
                               uint32_t                     nof_ue,
                               const srsran_pucch_gpu_ue_t* ues,
                               srsran_pucch_res_t*          res)
{
  if (!q || !q->gpu || (nof_ue && (!ues || !res))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PucchGpu* g = (PucchGpu*)q->gpu;
  // plan every entry on copies of the configurations: nothing is written or launched on an error
  std::vector<EntryPlan> plan(nof_ue);
  std::vector<PucchCand> cands;
  cands.reserve((size_t)nof_ue * 2);
  for (uint32_t e = 0; e < nof_ue; e++) {
    const srsran_pucch_gpu_ue_t& ue = ues[e];
    if (!ue.chest || !ue.chest->gpu || !ue.sf || !ue.cfg || !ue.d_sf_symbols || !cell_valid(ue.chest->cell)) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    const srsran_cell_t& cell = ue.chest->cell;
    if (!srsran_pucch_cfg_isvalid(ue.cfg, cell.nof_prb)) {
      fprintf(stderr, "[srsran_pucch] Invalid PUCCH configuration\n");
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (check_estimator(ue.chest, ue.cfg) != SRSRAN_SUCCESS) {
      return SRSRAN_ERROR;
    }
    const CellTables*  t   = cell_tables(cell);
    srsran_pucch_cfg_t cfg = *ue.cfg;
    EntryPlan&         p   = plan[e];
    p.first                = (uint32_t)cands.size();
    p.cqi_dropped = !cfg.simul_cqi_ack && srsran_uci_cfg_total_ack(&cfg.uci_cfg) > 0 && cfg.uci_cfg.cqi.data_enable;
    if (p.cqi_dropped) {
      cfg.uci_cfg.cqi.data_enable = false;
    }
    p.npass = cfg.uci_cfg.is_scheduling_request_tti && srsran_uci_cfg_total_ack(&cfg.uci_cfg) ? 2 : 1;
    for (uint32_t pass = 0; pass < p.npass; pass++) {
      if (pass == 1) {
        cfg.uci_cfg.is_scheduling_request_tti = false;
      }
      if (plan_pass(cell, &cfg, p.pass[pass]) != SRSRAN_SUCCESS) {
        return SRSRAN_ERROR;
      }
      for (int i = 0; i < p.pass[pass].nres; i++) {
        cfg.n_pucch = (uint16_t)p.pass[pass].n_pucch[i];
        PucchCand c;
        if (build_cand(cell, *t, ue.chest, ue.sf, &cfg, c) != SRSRAN_SUCCESS) {
          return SRSRAN_ERROR;
        }
        c.grid      = (const float2*)ue.d_sf_symbols;
        c.do_decode = 1;
        cands.push_back(c);
      }
    }
  }
  const uint32_t ncand = (uint32_t)cands.size();
  if (ncand == 0) {
    return SRSRAN_SUCCESS;
  }
  if (!reserve(g, ncand)) {
    return SRSRAN_ERROR;
  }
  memcpy(g->h_cand, cands.data(), (size_t)ncand * sizeof(PucchCand));
  if (hipMemcpyAsync(g->d_cand, g->h_cand, (size_t)ncand * sizeof(PucchCand), hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      pucch_launch(g->d_cand, g->d_out, ncand, g->stream) != hipSuccess ||
      hipMemcpyAsync(g->h_out, g->d_out, (size_t)ncand * sizeof(PucchCandOut), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  // the pick of each pass, the override rule and the write-backs (enb_ul.c:233-273)
  for (uint32_t e = 0; e < nof_ue; e++) {
    srsran_pucch_cfg_t* cfg = ues[e].cfg;
    const EntryPlan&    p   = plan[e];
    if (p.cqi_dropped) {
      cfg->uci_cfg.cqi.data_enable = false;
    }
    finish_pass(cfg, p.pass[0], g->h_out + p.first, &res[e]);
    if (p.npass == 2) {
      cfg->uci_cfg.is_scheduling_request_tti = false;
      srsran_pucch_res_t no_sr;
      memset(&no_sr, 0, sizeof(no_sr));
      finish_pass(cfg, p.pass[1], g->h_out + p.first + p.pass[0].nres, &no_sr);
      if (no_sr.detected && (!res[e].detected || no_sr.correlation > res[e].correlation)) {
        res[e] = no_sr;
      } else {
        cfg->uci_cfg.is_scheduling_request_tti = true;
      }
    }
  }
  return SRSRAN_SUCCESS;
}

}  // extern "C"

// ---------------- transmit (UE side) ----------------
namespace {

// (20, A) basis sequences, 36.212 Table 5.2.3.3-1: bit n of word i is M_{i,n}
const uint16_t kPucchBasis[SRSRAN_UCI_CQI_CODED_PUCCH_B] = {0x0C03, 0x0E07, 0x1F49, 0x1D0D, 0x1C8F, 0x1DD3, 0x1F55,
                                                            0x1D99, 0x1E9B, 0x1E5D, 0x1EE5, 0x1D67, 0x1FA9, 0x1EAB,
                                                            0x14B1, 0x16F3, 0x1A77, 0x1939, 0x00FB, 0x0061};
// (32, O) basis sequences, 36.212 Table 5.2.2.6.4-1 (as uci_host.cpp's kBlockBasisHost)
const uint16_t kBlockBasis[32] = {0x403, 0x607, 0x749, 0x50D, 0x48F, 0x5D3, 0x755, 0x599, 0x69B, 0x65D, 0x6E5,
                                  0x567, 0x7A9, 0x6AB, 0x4B1, 0x6F3, 0x277, 0x139, 0x0FB, 0x061, 0x445, 0x60B,
                                  0x591, 0x717, 0x3DF, 0x4E3, 0x32D, 0x3AF, 0x175, 0x1FD, 0x7FF, 0x001};

// srsran_uci_encode_cqi_pucch (uci.c:92-106): bit i of the result is b(i)
uint64_t encode_cqi_pucch(const uint8_t* data, uint32_t len)
{
  uint32_t w = 0;
  for (uint32_t n = 0; n < len && n < SRSRAN_UCI_MAX_CQI_LEN_PUCCH; n++) {
    w |= (uint32_t)(data[n] & 1u) << n;
  }
  uint64_t b = 0;
  for (uint32_t i = 0; i < SRSRAN_UCI_CQI_CODED_PUCCH_B; i++) {
    b |= (uint64_t)(__builtin_popcount(w & kPucchBasis[i]) & 1) << i;
  }
  return b;
}

// encode_bits (pucch.c:583-623): the bits the kernel modulates, bit i of *bits is b(i); writes pucch2_drs_bits
int tx_encode_bits(srsran_pucch_cfg_t* cfg, const srsran_uci_value_t* v, uint64_t* bits)
{
  const srsran_pucch_format_t f       = cfg->format;
  const uint32_t              nof_ack = std::min<uint32_t>(srsran_uci_cfg_total_ack(&cfg->uci_cfg), SRSRAN_UCI_MAX_ACK_BITS);
  *bits                               = 0;
  if (is_f1(f)) {
    for (uint32_t a = 0; a < nof_ack && a < 2; a++) {
      *bits |= (uint64_t)(v->ack.ack_value[a] ? 1u : 0u) << a;  // any non-zero value modulates as 1
    }
  } else if (is_f2(f)) {
    if (cfg->uci_cfg.cqi.ri_len) {  // RI goes alone
      const uint8_t temp[2] = {v->ri, 0};
      if (cfg->uci_cfg.cqi.ri_len > SRSRAN_UCI_MAX_CQI_LEN_PUCCH) {
        return SRSRAN_ERROR;
      }
      *bits = encode_cqi_pucch(temp, std::min<uint32_t>(cfg->uci_cfg.cqi.ri_len, 2));
    } else {
      uint8_t   buff[SRSRAN_CQI_MAX_BITS] = {};
      const int len = srsran_cqi_value_pack(&cfg->uci_cfg.cqi, const_cast<srsran_cqi_value_t*>(&v->cqi), buff);
      if (len < 0 || len > SRSRAN_UCI_MAX_CQI_LEN_PUCCH) {
        fprintf(stderr, "[srsran_pucch] Error encoding CQI\n");
        return SRSRAN_ERROR;
      }
      *bits = encode_cqi_pucch(buff, (uint32_t)len);
    }
    if (f != SRSRAN_PUCCH_FORMAT_2) {
      cfg->pucch2_drs_bits[0] = v->ack.ack_value[0];
      cfg->pucch2_drs_bits[1] = v->ack.ack_value[1];  // ignored in format 2a
    }
  } else if (f == SRSRAN_PUCCH_FORMAT_3) {
    uint32_t w = 0, k = 0;
    for (; k < nof_ack; k++) {
      w |= (uint32_t)(v->ack.ack_value[k] == 1 ? 1u : 0u) << k;
    }
    if (cfg->uci_cfg.is_scheduling_request_tti) {
      w |= (uint32_t)(v->scheduling_request ? 1u : 0u) << k;
      k++;
    }
    w &= 0x7FFu;  // srsran_block_encode takes the first 11 bits
    for (uint32_t i = 0; i < SRSRAN_PUCCH3_NOF_BITS; i++) {
      *bits |= (uint64_t)(__builtin_popcount(w & kBlockBasis[i % 32]) & 1) << i;
    }
  }
  return SRSRAN_SUCCESS;
}

// the cover arguments as the reference's tables hold them (pucch.c:211-217, refsignal_ul.c:46-53), from the phase in
// units of pi / 12
float cover_arg(uint8_t ph)
{
  switch (ph) {
    case 8:
      return (float)(2 * M_PI / 3);
    case 12:
      return (float)M_PI;
    case 16:
      return (float)(4 * M_PI / 3);
    default:
      return 0.0f;
  }
}

// The transmit descriptor of (cell, subframe, cfg->format, cfg->n_pucch): build_cand's fields plus the cover
// arguments, the bits and d(10).  Pointers are left null.
int build_tx(const srsran_cell_t& cell, const srsran_ul_sf_cfg_t* sf, srsran_pucch_cfg_t* cfg, uint64_t bits, PucchTxUe& d)
{
  const CellTables& t = *cell_tables(cell);
  PucchCand         c;
  const int         err = build_cand(cell, t, nullptr, sf, cfg, c);
  if (err != SRSRAN_SUCCESS) {
    return err;
  }
  memset(&d, 0, sizeof(d));
  d.ncell_re  = c.ncell_re;
  d.nsym_slot = c.nsym_slot;
  d.format    = c.format;
  d.n_rs      = c.n_rs;
  memcpy(d.phi, c.phi, sizeof(d.phi));
  memcpy(d.rs_sym, c.rs_sym, sizeof(d.rs_sym));
  memcpy(d.data_sym, c.data_sym, sizeof(d.data_sym));
  memcpy(d.rs_ncs, c.rs_ncs, sizeof(d.rs_ncs));
  memcpy(d.data_ncs, c.data_ncs, sizeof(d.data_ncs));
  memcpy(d.f3_noc, c.f3_noc, sizeof(d.f3_noc));
  for (uint32_t s = 0; s < 2; s++) {
    const uint32_t ns = 2 * (sf->tti % 10) + s;
    d.n_prb[s]        = c.n_prb[s];
    d.n_sf[s]         = c.n_sf[s];
    for (uint32_t m = 0; m < c.n_rs; m++) {
      d.rs_warg[s][m] = cover_arg(c.rs_ph[s][m]);
    }
    for (uint32_t i = 0; i < c.n_sf[s] && is_f1(cfg->format); i++) {
      // pucch.c:419-432: w_n_oc(i) of the DMRS n_oc, plus S(ns), both single precision
      uint32_t n_oc = 0, n_prime = 0;
      ncs_format1(t.n_cs_cell, cfg, cell.cp, true, ns, c.data_sym[i], &n_oc, &n_prime);
      d.data_warg[s][i] = cover_arg(kDataW[c.n_sf[s] == 3 ? 1 : 0][n_oc % 3][i]) + (n_prime % 2 ? (float)(M_PI / 2) : 0.0f);
    }
  }
  d.bits   = bits;
  d.scr    = c.scr;
  d.drs[0] = cfg->pucch2_drs_bits[0] ? 1 : 0;
  d.drs[1] = cfg->pucch2_drs_bits[1] ? 1 : 0;
  return SRSRAN_SUCCESS;
}

}  // namespace

namespace srsran_amd {

// srsran_pucch_encode up to the kernel, for the UE uplink (ue_ul_api.cpp): the descriptor of cfg->format /
// cfg->n_pucch carrying *uci, pointers left null.  Writes cfg->pucch2_drs_bits for 2a / 2b.
int pucch_tx_prepare(const srsran_cell_t&      cell,
                     const srsran_ul_sf_cfg_t* sf,
                     srsran_pucch_cfg_t*       cfg,
                     const srsran_uci_value_t* uci,
                     PucchTxUe*                d)
{
  uint64_t bits = 0;
  if (tx_encode_bits(cfg, uci, &bits) != SRSRAN_SUCCESS) {
    return SRSRAN_ERROR;
  }
  return build_tx(cell, sf, cfg, bits, *d) == SRSRAN_SUCCESS ? SRSRAN_SUCCESS : SRSRAN_ERROR;
}

}  // namespace srsran_amd

extern "C" {

// pucch.c:83
int srsran_pucch_init_ue(srsran_pucch_t* q)
{
  const int ret = srsran_pucch_init_enb(q);
  if (ret == SRSRAN_SUCCESS) {
    q->is_ue = true;
  }
  return ret;
}

// pucch.c:768-794
int srsran_pucch_encode(srsran_pucch_t*     q,
                        srsran_ul_sf_cfg_t* sf,
                        srsran_pucch_cfg_t* cfg,
                        srsran_uci_value_t* uci_data,
                        cf_t*               sf_symbols)
{
  if (!q || !q->gpu || !sf || !cfg || !uci_data || !sf_symbols || !cell_valid(q->cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PucchGpu* g = (PucchGpu*)q->gpu;
  PucchTxUe d;
  if (pucch_tx_prepare(q->cell, sf, cfg, uci_data, &d) != SRSRAN_SUCCESS) {
    fprintf(stderr, "[srsran_pucch] Error encoding PUCCH (format %s)\n", srsran_pucch_format_text(cfg->format));
    return SRSRAN_ERROR;
  }
  if (!g->d_tx.reserve(1)) {
    return SRSRAN_ERROR;
  }
  const uint32_t nre = (d.n_sf[0] + d.n_sf[1]) * SRSRAN_NRE;
  cf_t           z[PUCCH_MAX_RE];
  d.z_out = g->d_re;
  if (hipMemcpyAsync(g->d_tx, &d, sizeof(d), hipMemcpyHostToDevice, g->stream) != hipSuccess ||
      pucch_tx_launch(g->d_tx, 1, g->stream) != hipSuccess ||
      hipMemcpyAsync(z, g->d_re, nre * sizeof(float2), hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
      hipStreamSynchronize(g->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  // pucch_put (pucch.c:321-367): only the data REs are written
  for (uint32_t s = 0; s < 2; s++) {
    for (uint32_t i = 0; i < d.n_sf[s]; i++) {
      memcpy(&sf_symbols[(size_t)(s * d.nsym_slot + d.data_sym[i]) * d.ncell_re + d.n_prb[s] * SRSRAN_NRE],
             &z[(s * d.n_sf[0] + i) * SRSRAN_NRE], SRSRAN_NRE * sizeof(cf_t));
    }
  }
  return SRSRAN_SUCCESS;
}

// refsignal_ul.c:432-512, r_pucch[(slot N_rs + m) 12 + n].  There is no device object to run on here: the values
// are those of the kernel's per-RE function, evaluated on the host.
int srsran_refsignal_dmrs_pucch_gen_cell(const srsran_cell_t* cell,
                                         srsran_ul_sf_cfg_t*  sf,
                                         srsran_pucch_cfg_t*  cfg,
                                         cf_t*                r_pucch)
{
  if (!cell || !sf || !cfg || !r_pucch || !cell_valid(*cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  PucchTxUe d;
  if (build_tx(*cell, sf, cfg, 0, d) != SRSRAN_SUCCESS) {
    return SRSRAN_ERROR;
  }
  for (uint32_t s = 0; s < 2; s++) {
    for (uint32_t m = 0; m < d.n_rs; m++) {
      for (uint32_t n = 0; n < SRSRAN_NRE; n++) {
        const float2 v = pucch_tx_re(d, s, true, m, n);
        cf_t*        o = &r_pucch[(s * d.n_rs + m) * SRSRAN_NRE + n];
        memcpy(o, &v, sizeof(v));
      }
    }
  }
  return SRSRAN_SUCCESS;
}

// refsignal_ul.c:514-552
int srsran_refsignal_dmrs_pucch_put_cell(const srsran_cell_t* cell, srsran_pucch_cfg_t* cfg, cf_t* r_pucch, cf_t* output)
{
  if (!cell || !cfg || !r_pucch || !output || !cell_valid(*cell)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  const uint32_t N_rs = srsran_refsignal_dmrs_N_rs(cfg->format, cell->cp), nsym = nsymb_slot(cell->cp);
  if (!N_rs || cfg->delta_pucch_shift == 0) {
    return SRSRAN_ERROR;
  }
  for (uint32_t s = 0; s < 2; s++) {
    const uint32_t n_prb = srsran_pucch_n_prb(cell, cfg, s);
    if (n_prb >= cell->nof_prb) {
      fprintf(stderr, "[srsran_refsignal] Invalid PUCCH n_prb=%u\n", n_prb);
      return SRSRAN_ERROR;
    }
    for (uint32_t i = 0; i < N_rs; i++) {
      const uint32_t l = srsran_refsignal_dmrs_pucch_symbol(i, cfg->format, cell->cp);
      memcpy(&output[(size_t)(l + s * nsym) * cell->nof_prb * SRSRAN_NRE + n_prb * SRSRAN_NRE],
             &r_pucch[(s * N_rs + i) * SRSRAN_NRE], SRSRAN_NRE * sizeof(cf_t));
    }
  }
  return SRSRAN_SUCCESS;
}

}  // extern "C"
