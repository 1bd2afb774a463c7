// srsran_4g_amd/csrc/ulsch_api.cpp -- the UL-SCH with UCI on the srsran_sch_t object (include/srsran_sch.h,
// sch_internal.h):
//   receive   srsran_ulsch_decode (sch.c:994-1193), single and batched: ACK / RI decode, de-interleaver, CQI decode
//             on the GPU (uci_kernel.hip, sch_kernel.hip), then decode_tb through the DL-SCH path of sch_api.cpp
//   transmit  srsran_ulsch_encode (sch.c:1195-1337): the host plan and UCI channel coding (uci_host.cpp), then the
//             TB CRC and code block launches of enc_kernel.hip and the multiplexer of pusch_tx_kernel.hip
// The receiver tests cfg->grant.tb.tbs == 0 for "no TB" and takes up to four RI bits; the transmitter tests the
// segmentation's s.tbs == 0 and takes up to two, as the reference's two functions do: the plans stay apart.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/srsran_sch.h"
#include "dev_buf.h"
#include "enc_kernel.h"
#include "pdsch_internal.h"
#include "sch_internal.h"
#include "sch_kernel.h"
#include "sch_units.h"
#include "uci_host.h"
#include "uci_kernel.h"

using namespace srsran_amd;

static_assert(UCI_MAX_CQI_BITS == SRSRAN_CQI_MAX_BITS, "the kernels' CQI buffer is the public header's");
static_assert(UCI_BIT_0 == TX_BIT_0 && UCI_BIT_1 == TX_BIT_1 && UCI_BIT_REPETITION == TX_BIT_REPETITION &&
                  UCI_BIT_PLACEHOLDER == TX_BIT_PLACEHOLDER,
              "uci_host.cpp writes the bit types the multiplexing kernel reads");

namespace {

// ---------------- UL-SCH receive with UCI (sch.c:994-1193) ----------------
// The host part shared by srsran_ulsch_decode and the batched path: segmentation, sizes, Q'_ACK / Q'_RI.
struct UlsPlan {
  srsran_cbsegm_t s;
  uint32_t        nb, Qm, nsymb, H, rows, nack, ack_Qp, ri_Qp;
  bool            uci, hl_ri, need_c;
};

int ulsch_plan(srsran_pusch_cfg_t* cfg, UlsPlan* p)
{
  srsran_cbsegm_t& s = p->s;
  if (srsran_cbsegm(&s, (uint32_t)cfg->grant.tb.tbs)) {
    fprintf(stderr, "[srsran_sch] Error computing segmentation for TBS=%d\n", cfg->grant.tb.tbs);
    return SRSRAN_ERROR;
  }
  p->nb       = cfg->grant.tb.nof_bits;
  p->Qm       = srsran_mod_bits_x_symbol(cfg->grant.tb.mod);
  cfg->K_segm = s.C1 * s.K1 + s.C2 * s.K2;
  if (p->Qm == 0) {
    fprintf(stderr, "[srsran_sch] Invalid modulation\n");
    return SRSRAN_ERROR;
  }
  p->nsymb = cfg->grant.nof_symb;
  if (p->nsymb == 0 || p->nsymb > 14 || p->nb % p->Qm || p->Qm > 8) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  p->H                  = p->nb / p->Qm;
  p->rows               = p->H / p->nsymb;
  srsran_cqi_cfg_t& cq  = cfg->uci_cfg.cqi;
  p->nack               = srsran_uci_cfg_total_ack(&cfg->uci_cfg);
  p->uci                = p->nack > 0 || cq.ri_len > 0 || cq.data_enable;
  // ---- uci_decode_ri_ack, host part (sch.c:1023-1120): Q'_ACK, Q'_RI ----
  p->hl_ri = cq.data_enable && cq.type == SRSRAN_CQI_TYPE_SUBBAND_HL && cq.ri_len;
  if (p->hl_ri) {
    cq.rank_is_not_one = false;  // RI = 1 assumed for the RI / ACK sizes (36.212 5.2.4.1)
  }
  const uint32_t cqi_len0 = (uint32_t)srsran_cqi_size(&cq);
  const bool     no_tb    = cfg->grant.tb.tbs == 0;
  p->ack_Qp = p->ri_Qp = 0;
  if (p->nack > 0) {
    if (p->nack > SRSRAN_UCI_MAX_ACK_BITS) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    p->ack_Qp = qprime_ri_ack_cfg(cfg, no_tb, p->nsymb, p->nack, cqi_len0, beta_harq(cfg->uci_offset.I_offset_ack));
  }
  if (cq.ri_len > 0) {
    if (cq.ri_len > 4) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    p->ri_Qp = qprime_ri_ack_cfg(cfg, no_tb, p->nsymb, cq.ri_len, cqi_len0, beta_ri(cfg->uci_offset.I_offset_ri));
  }
  // the ACK / RI rows are counted up from the bottom of the interleaver: positions past its top
  // (uci.c:378-386 "Error interleaving") are refused
  if (p->ack_Qp > 4 * p->rows || p->ri_Qp > 4 * p->rows || p->ri_Qp > p->H) {
    fprintf(stderr, "[srsran_sch] UCI does not fit the PUSCH interleaver (Q'_ACK=%u Q'_RI=%u rows=%u)\n", p->ack_Qp,
            p->ri_Qp, p->rows);
    return SRSRAN_ERROR;
  }
  p->need_c = (p->nack == 1 && p->ack_Qp > 0) || (cq.ri_len == 1 && p->ri_Qp > 0);
  return SRSRAN_SUCCESS;
}

// The de-interleaver descriptor: it skips the RI cells, column set[c] holding the RI indices
// q = 3c mod 4 (mod 4)
UlDeint ulsch_deint_desc(int16_t* d_q, int16_t* d_g, const UlsPlan& p)
{
  UlDeint d = {d_q, d_g, p.rows, p.nsymb, p.Qm, {}, -1};
  if (p.ri_Qp > 0) {
    const uint8_t* set  = uci_ri_cols(p.nsymb);
    int64_t        last = -1;  // the largest RI position in q order
    for (uint32_t c = 0; c < 4; c++) {
      const uint32_t m = (3 * c) % 4, n = p.ri_Qp > m ? (p.ri_Qp - m + 3) / 4 : 0;
      d.ri_rows[set[c]] = (uint16_t)n;
      if (n > 0) {
        last = std::max<int64_t>(last, (int64_t)(p.rows - 1) * p.Qm + (int64_t)set[c] * p.rows * p.Qm + p.Qm - 1);
      }
    }
    uint32_t first = 0;  // the first non-RI column of row 0 holds g[0] in its own right
    while (first < p.nsymb && d.ri_rows[first] >= p.rows) {
      first++;
    }
    d.g0_src = (int32_t)std::max<int64_t>(last, (int64_t)first * p.rows * p.Qm);
  }
  return d;
}

// CQI (sch.c:1160-1183): its size may depend on the RI just decoded (ri: the decoded RI, or -1 when
// not needed)
int ulsch_cqi_plan(srsran_pusch_cfg_t* cfg, const UlsPlan& p, int ri, uint32_t* cqi_len, uint32_t* cqi_Qp)
{
  srsran_cqi_cfg_t& cq = cfg->uci_cfg.cqi;
  *cqi_len = *cqi_Qp = 0;
  if (!cq.data_enable) {
    if (p.hl_ri) {
      cq.rank_is_not_one = false;
    }
    return SRSRAN_SUCCESS;
  }
  if (p.hl_ri) {
    cq.rank_is_not_one = ri > 0;
  }
  const int len = srsran_cqi_size(&cq);
  if (len <= 0 || len > (int)UCI_MAX_CQI_BITS) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  *cqi_len = (uint32_t)len;
  *cqi_Qp  = qprime_cqi(cfg->K_segm, cfg->grant.L_prb, p.nsymb, (uint32_t)len, beta_cqi(cfg->uci_offset.I_offset_cqi),
                        p.ri_Qp);
  return (uint64_t)*cqi_Qp + p.ri_Qp > p.H ? SRSRAN_ERROR : SRSRAN_SUCCESS;
}

// The decoded UCI into the caller's srsran_uci_value_t (sch.c:1084-1117, uci.c)
void ulsch_uci_out(srsran_pusch_cfg_t* cfg, const UlsPlan& p, const UciOut& o, srsran_uci_value_t* uci)
{
  srsran_cqi_cfg_t& cq = cfg->uci_cfg.cqi;
  if (p.nack > 0) {
    memcpy(uci->ack.ack_value, o.ack, std::min<uint32_t>(p.nack, SRSRAN_UCI_MAX_ACK_BITS));
    uci->ack.valid = o.ack_valid != 0;
  }
  if (cq.ri_len > 0) {
    uci->ri = o.ri[0];
  }
  if (cq.data_enable) {
    uci->cqi.data_crc = o.cqi_crc != 0;
    srsran_cqi_value_unpack(&cq, const_cast<uint8_t*>(o.cqi), &uci->cqi);
  }
  if (p.hl_ri) {
    cq.rank_is_not_one = uci->ri > 0;  // sch.c:1112-1117
  }
}

// One device scratch block per call: the UCI / de-interleaver descriptors, the UCI results and
// the unpacked scrambling sequence.
struct UlsUciScratch {
  UciDesc uci;
  UlDeint deint;
  UciOut  out;
};

// srsran_ulsch_decode's body.  The LLRs come from the host (h_q) or are already on the device
// (d_q_ext, zeroed in place at the ACK positions); the scrambling sequence likewise (h_c / d_c_ext).
// q_out / g_bits (host, optional) receive q after the ACK zeroing and the de-interleaved LLRs.
int ulsch_decode_impl(srsran_sch_t*       q,
                      srsran_pusch_cfg_t* cfg,
                      const int16_t*      h_q,
                      int16_t*            d_q_ext,
                      int16_t*            q_out,
                      int16_t*            g_bits,
                      const uint8_t*      h_c,
                      const uint8_t*      d_c_ext,
                      uint8_t*            data,
                      srsran_uci_value_t* uci_data)
{
  if (!q || !q->gpu || !cfg || (!h_q && !d_q_ext)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (q->llr_is_8bit) {
    // srsENB's experimental pusch_8bit_decoder (cc_worker.cc:155-157): pusch.c:419-440 writes int8 LLRs into its
    // int16 q buffer and hands it to srsran_ulsch_decode, whose uci_decode_ri_ack / ulsch_deinterleave read it as
    // int16 (sch.c:1145-1161: pairs of int8 LLRs taken as one, nof_bits of them, past the int8 data) -- the
    // reference's own 8-bit UL-SCH cannot decode, so there is no behaviour to reproduce; refused
    fprintf(stderr, "[srsran_sch] 8-bit UL-SCH LLRs are not provided (the reference's 8-bit PUSCH path passes int8 "
                    "LLRs through int16 interfaces)\n");
    return SRSRAN_ERROR;
  }
  UlsPlan   p;
  const int prc = ulsch_plan(cfg, &p);
  if (prc != SRSRAN_SUCCESS) {
    return prc;
  }
  const uint32_t nb = p.nb, Qm = p.Qm, H = p.H;
  if ((p.uci && !uci_data) || (p.need_c && !h_c && !d_c_ext)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }

  SchCtx* x = (SchCtx*)q->gpu;
  if (!x->d_ul.reserve(2 * (size_t)nb)) {
    return SRSRAN_ERROR;
  }
  int16_t* d_q = d_q_ext ? d_q_ext : x->d_ul;
  int16_t* d_g = x->d_ul + nb;
  // the reference leaves the de-interleaved LLRs in g_bits (positions it does not write untouched)
  if ((g_bits && hipMemcpyAsync(d_g, g_bits, (size_t)nb * 2, hipMemcpyHostToDevice, x->stream) != hipSuccess) ||
      (h_q && hipMemcpyAsync(d_q, h_q, (size_t)nb * 2, hipMemcpyHostToDevice, x->stream) != hipSuccess)) {
    return SRSRAN_ERROR;
  }
  if (!p.uci) {
    if (ul_deint_launch(d_q, d_g, Qm, H, p.nsymb, x->stream) != hipSuccess ||
        (g_bits && hipMemcpyAsync(g_bits, d_g, (size_t)nb * 2, hipMemcpyDeviceToHost, x->stream) != hipSuccess) ||
        (q_out && hipMemcpyAsync(q_out, d_q, (size_t)nb * 2, hipMemcpyDeviceToHost, x->stream) != hipSuccess) ||
        hipStreamSynchronize(x->stream) != hipSuccess) {
      return SRSRAN_ERROR;
    }
    if (p.s.tbs == 0) {
      return SRSRAN_SUCCESS;
    }
    srsran_pdsch_cfg_t pc;
    memset(&pc, 0, sizeof(pc));
    pc.grant.nof_tb       = 1;
    pc.grant.tb[0]        = cfg->grant.tb;
    pc.softbuffers.rx[0]  = cfg->softbuffers.rx;
    pc.max_nof_iterations = cfg->max_nof_iterations;
    return dlsch_decode_sync(q, &pc, nullptr, d_g, data, 0, 1);
  }

  // ---- device scratch: descriptors, results, sequence ----
  const bool   up_c = p.need_c && !d_c_ext;
  const size_t scr  = align16(sizeof(UlsUciScratch)) + (up_c ? (size_t)nb : 0);
  if (!x->d_uci.reserve(scr)) {
    return SRSRAN_ERROR;
  }
  UlsUciScratch* d_s = (UlsUciScratch*)x->d_uci.get();
  const uint8_t* d_c = up_c ? x->d_uci + align16(sizeof(UlsUciScratch)) : d_c_ext;
  srsran_cqi_cfg_t& cq = cfg->uci_cfg.cqi;
  UlsUciScratch  h;
  memset(&h, 0, sizeof(h));
  h.uci   = {d_q, p.need_c ? d_c : nullptr, d_g, &d_s->out, Qm, p.rows, p.nsymb, p.nack, p.ack_Qp, cq.ri_len, p.ri_Qp, 0, 0};
  h.deint = ulsch_deint_desc(d_q, d_g, p);
  if (hipMemcpyAsync(d_s, &h, sizeof(h), hipMemcpyHostToDevice, x->stream) != hipSuccess ||
      (up_c && hipMemcpyAsync((void*)d_c, h_c, nb, hipMemcpyHostToDevice, x->stream) != hipSuccess) ||
      uci_ack_ri_launch(&d_s->uci, 1, x->stream) != hipSuccess ||
      ul_deint_batch_launch(&d_s->deint, 1, p.rows, x->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }

  // ---- CQI (sch.c:1160-1183): its size may depend on the RI just decoded ----
  uint32_t cqi_len = 0, cqi_Qp = 0;
  if (cq.data_enable && p.hl_ri &&
      (hipMemcpyAsync(&h.out, &d_s->out, sizeof(UciOut), hipMemcpyDeviceToHost, x->stream) != hipSuccess ||
       hipStreamSynchronize(x->stream) != hipSuccess)) {
    return SRSRAN_ERROR;
  }
  const int crc = ulsch_cqi_plan(cfg, p, h.out.ri[0], &cqi_len, &cqi_Qp);
  if (crc != SRSRAN_SUCCESS) {
    return crc;
  }
  UciDesc u  = h.uci;  // a second copy: the first upload may still be reading h
  u.cqi_bits = cqi_len;
  u.cqi_Qp   = cqi_Qp;
  if (cqi_len && (hipMemcpyAsync(&d_s->uci, &u, sizeof(UciDesc), hipMemcpyHostToDevice, x->stream) != hipSuccess ||
                  uci_cqi_launch(&d_s->uci, 1, x->stream) != hipSuccess)) {
    return SRSRAN_ERROR;
  }

  // ---- decode_tb over the UL-SCH part (after the CQI) ----
  int ret = cq.data_enable ? (int)cqi_Qp : (int)p.ri_Qp;  // the value left in ret when there is no TB
  if (p.s.tbs > 0) {
    srsran_pdsch_cfg_t pc;
    memset(&pc, 0, sizeof(pc));
    pc.grant.nof_tb          = 1;
    pc.grant.tb[0]           = cfg->grant.tb;
    pc.grant.tb[0].nof_bits  = (H - p.ri_Qp - cqi_Qp) * Qm;
    pc.softbuffers.rx[0]     = cfg->softbuffers.rx;
    pc.max_nof_iterations    = cfg->max_nof_iterations;
    ret                      = dlsch_decode_sync(q, &pc, nullptr, d_g + (size_t)cqi_Qp * Qm, data, 0, 1);
  }
  if (hipMemcpyAsync(&h.out, &d_s->out, sizeof(UciOut), hipMemcpyDeviceToHost, x->stream) != hipSuccess ||
      (q_out && hipMemcpyAsync(q_out, d_q, (size_t)nb * 2, hipMemcpyDeviceToHost, x->stream) != hipSuccess) ||
      (g_bits && hipMemcpyAsync(g_bits, d_g, (size_t)nb * 2, hipMemcpyDeviceToHost, x->stream) != hipSuccess) ||
      hipStreamSynchronize(x->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  ulsch_uci_out(cfg, p, h.out, uci_data);
  return ret;
}

}  // namespace

extern "C" int srsran_ulsch_decode(srsran_sch_t*       q,
                                   srsran_pusch_cfg_t* cfg,
                                   int16_t*            q_bits,
                                   int16_t*            g_bits,
                                   uint8_t*            c_seq,
                                   uint8_t*            data,
                                   srsran_uci_value_t* uci_data)
{
  if (!q_bits || !g_bits) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  return ulsch_decode_impl(q, cfg, q_bits, nullptr, q_bits, g_bits, c_seq, nullptr, data, uci_data);
}

namespace srsran_amd {

int ulsch_decode_dev(srsran_sch_t* q, srsran_pusch_cfg_t* cfg, int16_t* d_q, const uint8_t* d_c, uint8_t* data,
                     srsran_uci_value_t* uci_data)
{
  return ulsch_decode_impl(q, cfg, nullptr, d_q, nullptr, nullptr, nullptr, d_c, data, uci_data);
}

// Batched srsran_ulsch_decode (sch_internal.h): the same stages as ulsch_decode_impl, each one launch
// over every UE of the batch, and one decode_tb batch for all their transport blocks.
int ulsch_decode_batch_dev(srsran_sch_t* q, uint32_t n, UlschBatchUe* ues, const uint8_t* d_data_base,
                           size_t data_bytes, hipStream_t st)
{
  if (!q || !q->gpu || (n && !ues)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (q->llr_is_8bit) {
    return SRSRAN_ERROR;
  }
  SchCtx*              x = (SchCtx*)q->gpu;
  std::vector<UlsPlan> plan(n);
  std::vector<int32_t> uix(n, -1);  // index in the UCI arrays
  std::vector<uint32_t> live;
  uint32_t              m = 0, max_rows = 0;
  bool                  need_ri = false;
  for (uint32_t i = 0; i < n; i++) {
    UlschBatchUe& u = ues[i];
    u.avg           = NAN;
    u.ret           = u.cfg ? ulsch_plan(u.cfg, &plan[i]) : SRSRAN_ERROR_INVALID_INPUTS;
    if (u.ret == SRSRAN_SUCCESS &&
        (!u.d_q || !u.d_g || (plan[i].uci && !u.uci) || (plan[i].need_c && !u.d_c) ||
         (plan[i].s.tbs > 0 && (!u.cfg->softbuffers.rx || !u.d_data || u.d_data < d_data_base ||
                                u.d_data + plan[i].s.tbs / 8 > d_data_base + data_bytes)))) {
      u.ret = SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (u.ret != SRSRAN_SUCCESS) {
      continue;
    }
    live.push_back(i);
    max_rows = std::max(max_rows, plan[i].rows);
    if (plan[i].uci) {
      uix[i] = (int32_t)m++;
      need_ri |= plan[i].hl_ri;
    }
  }
  const uint32_t nl = (uint32_t)live.size();
  // device scratch: UciDesc[m] | UlDeint[nl] | UciOut[m] | result[nl] | avg[nl]; pinned staging:
  // the two uploads (the CQI pass rewrites the UCI descriptors) and the read-back
  const size_t o_dd = align16(m * sizeof(UciDesc)), o_out = o_dd + align16(nl * sizeof(UlDeint));
  const size_t o_res = o_out + align16(m * sizeof(UciOut)), o_avg = o_res + align16(nl * sizeof(int32_t));
  const size_t dev_need = o_avg + align16(nl * sizeof(float));
  const size_t h_cqi = dev_need, h_back = h_cqi + align16(m * sizeof(UciDesc));
  const size_t back_len = dev_need - o_out, h_need = h_back + back_len + data_bytes;
  if (!x->d_ubs.reserve(dev_need) || !x->h_ubs.reserve(h_need)) {
    return SRSRAN_ERROR;
  }
  uint8_t* d = x->d_ubs;
  uint8_t* h = x->h_ubs;
  UciDesc* h_ud  = (UciDesc*)h;
  UlDeint* h_dd  = (UlDeint*)(h + o_dd);
  UciOut*  d_out = (UciOut*)(d + o_out);
  for (uint32_t j = 0; j < nl; j++) {
    const uint32_t i = live[j];
    const UlsPlan& p = plan[i];
    h_dd[j]          = ulsch_deint_desc(ues[i].d_q, ues[i].d_g, p);
    if (uix[i] >= 0) {
      h_ud[uix[i]] = {ues[i].d_q, p.need_c ? ues[i].d_c : nullptr, ues[i].d_g, d_out + uix[i], p.Qm, p.rows, p.nsymb,
                      p.nack, p.ack_Qp, ues[i].cfg->uci_cfg.cqi.ri_len, p.ri_Qp, 0, 0};
    }
  }
  // ACK decode + zeroing and RI decode (sch.c:1023-1120), then the de-interleaver reading the zeroed q
  if (nl && (hipMemcpyAsync(d, h, o_out, hipMemcpyHostToDevice, st) != hipSuccess ||
             (m && uci_ack_ri_launch((const UciDesc*)d, m, st) != hipSuccess) ||
             ul_deint_batch_launch((const UlDeint*)(d + o_dd), nl, max_rows, st) != hipSuccess)) {
    return SRSRAN_ERROR;
  }
  UciOut* h_out = (UciOut*)(h + h_back);
  if (need_ri && (hipMemcpyAsync(h_out, d_out, m * sizeof(UciOut), hipMemcpyDeviceToHost, st) != hipSuccess ||
                  hipStreamSynchronize(st) != hipSuccess)) {
    return SRSRAN_ERROR;
  }
  // CQI sizes (after the RI where the report needs it) and the UL-SCH parts
  std::vector<uint32_t>              cqi_Qp(n, 0);
  std::vector<srsran_dlsch_gpu_tb_t> tbs;
  std::vector<int32_t>               tbix(n, -1);
  UciDesc*                           h_ud2 = (UciDesc*)(h + h_cqi);
  bool                               any_cqi = false;
  std::vector<uint32_t>              tb_maxit;  // each TB's max_nof_iterations (pusch.c:450 sets it per UE)
  memcpy(h_ud2, h_ud, m * sizeof(UciDesc));
  for (uint32_t i : live) {
    UlschBatchUe&  u = ues[i];
    const UlsPlan& p = plan[i];
    if (uix[i] >= 0) {
      uint32_t len = 0;
      u.ret        = ulsch_cqi_plan(u.cfg, p, need_ri ? h_out[uix[i]].ri[0] : 0, &len, &cqi_Qp[i]);
      if (u.ret != SRSRAN_SUCCESS) {
        continue;
      }
      h_ud2[uix[i]].cqi_bits = len;
      h_ud2[uix[i]].cqi_Qp   = cqi_Qp[i];
      any_cqi |= len > 0;
    }
    if (p.s.tbs > 0) {
      srsran_dlsch_gpu_tb_t t;
      memset(&t, 0, sizeof(t));
      t.tbs        = p.s.tbs;
      t.Qm         = p.Qm;
      t.rv         = (uint32_t)u.cfg->grant.tb.rv;
      t.nof_e_bits = (p.H - p.ri_Qp - cqi_Qp[i]) * p.Qm;
      t.d_e_bits   = u.d_g + (size_t)cqi_Qp[i] * p.Qm;
      t.d_data     = u.d_data;
      t.softbuffer = u.cfg->softbuffers.rx;
      t.new_data   = u.new_data ? 1 : 0;
      tbix[i]      = (int32_t)tbs.size();
      tbs.push_back(t);
      tb_maxit.push_back(u.cfg->max_nof_iterations ? u.cfg->max_nof_iterations : 10);  // set unconditionally
    }
  }
  if (any_cqi && (hipMemcpyAsync(d, h_ud2, m * sizeof(UciDesc), hipMemcpyHostToDevice, st) != hipSuccess ||
                  uci_cqi_launch((const UciDesc*)d, m, st) != hipSuccess)) {
    return SRSRAN_ERROR;
  }
  if (!tbs.empty() &&
      srsran_amd::dlsch_gpu_decode_batch_limits(q, (uint32_t)tbs.size(), tbs.data(), tb_maxit.data(),
                                                (int32_t*)(d + o_res), (float*)(d + o_avg), st) != SRSRAN_SUCCESS) {
    return SRSRAN_ERROR;  // one decode batch per UE iteration limit (pusch.c:450 sets it per decode)
  }
  // results, UCI and payloads back in one sync
  if ((nl && hipMemcpyAsync(h + h_back, d + o_out, back_len, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      (!tbs.empty() && data_bytes &&
       hipMemcpyAsync(h + h_back + back_len, d_data_base, data_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipStreamSynchronize(st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  const int32_t* h_res = (const int32_t*)(h + h_back + (o_res - o_out));
  const float*   h_avg = (const float*)(h + h_back + (o_avg - o_out));
  float          last  = q->avg_iterations;  // avg_iterations as sequential decodes would leave it
  for (uint32_t i = 0; i < n; i++) {
    UlschBatchUe&  u = ues[i];
    const UlsPlan& p = plan[i];
    if (uix[i] < 0 && tbix[i] < 0) {
      u.avg = last;
      continue;  // a failed check, or neither UCI nor a TB: srsran_ulsch_decode returns SUCCESS
    }
    if (u.ret != SRSRAN_SUCCESS) {
      u.avg = last;
      continue;
    }
    if (uix[i] >= 0) {
      ulsch_uci_out(u.cfg, p, h_out[uix[i]], u.uci);
      u.ret = u.cfg->uci_cfg.cqi.data_enable ? (int)cqi_Qp[i] : (int)p.ri_Qp;
    }
    if (tbix[i] >= 0) {
      u.ret = h_res[tbix[i]];
      last  = h_avg[tbix[i]];
      if (u.data) {
        memcpy(u.data, h + h_back + back_len + (u.d_data - d_data_base), p.s.tbs / 8);
      }
    }
    u.avg = last;
  }
  q->avg_iterations = last;
  return SRSRAN_SUCCESS;
}
}  // namespace srsran_amd

extern "C" int srsran_ulsch_gpu_decode_batch(srsran_sch_t*                q,
                                             uint32_t                     nof_tb,
                                             const srsran_ulsch_gpu_tb_t* tbs,
                                             int32_t*                     d_result,
                                             float*                       d_avg_noi,
                                             void*                        stream)
{
  if (!q || !q->gpu || (nof_tb && (!tbs || !d_result || !d_avg_noi))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (q->llr_is_8bit) {
    return SRSRAN_ERROR;
  }
  std::vector<srsran_dlsch_gpu_tb_t> dl(nof_tb);
  std::vector<UlDeint>               desc(nof_tb);
  uint32_t                           max_n = 0;
  for (uint32_t i = 0; i < nof_tb; i++) {
    const srsran_ulsch_gpu_tb_t& t = tbs[i];
    if (!t.d_q_bits || !t.d_g_bits || t.Qm == 0 || t.Qm > 8 || t.nof_symb == 0 || t.nof_symb > 14 ||
        t.nof_e_bits % t.Qm) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    const uint32_t rows = t.nof_e_bits / t.Qm / t.nof_symb;
    desc[i]             = {t.d_q_bits, t.d_g_bits, rows, t.nof_symb, t.Qm, {}, -1};
    max_n               = std::max(max_n, rows);
    dl[i]               = {t.tbs, t.Qm, t.rv, t.nof_e_bits, t.d_g_bits, t.d_data, t.softbuffer, t.new_data};
  }
  SchCtx* x = (SchCtx*)q->gpu;
  // the previous call's de-interleaver must have read its descriptors before staging is rewritten
  if (x->uldesc_live) {
    hipEventSynchronize(x->uldesc_used);
  }
  if (!x->uldesc_used && hipEventCreateWithFlags(&x->uldesc_used, hipEventDisableTiming) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  if (nof_tb > x->d_uldesc.cap() || nof_tb > x->h_uldesc.cap()) {
    const size_t cap = std::max<size_t>(2 * nof_tb, 64);
    if (!x->d_uldesc.reserve(cap) || !x->h_uldesc.reserve(cap)) {
      return SRSRAN_ERROR;
    }
  }
  if (nof_tb) {
    memcpy(x->h_uldesc, desc.data(), nof_tb * sizeof(UlDeint));
    if (hipMemcpyAsync(x->d_uldesc, x->h_uldesc, nof_tb * sizeof(UlDeint), hipMemcpyHostToDevice,
                       (hipStream_t)stream) != hipSuccess ||
        ul_deint_batch_launch(x->d_uldesc, nof_tb, max_n, (hipStream_t)stream) != hipSuccess) {
      return SRSRAN_ERROR;
    }
    hipEventRecord(x->uldesc_used, (hipStream_t)stream);
    x->uldesc_live = true;
  }
  return srsran_dlsch_gpu_decode_batch(q, nof_tb, dl.data(), d_result, d_avg_noi, stream);
}

// ---------------- UL-SCH transmit with UCI (sch.c:1195-1337; uci.c:200-257, 334-361, 457-632) ----------------
namespace {

struct UlsTxPlan {
  srsran_cbsegm_t      s;
  uint32_t             Qm, nsymb, H, rows, ri_Qp, ack_Qp, cqi_Qp, G;
  std::vector<uint8_t> cqi, ri, ack;
};

// srsran_ulsch_encode's host part: returns (Q'_ACK + Q'_RI) Qm or an error
int ulsch_tx_plan(srsran_pusch_cfg_t* cfg, const srsran_uci_value_t* uci, UlsTxPlan* p)
{
  const uint32_t nb_q = cfg->grant.tb.nof_bits;
  p->Qm               = srsran_mod_bits_x_symbol(cfg->grant.tb.mod);
  p->nsymb            = cfg->grant.nof_symb;
  if (p->Qm == 0 || p->nsymb == 0) {
    fprintf(stderr, "[srsran_sch] Invalid input\n");
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  // the multiplexing kernel's shapes: QPSK / 16QAM / 64QAM, whole interleaver columns, four symbols a thread
  if (p->Qm > 6 || p->nsymb > 14 || nb_q % p->Qm || (nb_q / p->Qm) % p->nsymb ||
      (nb_q / p->Qm) % PUSCH_TX_SYM_PER_THREAD || cfg->grant.tb.rv < 0 || cfg->grant.tb.rv > 3) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  srsran_cbsegm_t& s = p->s;
  if (cfg->grant.tb.tbs < 0 || srsran_cbsegm(&s, (uint32_t)cfg->grant.tb.tbs)) {
    fprintf(stderr, "[srsran_sch] Error computing segmentation for TBS=%d\n", cfg->grant.tb.tbs);
    return SRSRAN_ERROR;
  }
  if (s.F) {
    fprintf(stderr, "[srsran_sch] Error filler bits are not supported. Use standard TBS\n");
    return SRSRAN_ERROR;
  }
  cfg->K_segm = s.C1 * s.K1 + s.C2 * s.K2;
  p->H        = nb_q / p->Qm;
  p->rows     = p->H / p->nsymb;
  p->ri_Qp = p->ack_Qp = p->cqi_Qp = 0;

  srsran_cqi_cfg_t& cq = cfg->uci_cfg.cqi;
  uint8_t           cqi_buff[SRSRAN_CQI_MAX_BITS];
  memset(cqi_buff, 0, sizeof(cqi_buff));
  int cqi_len = 0;
  if (cq.data_enable) {
    if (!uci || (cqi_len = srsran_cqi_value_pack(&cq, const_cast<srsran_cqi_value_t*>(&uci->cqi), cqi_buff)) < 0 ||
        cqi_len > (int)UCI_MAX_CQI_BITS) {
      fprintf(stderr, "[srsran_sch] Error encoding CQI bits\n");
      return SRSRAN_ERROR;
    }
  }
  const uint32_t nack = srsran_uci_cfg_total_ack(&cfg->uci_cfg);
  if ((nack > 0 || cq.ri_len > 0) && !uci) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (cq.ri_len > 0) {
    if (cq.ri_len > 2) {  // the reference encodes ri[2] = {ri, 0}: one or two bits
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    p->ri_Qp = qprime_ri_ack_cfg(cfg, s.tbs == 0, p->nsymb, cq.ri_len, (uint32_t)cqi_len,
                                 beta_ri(cfg->uci_offset.I_offset_ri));
    if ((int)p->ri_Qp < 0) {
      return (int)p->ri_Qp;
    }
    const uint8_t ri[2] = {uci->ri, 0};
    ri_ack_types(ri, cq.ri_len, p->Qm, p->ri_Qp, p->ri);
  }
  if (p->ri_Qp > 4 * p->rows || p->ri_Qp > p->H) {  // uci.c:400-415 "Error interleaving"
    fprintf(stderr, "[srsran_sch] UCI does not fit the PUSCH interleaver (Q'_RI=%u rows=%u)\n", p->ri_Qp, p->rows);
    return SRSRAN_ERROR;
  }
  if (cqi_len > 0) {
    const float beta = beta_cqi(cfg->uci_offset.I_offset_cqi);
    p->cqi_Qp        = qprime_cqi(cfg->K_segm, cfg->grant.L_prb, p->nsymb, (uint32_t)cqi_len, beta, p->ri_Qp);
    if ((uint64_t)p->cqi_Qp + p->ri_Qp > p->H) {
      return SRSRAN_ERROR;
    }
    p->cqi.assign((size_t)p->cqi_Qp * p->Qm, 0);
    if (cqi_len <= 11) {
      block_encode(cqi_buff, (uint32_t)cqi_len, p->cqi.data(), (uint32_t)p->cqi.size());
    } else if (!cqi_encode_long(cqi_buff, (uint32_t)cqi_len, p->cqi.data(), (uint32_t)p->cqi.size())) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
  }
  p->G = p->H - p->ri_Qp - p->cqi_Qp;
  if (nack > 0) {
    if (nack > SRSRAN_UCI_MAX_ACK_BITS) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    p->ack_Qp = qprime_ri_ack_cfg(cfg, s.tbs == 0, p->nsymb, nack, (uint32_t)cqi_len,
                                  beta_harq(cfg->uci_offset.I_offset_ack));
    if ((int)p->ack_Qp < 0) {
      return (int)p->ack_Qp;
    }
    if (p->ack_Qp > 4 * p->rows) {  // uci.c:373-387
      fprintf(stderr, "[srsran_sch] UCI does not fit the PUSCH interleaver (Q'_ACK=%u rows=%u)\n", p->ack_Qp, p->rows);
      return SRSRAN_ERROR;
    }
    ri_ack_types(uci->ack.ack_value, nack, p->Qm, p->ack_Qp, p->ack);
    ack_scramble_tdd(p->ack, nack, cfg->uci_cfg.ack[0].N_bundle);
  }
  return (int)((p->ack_Qp + p->ri_Qp) * p->Qm);
}

}  // namespace

namespace srsran_amd {

int ulsch_tx_prepare(srsran_sch_t* q, uint32_t n, UlschTxJob* jobs, PuschTxUe* desc, hipStream_t st)
{
  if (!q || !q->gpu || (n && (!jobs || !desc))) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  SchCtx*                x = (SchCtx*)q->gpu;
  std::vector<UlsTxPlan> plan(n);
  std::vector<EncTb>     tb;
  std::vector<EncCb>     cb;
  EncFwdMap              fwd;
  std::vector<uint8_t>   lists;  // every job's CQI bits, RI types, ACK types
  struct Off {
    size_t cqi, ri, ack, e, g, qb, sb, d;
    int    tb;
  };
  std::vector<Off> off(n);
  size_t           e_tot = 0, bits_tot = 0, sym_tot = 0;
  for (uint32_t i = 0; i < n; i++) {
    UlschTxJob& j = jobs[i];
    UlsTxPlan&  p = plan[i];
    j.ret         = j.cfg ? ulsch_tx_plan(j.cfg, j.uci, &p) : SRSRAN_ERROR_INVALID_INPUTS;
    if (j.ret < 0) {
      return j.ret;
    }
    Off& o = off[i];
    o.cqi  = lists.size();
    lists.insert(lists.end(), p.cqi.begin(), p.cqi.end());
    o.ri = lists.size();
    lists.insert(lists.end(), p.ri.begin(), p.ri.end());
    o.ack = lists.size();
    lists.insert(lists.end(), p.ack.begin(), p.ack.end());
    o.tb = -1;
    o.e  = e_tot;
    if (p.s.tbs > 0) {
      if (!j.d_data) {
        fprintf(stderr, "[srsran_sch] encoding from the soft buffer (data == NULL) is not provided\n");
        return j.ret = SRSRAN_ERROR;
      }
      const uint32_t ne = p.G * p.Qm;
      uint32_t       wp = 0;
      o.tb              = (int)tb.size();
      const int r = enc_push_cbs(cb, fwd, p.s, p.Qm, (uint32_t)j.cfg->grant.tb.rv, ne, j.d_data, p.s.tbs, e_tot,
                                 (uint32_t)o.tb, &wp);
      if (r != SRSRAN_SUCCESS || wp > ne) {
        return j.ret = r != SRSRAN_SUCCESS ? r : SRSRAN_ERROR_INVALID_INPUTS;
      }
      tb.push_back({j.d_data, nullptr, nullptr, nullptr, p.s.tbs / 8, ne});
      e_tot += align16(ne);
    }
    const size_t nbytes = align16((size_t)p.H * p.Qm / 8);
    o.g  = bits_tot;
    o.qb = bits_tot + nbytes;
    o.sb = bits_tot + 2 * nbytes;
    bits_tot += 3 * nbytes;
    o.d = sym_tot;
    sym_tot += p.H;
  }
  // device scratch: [EncTb][EncCb][lists] (uploaded) [TB CRCs][e bits][g / q / scrambled bits][symbols]
  const size_t o_cb = align16(tb.size() * sizeof(EncTb)), o_lists = o_cb + align16(cb.size() * sizeof(EncCb));
  const size_t o_crc = o_lists + align16(lists.size()), o_e = o_crc + align16(tb.size() * sizeof(uint32_t));
  const size_t o_bits = o_e + e_tot, o_sym = o_bits + bits_tot, need = o_sym + sym_tot * sizeof(float2);
  if (!x->d_ultx.reserve(need)) {
    return SRSRAN_ERROR;
  }
  uint8_t*  base  = x->d_ultx;
  uint32_t* d_crc = (uint32_t*)(base + o_crc);
  for (size_t t = 0; t < tb.size(); t++) {
    tb[t].crc = d_crc + t;
  }
  for (EncCb& c : cb) {
    c.e      = base + o_e + (size_t)(uintptr_t)c.e;
    c.tb_crc = d_crc + (size_t)(uintptr_t)c.tb_crc;
  }
  for (uint32_t i = 0; i < n; i++) {
    const UlsTxPlan& p = plan[i];
    const Off&       o = off[i];
    PuschTxUe&       u = desc[i];
    u.cqi    = base + o_lists + o.cqi;
    u.ri     = base + o_lists + o.ri;
    u.ack    = base + o_lists + o.ack;
    u.e      = o.tb >= 0 ? base + o_e + o.e : nullptr;
    u.g_pack = jobs[i].want_g ? base + o_bits + o.g : nullptr;
    u.q_pack = jobs[i].want_q ? base + o_bits + o.qb : nullptr;
    u.s_pack = base + o_bits + o.sb;
    u.d      = (float2*)(base + o_sym) + o.d;
    u.mod    = (uint32_t)jobs[i].cfg->grant.tb.mod;
    u.Qm     = p.Qm;
    u.rows   = p.rows;
    u.cols   = p.nsymb;
    u.H      = p.H;
    u.ncqi   = p.cqi_Qp * p.Qm;
    u.ne     = o.tb >= 0 ? p.G * p.Qm : 0;
    u.ri_Qp  = p.ri_Qp;
    u.ack_Qp = p.ack_Qp;
    memcpy(u.ri_col, uci_ri_cols(p.nsymb), 4);
    memcpy(u.ack_col, uci_ack_cols(p.nsymb), 4);
  }
  if ((!tb.empty() && hipMemcpyAsync(base, tb.data(), tb.size() * sizeof(EncTb), hipMemcpyHostToDevice, st) != hipSuccess) ||
      (!cb.empty() &&
       hipMemcpyAsync(base + o_cb, cb.data(), cb.size() * sizeof(EncCb), hipMemcpyHostToDevice, st) != hipSuccess) ||
      (!lists.empty() &&
       hipMemcpyAsync(base + o_lists, lists.data(), lists.size(), hipMemcpyHostToDevice, st) != hipSuccess) ||
      enc_tb_crc_launch((const EncTb*)base, (uint32_t)tb.size(), st) != hipSuccess ||
      enc_cb_launch((const EncCb*)(base + o_cb), (uint32_t)cb.size(), st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

}  // namespace srsran_amd

extern "C" int srsran_ulsch_encode(srsran_sch_t*       q,
                                   srsran_pusch_cfg_t* cfg,
                                   uint8_t*            data,
                                   srsran_uci_value_t* uci_data,
                                   uint8_t*            g_bits,
                                   uint8_t*            q_bits)
{
  if (!q || !q->gpu || !cfg || !g_bits || !q_bits) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  SchCtx*        x      = (SchCtx*)q->gpu;
  const uint32_t nbytes = cfg->grant.tb.tbs > 0 ? (uint32_t)cfg->grant.tb.tbs / 8 : 0;
  if (nbytes && !data) {
    fprintf(stderr, "[srsran_sch] encoding from the soft buffer (data == NULL) is not provided\n");
    return SRSRAN_ERROR;
  }
  // payload and the descriptor on the device for the length of the call
  uint8_t* d_io = nullptr;
  if (hipMallocAsync((void**)&d_io, align16(nbytes + 16) + sizeof(PuschTxUe), x->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  PuschTxUe* d_desc = (PuschTxUe*)(d_io + align16(nbytes + 16));
  PuschTxUe  u;
  memset(&u, 0, sizeof(u));
  UlschTxJob job = {cfg, uci_data, nbytes ? d_io : nullptr, true, true, 0};
  int        ret = SRSRAN_ERROR;
  if (!nbytes || hipMemcpyAsync(d_io, data, nbytes, hipMemcpyHostToDevice, x->stream) == hipSuccess) {
    ret = ulsch_tx_prepare(q, 1, &job, &u, x->stream);
    if (ret == SRSRAN_SUCCESS) {
      const uint32_t ng = (u.ncqi + u.ne + 7) / 8, nq = u.H * u.Qm / 8;
      ret               = job.ret;
      if (hipMemcpyAsync(d_desc, &u, sizeof(u), hipMemcpyHostToDevice, x->stream) != hipSuccess ||
          pusch_tx_mux_launch(d_desc, 1, u.H, x->stream) != hipSuccess ||
          (ng && hipMemcpyAsync(g_bits, u.g_pack, ng, hipMemcpyDeviceToHost, x->stream) != hipSuccess) ||
          hipMemcpyAsync(q_bits, u.q_pack, nq, hipMemcpyDeviceToHost, x->stream) != hipSuccess) {
        ret = SRSRAN_ERROR;
      }
    }
  }
  hipFreeAsync(d_io, x->stream);
  if (hipStreamSynchronize(x->stream) != hipSuccess) {
    ret = SRSRAN_ERROR;
  }
  return ret;
}
