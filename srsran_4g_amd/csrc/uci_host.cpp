// srsran_4g_amd/csrc/uci_host.cpp -- UCI on PUSCH, host arithmetic only (include/srsran_sch.h, uci_host.h):
//   offset tables and their inverse   sch.c:43-136
//   Q'_ACK / Q'_RI / Q'_CQI           uci.c:170-186, 414-440
//   CQI report sizes, pack, unpack    cqi.c:41-384
//   the transmitter's channel coding  block.c:78-104, uci.c:225-257, 457-613
// No HIP include: the unit builds with a plain C++ compiler, alone or into the library.
#include "uci_host.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace srsran_amd {

float beta_harq(uint32_t i)
{
  static const float t[15] = {2.0f, 2.5f, 3.125f, 4.0f, 5.0f, 6.25f, 8.0f, 10.0f, 12.625f, 15.875f, 20.0f, 31.0f,
                              50.0f, 80.0f, 126.0f};
  if (i < 15) {
    return t[i];
  }
  fprintf(stderr, "[srsran_sch] Invalid I_offset_ack %u (min: 0, max: 14)\n", i);
  return t[0];
}

float beta_ri(uint32_t i)
{
  static const float t[13] = {1.25f, 1.625f, 2.0f, 2.5f, 3.125f, 4.0f, 5.0f, 6.25f, 8.0f, 10.0f, 12.625f, 15.875f,
                              20.0f};
  if (i < 13) {
    return t[i];
  }
  fprintf(stderr, "[srsran_sch] Invalid I_offset_ri %u (min: 0, max: 12)\n", i);
  return t[0];
}

float beta_cqi(uint32_t i)
{
  static const float t[16] = {-1.0f, -1.0f, 1.125f, 1.25f, 1.375f, 1.625f, 1.75f, 2.0f, 2.25f, 2.5f, 2.875f,
                              3.125f, 3.5f, 4.0f, 5.0f, 6.25f};
  if (i > 1 && i < 16) {
    return t[i];
  }
  fprintf(stderr, "[srsran_sch] Invalid I_offset_cqi %u (min: 2, max: 15)\n", i);
  return t[2];
}

uint32_t qprime_ri_ack(uint32_t K, uint32_t L_prb, uint32_t nof_symb, uint32_t O, uint32_t O_cqi, float beta)
{
  if (beta < 0) {
    return (uint32_t)-1;
  }
  if (K == 0) {  // no UL-SCH: 5.2.4.1
    K = O_cqi <= 11 ? O_cqi : O_cqi + 8;
  }
  if (K == 0) {
    return 0;
  }
  const uint32_t x = (uint32_t)ceilf((float)O * (float)L_prb * (float)SRSRAN_NRE * (float)nof_symb * beta / (float)K);
  return std::min(x, 4 * L_prb * SRSRAN_NRE);
}

uint32_t qprime_ri_ack_cfg(const srsran_pusch_cfg_t* cfg, bool no_tb, uint32_t nof_symb, uint32_t O, uint32_t O_cqi,
                           float beta)
{
  if (no_tb) {
    beta /= beta_cqi(cfg->uci_offset.I_offset_cqi);
  }
  return qprime_ri_ack(cfg->K_segm, cfg->grant.L_prb, nof_symb, O, O_cqi, beta);
}

uint32_t qprime_cqi(uint32_t K, uint32_t L_prb, uint32_t nof_symb, uint32_t O, float beta, uint32_t Q_prime_ri)
{
  const uint32_t L = O < 11 ? 0 : 8;
  uint32_t       x = 999999;
  if (K > 0) {
    x = (uint32_t)ceilf((float)(O + L) * (float)L_prb * (float)SRSRAN_NRE * (float)nof_symb * beta / (float)K);
  }
  return std::min(x, L_prb * SRSRAN_NRE * nof_symb - Q_prime_ri);
}

const uint8_t* uci_ri_cols(uint32_t nof_symb)
{
  static const uint8_t norm[4] = {1, 4, 7, 10}, ext[4] = {0, 3, 5, 8};
  return nof_symb > 10 ? norm : ext;
}

const uint8_t* uci_ack_cols(uint32_t nof_symb)
{
  static const uint8_t norm[4] = {2, 3, 8, 9}, ext[4] = {1, 2, 6, 7};
  return nof_symb > 10 ? norm : ext;
}

// (32, O) basis sequences, 36.212 Table 5.2.2.6.4-1, as block_dev.h's kBlockBasis (a __constant__ the host cannot
// read): bit n of word i is M_{i,n}
static const uint16_t kBlockBasisHost[32] = {0x403, 0x607, 0x749, 0x50D, 0x48F, 0x5D3, 0x755, 0x599, 0x69B, 0x65D, 0x6E5,
                                             0x567, 0x7A9, 0x6AB, 0x4B1, 0x6F3, 0x277, 0x139, 0x0FB, 0x061, 0x445, 0x60B,
                                             0x591, 0x717, 0x3DF, 0x4E3, 0x32D, 0x3AF, 0x175, 0x1FD, 0x7FF, 0x001};

void block_encode(const uint8_t* in, uint32_t nin, uint8_t* out, uint32_t nout)
{
  uint32_t w = 0;
  for (uint32_t i = 0; i < std::min(nin, 11u); i++) {
    w |= (uint32_t)(in[i] & 1u) << i;
  }
  for (uint32_t i = 0; i < nout; i++) {
    out[i] = (uint8_t)(__builtin_popcount(w & kBlockBasisHost[i % 32]) & 1);
  }
}

bool cqi_encode_long(const uint8_t* data, uint32_t nbits, uint8_t* out, uint32_t Q)
{
  if (nbits + 8 >= 512) {  // SRSRAN_UCI_MAX_CQI_LEN_PUSCH
    return false;
  }
  const uint8_t        kTxNull = 100;  // SRSRAN_TX_NULL (turbocoder.h:40-42): a dummy bit of the interleaver
  const uint32_t       F       = nbits + 8;
  std::vector<uint8_t> in(F), coded(3 * F);
  uint32_t             crc = 0;
  for (uint32_t i = 0; i < nbits; i++) {
    in[i]              = data[i] & 1u;
    const uint32_t top = ((crc >> 7) & 1u) ^ in[i];
    crc                = ((crc << 1) & 0xFFu) ^ (top ? 0x9Bu : 0u);
  }
  for (uint32_t i = 0; i < 8; i++) {
    in[nbits + i] = (uint8_t)((crc >> (7 - i)) & 1u);
  }
  static const uint32_t poly[3] = {0x6D, 0x4F, 0x57};
  uint32_t              sr      = 0;
  for (uint32_t i = F - 6; i < F; i++) {
    sr = (sr << 1) | in[i];
  }
  for (uint32_t i = 0; i < F; i++) {
    sr = (sr << 1) | in[i];
    for (uint32_t j = 0; j < 3; j++) {
      coded[3 * i + j] = (uint8_t)(__builtin_popcount(sr & poly[j]) & 1);
    }
  }
  static const uint8_t perm[32] = {1, 17, 9,  25, 5, 21, 13, 29, 3, 19, 11, 27, 7, 23, 15, 31,
                                   0, 16, 8,  24, 4, 20, 12, 28, 2, 18, 10, 26, 6, 22, 14, 30};  // RM_PERM_CC
  const uint32_t       nrows = (F - 1) / 32 + 1, Kp = nrows * 32, ndummy = Kp - F;
  std::vector<uint8_t> tmp(3 * Kp);
  uint32_t             k = 0;
  for (uint32_t s = 0; s < 3; s++) {
    for (uint32_t j = 0; j < 32; j++) {
      for (uint32_t i = 0; i < nrows; i++) {
        const uint32_t x = i * 32 + perm[j];
        tmp[k++]         = x < ndummy ? kTxNull : coded[(x - ndummy) * 3 + s];
      }
    }
  }
  for (uint32_t n = 0, j = 0; n < Q; j = (j + 1) % (3 * Kp)) {
    if (tmp[j] != kTxNull) {
      out[n++] = tmp[j];
    }
  }
  return true;
}

void ri_ack_types(const uint8_t* data, uint32_t O, uint32_t Qm, uint32_t Qp, std::vector<uint8_t>& t)
{
  t.assign((size_t)Qp * Qm, UCI_BIT_0);
  uint8_t  enc[32];
  uint32_t len;
  if (O == 1) {
    len = Qm;
    for (uint32_t i = 0; i < Qm; i++) {
      enc[i] = i == 0 ? (data[0] ? UCI_BIT_1 : UCI_BIT_0) : i == 1 ? UCI_BIT_REPETITION : UCI_BIT_PLACEHOLDER;
    }
  } else if (O == 2) {
    const uint8_t o[3] = {(uint8_t)(data[0] ? 1 : 0), (uint8_t)(data[1] ? 1 : 0), (uint8_t)((data[0] ^ data[1]) ? 1 : 0)};
    len                = 3 * Qm;  // [o0 o1 x..] [o2 o0 x..] [o1 o2 x..]
    for (uint32_t s = 0; s < 3; s++) {
      for (uint32_t i = 0; i < Qm; i++) {
        enc[s * Qm + i] = i < 2 ? o[(2 * s + i) % 3] : (uint8_t)UCI_BIT_PLACEHOLDER;
      }
    }
  } else {
    len = 32;
    block_encode(data, O, enc, 32);
  }
  for (size_t i = 0; i < t.size(); i++) {
    t[i] = enc[i % len];
  }
}

void ack_scramble_tdd(std::vector<uint8_t>& q, uint32_t O_ack, uint32_t N_bundle)
{
  if (N_bundle == 0 || q.empty()) {
    return;
  }
  static const uint8_t w_scram[4][4] = {{1, 1, 1, 1}, {1, 0, 1, 0}, {1, 1, 0, 0}, {1, 0, 0, 1}};  // Table 5.2.2.6-A
  const uint32_t       wi = (N_bundle - 1) % 4, m = O_ack == 1 ? 1 : 3;
  uint8_t              q_m1 = q[0];
  uint32_t             k = 0;
  for (size_t i = 0; i < q.size(); i++) {
    if (q[i] == UCI_BIT_REPETITION) {
      if (i > 0) {
        q[i] = (uint8_t)(((q_m1 == UCI_BIT_1 ? 1 : 0) + w_scram[wi][k / m]) % 2);
      }
      k = (k + 1) % (4 * m);
    } else if (q[i] != UCI_BIT_PLACEHOLDER) {
      q_m1 = q[i];
      q[i] = (uint8_t)(((q[i] == UCI_BIT_1 ? 1 : 0) + w_scram[wi][k / m]) % 2);
      k    = (k + 1) % (4 * m);
    }
  }
}

}  // namespace srsran_amd

using namespace srsran_amd;

extern "C" {

float srsran_sch_beta_cqi(uint32_t I_cqi) { return I_cqi < 16 ? beta_cqi(I_cqi) : 0.0f; }
float srsran_sch_beta_ack(uint32_t I_harq) { return I_harq < 16 ? beta_harq(I_harq) : 0.0f; }

// the first index whose offset reaches beta (sch.c:108-136, 16 indices through the getters)
static uint32_t find_Ioffset(float (*offset)(uint32_t), float beta)
{
  for (uint32_t i = 0; i < 16; i++) {
    if (offset(i) >= beta) {
      return i;
    }
  }
  return 0;
}
uint32_t srsran_sch_find_Ioffset_ack(float beta) { return find_Ioffset(beta_harq, beta); }
uint32_t srsran_sch_find_Ioffset_ri(float beta) { return find_Ioffset(beta_ri, beta); }
uint32_t srsran_sch_find_Ioffset_cqi(float beta) { return find_Ioffset(beta_cqi, beta); }

uint32_t srsran_uci_cfg_total_ack(const srsran_uci_cfg_t* uci_cfg)
{
  uint32_t n = 0;  // uci.c:716-723
  for (uint32_t i = 0; i < SRSRAN_MAX_CARRIERS; i++) {
    n += uci_cfg->ack[i].nof_acks;
  }
  return n;
}

uint32_t srsran_qprime_cqi_ext(uint32_t L_prb, uint32_t nof_symbols, uint32_t tbs, float beta)
{
  return qprime_cqi(tbs, L_prb, nof_symbols, 20 + 8, beta, 0);  // O = SRSRAN_UCI_CQI_CODED_PUCCH_B + 8
}

uint32_t srsran_qprime_ack_ext(uint32_t L_prb, uint32_t nof_symbols, uint32_t tbs, uint32_t nof_ack, float beta)
{
  return qprime_ri_ack(tbs, L_prb, nof_symbols, nof_ack, 0, beta);
}

// ---- CQI report sizes and fields, 36.212 Tables 5.2.2.6.2-1/-2, 5.2.3.3.1-1/-2 (cqi.c:41-384) ----
static uint32_t bits_get(const uint8_t** p, uint32_t n)  // srsran_bit_pack: MSB first
{
  uint32_t v = 0;
  for (uint32_t i = 0; i < n; i++) {
    v = (v << 1) | ((*p)[i] & 1u);
  }
  *p += n;
  return v;
}

static void bits_put(uint32_t v, uint8_t** p, uint32_t n)  // srsran_bit_unpack
{
  for (uint32_t i = 0; i < n; i++) {
    (*p)[i] = (uint8_t)((v >> (n - 1 - i)) & 1u);
  }
  *p += n;
}

int srsran_cqi_size(srsran_cqi_cfg_t* cfg)
{
  if (!cfg->data_enable) {
    return (int)cfg->ri_len;
  }
  int size = 0;
  switch (cfg->type) {
    case SRSRAN_CQI_TYPE_WIDEBAND:
      size = 4;
      if (cfg->pmi_present) {
        if (cfg->four_antenna_ports) {
          size += (cfg->rank_is_not_one ? 3 : 0) + 4;
        } else {
          size += cfg->rank_is_not_one ? 3 + 1 : 2;
        }
      }
      break;
    case SRSRAN_CQI_TYPE_SUBBAND_UE:
      size = 4 + (cfg->subband_label_2_bits ? 2 : 1);
      break;
    case SRSRAN_CQI_TYPE_SUBBAND_UE_DIFF:
      size = 4 + 2 + (int)cfg->L;
      break;
    case SRSRAN_CQI_TYPE_SUBBAND_HL:
      size = 4 + 2 * (int)cfg->N;
      if (cfg->rank_is_not_one && cfg->pmi_present) {
        size += 4 + 2 * (int)cfg->N;
      }
      if (cfg->pmi_present) {
        size += cfg->four_antenna_ports ? 4 : cfg->rank_is_not_one ? 1 : 2;
      }
      break;
    default:
      size = SRSRAN_ERROR;
  }
  return size;
}

int srsran_cqi_value_pack(srsran_cqi_cfg_t* cfg, srsran_cqi_value_t* v, uint8_t buff[SRSRAN_CQI_MAX_BITS])
{
  uint8_t* p = buff;
  switch (cfg->type) {
    case SRSRAN_CQI_TYPE_WIDEBAND:
      bits_put(v->wideband.wideband_cqi, &p, 4);
      if (cfg->pmi_present) {
        if (cfg->rank_is_not_one) {
          bits_put(v->wideband.spatial_diff_cqi, &p, 3);
        }
        bits_put(v->wideband.pmi, &p, cfg->four_antenna_ports ? 4 : cfg->rank_is_not_one ? 1 : 2);
      }
      return (int)(p - buff);
    case SRSRAN_CQI_TYPE_SUBBAND_UE:
      bits_put(v->subband_ue.subband_cqi, &p, 4);
      bits_put(v->subband_ue.subband_label, &p, cfg->subband_label_2_bits ? 2 : 1);
      return 4 + (cfg->subband_label_2_bits ? 2 : 1);
    case SRSRAN_CQI_TYPE_SUBBAND_UE_DIFF:  // the reference writes subband_diff_cqi twice (cqi.c:77-85)
      bits_put(v->subband_ue_diff.wideband_cqi, &p, 4);
      bits_put(v->subband_ue_diff.subband_diff_cqi, &p, 2);
      bits_put(v->subband_ue_diff.subband_diff_cqi, &p, cfg->L);
      return 4 + 2 + (int)cfg->L;
    case SRSRAN_CQI_TYPE_SUBBAND_HL: {
      int n = 4 + 2 * (int)cfg->N;
      bits_put(v->subband_hl.wideband_cqi_cw0, &p, 4);
      bits_put(v->subband_hl.subband_diff_cqi_cw0, &p, 2 * cfg->N);
      if (cfg->rank_is_not_one) {
        bits_put(v->subband_hl.wideband_cqi_cw1, &p, 4);
        bits_put(v->subband_hl.subband_diff_cqi_cw1, &p, 2 * cfg->N);
        n += 4 + 2 * (int)cfg->N;
      }
      if (cfg->pmi_present) {
        const uint32_t w = cfg->four_antenna_ports ? 4 : cfg->rank_is_not_one ? 1 : 2;
        bits_put(v->subband_hl.pmi, &p, w);
        n += (int)w;
      }
      return n;
    }
  }
  return -1;
}

int srsran_cqi_value_unpack(srsran_cqi_cfg_t* cfg, uint8_t buff[SRSRAN_CQI_MAX_BITS], srsran_cqi_value_t* v)
{
  const uint8_t* p = buff;
  switch (cfg->type) {
    case SRSRAN_CQI_TYPE_WIDEBAND:
      v->wideband.wideband_cqi = (uint8_t)bits_get(&p, 4);
      if (cfg->pmi_present) {
        if (cfg->rank_is_not_one) {
          v->wideband.spatial_diff_cqi = (uint8_t)bits_get(&p, 3);
        }
        v->wideband.pmi = (uint8_t)bits_get(&p, cfg->four_antenna_ports ? 4 : cfg->rank_is_not_one ? 1 : 2);
      }
      return 4;
    case SRSRAN_CQI_TYPE_SUBBAND_UE:
      v->subband_ue.subband_cqi   = (uint8_t)bits_get(&p, 4);
      v->subband_ue.subband_label = (uint8_t)bits_get(&p, cfg->subband_label_2_bits ? 2 : 1);
      return 4 + (cfg->subband_label_2_bits ? 2 : 1);
    case SRSRAN_CQI_TYPE_SUBBAND_UE_DIFF:  // the L-bit field overwrites the 2-bit one (cqi.c:175-184)
      v->subband_ue_diff.wideband_cqi     = (uint8_t)bits_get(&p, 4);
      v->subband_ue_diff.subband_diff_cqi = (uint8_t)bits_get(&p, 2);
      v->subband_ue_diff.subband_diff_cqi = (uint8_t)bits_get(&p, cfg->L);
      return 4 + 2 + (int)cfg->L;
    case SRSRAN_CQI_TYPE_SUBBAND_HL: {
      int n = 4 + 2 * (int)cfg->N;
      v->subband_hl.wideband_cqi_cw0     = (uint8_t)bits_get(&p, 4);
      v->subband_hl.subband_diff_cqi_cw0 = bits_get(&p, 2 * cfg->N);
      if (cfg->rank_is_not_one) {
        v->subband_hl.wideband_cqi_cw1     = (uint8_t)bits_get(&p, 4);
        v->subband_hl.subband_diff_cqi_cw1 = bits_get(&p, 2 * cfg->N);
        n += 4 + 2 * (int)cfg->N;
      }
      if (cfg->pmi_present) {
        const uint32_t w = cfg->four_antenna_ports ? 4 : cfg->rank_is_not_one ? 1 : 2;
        v->subband_hl.pmi = (uint8_t)bits_get(&p, w);
        n += (int)w;
      }
      return n;
    }
  }
  return -1;
}

}  // extern "C"
