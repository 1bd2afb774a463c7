/*
 * include/srsran_phich.h -- PHICH (HARQ indicator) of the MI355X PHY: transmit for the eNB, decode for the UE.
 *
 * Drop-in for lib/include/srsran/phy/phch/phich.h:43-125 (phich.c): the resource / grant / result types, the
 * SRSRAN_PHICH_* constants and the srsran_phich_* functions with the reference's names, arguments and return
 * conventions; srsran_phich_t keeps the fields a caller reads (cell, nof_rx_antennas, regs), its buffers live on
 * the device behind `gpu`.  Also srsran_enb_dl_put_phich's counterpart for the UE, srsran_ue_dl_decode_phich
 * (ue/ue_dl.h, ue_dl.c:716-746).
 *
 * GPU work (phich_kernel.hip):
 *   transmit: one 64-lane workgroup per (subframe, mapping unit); a lane owns one RE of one port, sums the
 *     unit's items in the order they were put (3 x repetition, BPSK, Table 6.9.1-2 spreading, scrambling, the
 *     extended-CP half, layer mapping + transmit diversity as srsran_precoding_diversity for 1 / 2 / 4 ports)
 *     and stores once;
 *   receive: one wave per item: RE gather of every rx antenna and estimate, srsran_predecoding_single_multi
 *     (1 port) or srsran_predecoding_diversity_multi + srsran_layerdemap_diversity (2 / 4 ports), descrambling,
 *     de-spreading, BPSK soft demapping and srsran_phich_ack_decode's rule, with fixed summation order.
 * Four-port PHICH uses the ordinary SFBC + FSTD precoder as the reference does (phich.c:410), not 36.211 6.9.2.
 */
#ifndef SRSRAN_AMD_PHICH_H
#define SRSRAN_AMD_PHICH_H

#include "srsran_pdcch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRSRAN_PHICH_NORM_NSEQUENCES 8
#define SRSRAN_PHICH_EXT_NSEQUENCES 4
#define SRSRAN_PHICH_NBITS 3
#define SRSRAN_PHICH_NORM_MSYMB (SRSRAN_PHICH_NBITS * 4)
#define SRSRAN_PHICH_EXT_MSYMB (SRSRAN_PHICH_NBITS * 2)
#define SRSRAN_PHICH_MAX_NSYMB SRSRAN_PHICH_NORM_MSYMB
#define SRSRAN_PHICH_NORM_C 1
#define SRSRAN_PHICH_EXT_C 2
#define SRSRAN_PHICH_NORM_NSF 4
#define SRSRAN_PHICH_EXT_NSF 2

typedef struct {
  srsran_cell_t  cell;
  uint32_t       nof_rx_antennas;
  srsran_regs_t* regs;
  void*          gpu; /* added: device RE table, scratch grids, stream */
} srsran_phich_t;

typedef struct {
  uint32_t ngroup;
  uint32_t nseq;
} srsran_phich_resource_t;

typedef struct {
  uint32_t n_prb_lowest;
  uint32_t n_dmrs;
  uint32_t I_phich;
} srsran_phich_grant_t;

typedef struct {
  bool  ack_value;
  float distance;
} srsran_phich_res_t;

int  srsran_phich_init(srsran_phich_t* q, uint32_t nof_rx_antennas); /* 1..4 rx antennas */
void srsran_phich_free(srsran_phich_t* q);
int  srsran_phich_set_cell(srsran_phich_t* q, srsran_regs_t* regs, srsran_cell_t cell);
/* The REG tables the next calls use (their PHICH RE table is copied to the device). */
void srsran_phich_set_regs(srsran_phich_t* q, srsran_regs_t* regs);
/* 36.213 9.1.2 (phich.c:131-142): n_group / n_seq of an uplink grant. */
void srsran_phich_calc(srsran_phich_t* q, srsran_phich_grant_t* grant, srsran_phich_resource_t* n_phich);
/* The reference's group count: the mapping units of q->regs, x 2 with the extended CP (regs.c:351-353). */
uint32_t srsran_phich_ngroups(srsran_phich_t* q);
uint32_t srsran_phich_nsf(srsran_phich_t* q);
/* Zeroes the REs of every mapping unit in the host grids (srsran_regs_phich_reset on every non-NULL port). */
void    srsran_phich_reset(srsran_phich_t* q, cf_t* slot_symbols[SRSRAN_MAX_PORTS]);
void    srsran_phich_ack_encode(uint8_t ack, uint8_t bits[SRSRAN_PHICH_NBITS]);
uint8_t srsran_phich_ack_decode(float bits[SRSRAN_PHICH_NBITS], float* distance);
/* Host-synchronous.  encode adds the precoded symbols into the host grids sf_symbols[0..nof_ports) as
 * srsran_regs_phich_add does; decode reads nof_rx host grids and the full-grid host estimates channel->ce.
 * SRSRAN_ERROR_INVALID_INPUTS for an nseq / ngroup out of range (phich.c:198-212, 326-340), nothing written. */
int srsran_phich_encode(srsran_phich_t* q, srsran_dl_sf_cfg_t* sf, srsran_phich_resource_t n_phich, uint8_t ack,
                        cf_t* sf_symbols[SRSRAN_MAX_PORTS]);
int srsran_phich_decode(srsran_phich_t* q, srsran_dl_sf_cfg_t* sf, srsran_chest_dl_res_t* channel,
                        srsran_phich_resource_t n_phich, cf_t* sf_symbols[SRSRAN_MAX_PORTS], srsran_phich_res_t* result);

/* ---------------- added: batches on device buffers, asynchronous on `stream` ---------------- */
typedef struct {
  uint32_t                sf;  /* index of the subframe in the device grids */
  uint32_t                tti; /* tti % 10 selects the scrambling sequence */
  srsran_phich_resource_t n_phich;
  uint8_t                 ack; /* encode only */
} srsran_phich_gpu_item_t;

typedef struct {
  uint32_t ack_value;
  float    distance;
} srsran_phich_gpu_res_t;

/* d_grids: [nof_sf][cell.nof_ports][2 nsymb][12 nof_prb] cf_t (srsran_enb_dl_gpu_sf_symbols' layout).  The REs
 * of every mapping unit that has an item are overwritten with the sum of that unit's items in item order, which
 * on a cleared grid is what consecutive srsran_phich_encode calls leave; other REs are not touched.  One launch.
 * Every item is validated first: SRSRAN_ERROR_INVALID_INPUTS and nothing enqueued if one is out of range. */
int srsran_phich_gpu_encode_batch(srsran_phich_t* q, uint32_t nof_items, const srsran_phich_gpu_item_t* items,
                                  uint32_t nof_sf, cf_t* d_grids, void* stream);
/* d_grids: [nof_sf][nof_rx][2 nsymb][12 nof_prb]; d_ce: [nof_sf][port][rx][ce_row_len], read at grid index modulo
 * ce_row_len (srsran_ue_dl_gpu_last_ce's two forms); the noise estimate of subframe s is d_noise[s * noise_stride].
 * d_out[i]: item i's {ack_value, distance} as srsran_phich_decode gives them.  One launch. */
int srsran_phich_gpu_decode_batch(srsran_phich_t* q, uint32_t nof_items, const srsran_phich_gpu_item_t* items,
                                  uint32_t nof_sf, const cf_t* d_grids, const cf_t* d_ce, uint32_t ce_row_len,
                                  const float* d_noise, uint32_t noise_stride, srsran_phich_gpu_res_t* d_out,
                                  void* stream);

/* ---------------- ue_dl.h ---------------- */
/* ue_dl.c:716-746: selects the REG tables of the subframe's m_i (as the PDCCH search does), srsran_phich_calc,
 * then srsran_phich_decode on the grids and estimates srsran_ue_dl_decode_fft_estimate left.  0, or -1 on error. */
int srsran_ue_dl_decode_phich(srsran_ue_dl_t* q, srsran_dl_sf_cfg_t* sf, srsran_ue_dl_cfg_t* cfg,
                              srsran_phich_grant_t* grant, srsran_phich_res_t* result);

#ifdef __cplusplus
}
#endif
#endif /* SRSRAN_AMD_PHICH_H */
