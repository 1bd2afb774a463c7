/*
 * include/srsran_ue_ul.h -- MI355X UE uplink transmit (PUSCH and PUCCH branches) as a C-ABI drop-in.
 *
 * Replaces, with the reference's names, argument meaning and return codes:
 *   srsran_ue_ul_powerctrl_t, srsran_ul_cfg_t, srsran_ue_ul_normalize_mode_t, srsran_ue_ul_cfg_t
 *                                            lib/include/srsran/phy/ue/ue_ul.h:49-92
 *   srsran_refsignal_srs_cfg_t               lib/include/srsran/phy/ch_estimation/refsignal_ul.h:53-70
 *   srsran_pusch_hopping_cfg_t               lib/include/srsran/phy/phch/pusch_cfg.h:35-42
 *   srsran_ue_ul_t, srsran_ue_ul_init / free / set_cell / encode, srsran_ue_ul_pucch_resource_selection,
 *   srsran_ue_ul_sr_send_tti, srsran_ue_ul_gen_sr
 *                                            lib/include/srsran/phy/ue/ue_ul.h:94-142, lib/src/phy/ue/ue_ul.c:41-175, 246-351,
 *                                            497-659
 *   srsran_uci_data_t                        lib/include/srsran/phy/phch/uci_cfg.h:61-64
 *   srsran_refsignal_srs_pucch_shortened (as _cfg, without the unused object)
 *                                            lib/src/phy/ch_estimation/refsignal_ul.c:625-642
 *   srsran_refsignal_srs_send_cs / _send_ue / _rb_start_cs / _rb_L_cs, and as _cell / _cfg (the cell in place of the
 *   srsran_refsignal_ul_t object) srsran_refsignal_srs_M_sc, _pusch_shortened, _srs_gen, _srs_put, _srs_get
 *                                            lib/src/phy/ch_estimation/refsignal_ul.c:560-622, 644-830, 870-924
 * with srsran_pusch_init_ue / srsran_pusch_encode / srsran_refsignal_dmrs_pusch_put_cell (srsran_pusch.h) and
 * srsran_ulsch_encode (srsran_sch.h) underneath.
 *
 * srsran_ue_ul_encode with a grant: the grid zeroed, srsran_pusch_encode, the DMRS put, SC-FDMA modulation
 * (freq_shift_f = 0.5, normalize = true, the cell's CP), apply_cfo, apply_norm -- all on the GPU
 * (csrc/pusch_tx_kernel.hip, csrc/ofdm_kernel.hip); q->out_buffer (host) receives the subframe's samples.
 * Without a grant and with UCI pending (or a scheduling request) on cc_idx 0: the PUCCH branch (ue_ul.c:510-558) --
 * format and resource selection on a copy of the UCI value (cfg->ul_cfg.pucch.format / n_pucch are written, data->uci
 * is not), sf->shortened by the shortened rule, then the grid zeroed, srsran_pucch_encode and the PUCCH DMRS in one
 * kernel (csrc/pucch_tx_kernel.hip), the same modulator, apply_cfo and apply_norm from (float)nof_prb / 15 / 10.
 * srsran_ue_ul_gpu_tx_batch (added) does the same for many UEs of one or more cells on device buffers.
 *
 * A subframe that carries the UE's own sounding reference signal (srs_tx_enabled, ue_ul.c:453-462: ul_cfg.srs
 * configured, a cell-specific and a UE-specific SRS subframe): with a grant or with PUCCH the SRS is added to the
 * comb of the last symbol after the channel and its DMRS (add_srs, ue_ul.c:301-311, whatever sf->shortened says);
 * without either, the SRS-only branch (srs_encode, ue_ul.c:435-451): the grid zeroed, the SRS, the same modulator,
 * apply_cfo and apply_norm from (float)nof_prb / 15 / sqrtf(M_sc).  The sequence is formed on the GPU
 * (csrc/srs_kernel.hip).  An SRS configuration that srsran_refsignal_srs_cfg_isvalid refuses is SRSRAN_ERROR in
 * such a subframe.  For PUSCH sf->shortened is the caller's (srsran_refsignal_srs_pusch_shortened_cfg computes it).
 *
 * Not provided (SRSRAN_ERROR with a message): srsran_ue_ul_pregen_signals, srsran_ue_ul_set_cfr, a grant whose
 * L_prb is not 2^a 3^b 5^c, filler bits.  srsran_ue_ul_dci_to_pusch_grant, srsran_ue_ul_pusch_hopping and the power
 * helpers are not declared: the caller supplies the grant with n_prb_tilde set, as for the receive side.
 */
#ifndef SRSRAN_AMD_UE_UL_H
#define SRSRAN_AMD_UE_UL_H

#include <stdbool.h>
#include <stdint.h>

#include "srsran_pucch.h"
#include "srsran_pusch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRSRAN_SF_LEN(symbol_sz) ((symbol_sz) * 15)                                /* phy_common.h:134 */
#define SRSRAN_SF_LEN_PRB(nof_prb) ((uint32_t)SRSRAN_SF_LEN(srsran_symbol_sz(nof_prb))) /* phy_common.h:138 */

/* srsran_refsignal_srs_cfg_t: srsran_pusch.h (the eNB's SRS estimator takes it too) */

/* PUSCH hopping configuration: data only (the caller computes n_prb_tilde) */
typedef struct {
  enum { SRSRAN_PUSCH_HOP_MODE_INTER_SF = 1, SRSRAN_PUSCH_HOP_MODE_INTRA_SF = 0 } hop_mode;
  uint32_t hopping_offset;
  uint32_t n_sb;
  uint32_t n_rb_ho;
  uint32_t current_tx_nb;
  bool     hopping_enabled;
} srsran_pusch_hopping_cfg_t;

/* UE UL power control: data only */
typedef struct {
  float p0_nominal_pusch;
  float alpha;
  float p0_nominal_pucch;
  float delta_f_pucch[5];
  float delta_preamble_msg3;
  float p0_ue_pusch;
  bool  delta_mcs_based;
  bool  acc_enabled;
  float p0_ue_pucch;
  float p_srs_offset;
} srsran_ue_ul_powerctrl_t;

typedef struct {
  srsran_pucch_cfg_t                pucch;
  srsran_pusch_cfg_t                pusch;
  srsran_pusch_hopping_cfg_t        hopping;
  srsran_ue_ul_powerctrl_t          power_ctrl;
  srsran_refsignal_dmrs_pusch_cfg_t dmrs;
  srsran_refsignal_srs_cfg_t        srs;
} srsran_ul_cfg_t;

typedef enum {
  SRSRAN_UE_UL_NORMALIZE_MODE_AUTO = 0,
  SRSRAN_UE_UL_NORMALIZE_MODE_FORCE_AMPLITUDE
} srsran_ue_ul_normalize_mode_t;

typedef struct {
  srsran_ul_cfg_t               ul_cfg;
  bool                          grant_available;
  uint32_t                      cc_idx;
  srsran_ue_ul_normalize_mode_t normalize_mode;
  float                         force_peak_amplitude;
  bool                          cfo_en;
  float                         cfo_tol; /* not used: every call rotates by cfo_value, as srsran_vec_apply_cfo */
  float                         cfo_value;
} srsran_ue_ul_cfg_t;

/* The object keeps the reference's members that this library has (ue_ul.h:94-118); the pregenerated signals, the
 * PUCCH object, the hopping sequence and the CFR configuration have no counterpart. */
typedef struct {
  srsran_cell_t  cell;
  bool           signals_pregenerated; /* always false */
  srsran_ofdm_t  fft;
  srsran_pusch_t pusch;
  cf_t*          out_buffer;
  void*          gpu; /* added: device grid / sample staging, the cell's DMRS hopping tables, the CFO table */
} srsran_ue_ul_t;

int  srsran_ue_ul_init(srsran_ue_ul_t* q, cf_t* out_buffer, uint32_t max_prb);
void srsran_ue_ul_free(srsran_ue_ul_t* q);
int  srsran_ue_ul_set_cell(srsran_ue_ul_t* q, srsran_cell_t cell);
/* not provided: SRSRAN_ERROR */
int srsran_ue_ul_set_cfr(srsran_ue_ul_t* q, const void* cfr);
int srsran_ue_ul_pregen_signals(srsran_ue_ul_t* q, srsran_ue_ul_cfg_t* cfg);

/* ue_ul.c:618-659 (grant, then PUCCH, then SRS, then nothing): 1 when a subframe was generated, 0 when there is nothing to send (out_buffer zeroed), -1 on
 * error.  data->ptr: the host payload. */
int srsran_ue_ul_encode(srsran_ue_ul_t* q, srsran_ul_sf_cfg_t* sf, srsran_ue_ul_cfg_t* cfg, srsran_pusch_data_t* data);

/* ---- host helpers of the PUCCH branch, value-exact (ue_ul.c:497-506, 561-614; refsignal_ul.c:625-642) ---- */
typedef struct {
  srsran_uci_cfg_t   cfg;
  srsran_uci_value_t value;
} srsran_uci_data_t;

/* writes cfg->format and cfg->n_pucch; b: b(0) b(1) of format 1b with channel selection */
void srsran_ue_ul_pucch_resource_selection(const srsran_cell_t*      cell,
                                           srsran_pucch_cfg_t*       cfg,
                                           const srsran_uci_cfg_t*   uci_cfg,
                                           const srsran_uci_value_t* uci_value,
                                           uint8_t                   b[SRSRAN_UCI_MAX_ACK_BITS]);
/* 1 when current_tti is an SR opportunity of cfg->I_sr (36.213 Table 10.1.5-1), 0 when not or when no SR is
 * configured, -1 for I_sr > 157 */
int  srsran_ue_ul_sr_send_tti(const srsran_pucch_cfg_t* cfg, uint32_t current_tti);
bool srsran_ue_ul_gen_sr(srsran_ue_ul_cfg_t* cfg, srsran_ul_sf_cfg_t* sf, srsran_uci_data_t* uci_data, bool sr_request);
/* writes sf->shortened: format 1x in a cell SRS subframe with srs_cfg->configured and simul_ack */
void srsran_refsignal_srs_pucch_shortened_cfg(srsran_ul_sf_cfg_t*         sf,
                                              srsran_refsignal_srs_cfg_t* srs_cfg,
                                              srsran_pucch_cfg_t*         pucch_cfg);

/* ---- host helpers of the sounding reference signal, value-exact (refsignal_ul.c:560-622, 644-830, 870-924) ---- */
/* added: what every entry point checks before it touches a grid: bw_cfg < 8, B < 4, b_hop < 4, k_tc < 2, n_srs < 8,
 * n_rrc < 24, subframe_config < 15, I_srs < 637 and m_SRS,0 of the cell's bandwidth table <= nof_prb (the reference
 * computes nof_prb / 2 - m_SRS,0 / 2 unsigned and writes outside its grid where that fails) */
bool srsran_refsignal_srs_cfg_isvalid(const srsran_refsignal_srs_cfg_t* cfg, uint32_t nof_prb);
/* 1: an SRS subframe, 0: not, SRSRAN_ERROR_INVALID_INPUTS out of range (FDD tables only, as the reference) */
int srsran_refsignal_srs_send_cs(uint32_t subframe_config, uint32_t sf_idx);
int srsran_refsignal_srs_send_ue(uint32_t I_srs, uint32_t tti);
/* the cell-specific SRS region in PRB (the reference's unsigned arithmetic, also where m_SRS,0 > nof_prb) */
uint32_t srsran_refsignal_srs_rb_start_cs(uint32_t bw_cfg, uint32_t nof_prb);
uint32_t srsran_refsignal_srs_rb_L_cs(uint32_t bw_cfg, uint32_t nof_prb);
/* M_sc,b = m_SRS,B 12 / 2, and k0 of the subframe with frequency hopping (the reference's static srs_k0_ue); 0 for a
 * configuration that is not valid */
uint32_t srsran_refsignal_srs_M_sc_cell(const srsran_cell_t* cell, const srsran_refsignal_srs_cfg_t* cfg);
uint32_t srsran_refsignal_srs_k0_cell(const srsran_cell_t* cell, const srsran_refsignal_srs_cfg_t* cfg, uint32_t tti);
/* writes sf->shortened: never for a RAR grant; in the UE's own SRS subframes unless the allocation is contiguous to
 * the cell's SRS region; in the cell's SRS subframes where the allocation overlaps that region */
void srsran_refsignal_srs_pusch_shortened_cfg(const srsran_cell_t*        cell,
                                              srsran_ul_sf_cfg_t*         sf,
                                              srsran_refsignal_srs_cfg_t* srs_cfg,
                                              srsran_pusch_cfg_t*         pusch_cfg);
/* r_srs: 2 M_sc values, the sequences of slots 2 sf_idx and 2 sf_idx + 1 (put / get use the first M_sc only, as the
 * reference: with group or sequence hopping the SRS carries the sequence of slot 2 sf_idx).  sf_symbols: the
 * subframe grid.  SRSRAN_ERROR_INVALID_INPUTS for a configuration that is not valid. */
int srsran_refsignal_srs_gen_cell(const srsran_cell_t*               cell,
                                  srsran_refsignal_srs_cfg_t*        cfg,
                                  srsran_refsignal_dmrs_pusch_cfg_t* pusch_cfg,
                                  uint32_t                           sf_idx,
                                  cf_t*                              r_srs);
int srsran_refsignal_srs_put_cell(const srsran_cell_t*        cell,
                                  srsran_refsignal_srs_cfg_t* cfg,
                                  uint32_t                    tti,
                                  cf_t*                       r_srs,
                                  cf_t*                       sf_symbols);
int srsran_refsignal_srs_get_cell(const srsran_cell_t*        cell,
                                  srsran_refsignal_srs_cfg_t* cfg,
                                  uint32_t                    tti,
                                  cf_t*                       r_srs,
                                  cf_t*                       sf_symbols);

/* ---- added: many UE subframes of one or more cells, asynchronous on `stream` ----
 * Every stage (TB CRC, code blocks, multiplexing + scrambling + mapping, transform precoding + DMRS, normalisation)
 * is one launch over all entries; the OFDM modulation is one launch pair per cell object, the CFO product one launch
 * per entry that enables it.  Results are bit-identical to single-entry calls in any order and composition.
 * The transmit scratch of entries[0].q serves the whole batch, and every object keeps device state between calls (its
 * grids, samples and the CFO phasor table): use one stream per object, one batch at a time, in stream order.  The
 * descriptors are uploaded from pageable host memory, so the call returns once they are staged, not before.
 * cfg->ul_cfg.pusch is updated as srsran_pusch_encode updates it.
 * An entry without grant_available is a PUCCH entry under srsran_ue_ul_encode's conditions (uci == NULL: an all-zero
 * value; d_data is ignored): all of them go through one PUCCH launch and share the modulator and normalisation
 * launches with the PUSCH entries; cfg->ul_cfg.pucch.format / n_pucch / pucch2_drs_bits and sf->shortened are written.
 * An entry whose subframe carries the UE's SRS gets the SRS on its grid after its channel; all of them, and the
 * entries with the SRS alone, go through one SRS launch after the PUSCH and PUCCH launches and share the modulator
 * and normalisation launches.
 * An entry with nothing to send gets zeroed d_out / d_grid and is not an error. */
typedef struct {
  srsran_ue_ul_t*           q;      /* the entry's cell (srsran_ue_ul_set_cell done) */
  srsran_ul_sf_cfg_t*       sf;
  srsran_ue_ul_cfg_t*       cfg;
  const srsran_uci_value_t* uci;    /* may be NULL without UCI */
  const uint8_t*            d_data; /* device payload, tbs / 8 bytes (may be NULL with tbs == 0) */
  cf_t*                     d_out;  /* device, SRSRAN_SF_LEN_PRB(cell.nof_prb) samples; NULL: grid only */
  cf_t*                     d_grid; /* device, optional: the subframe grid, 2 N_symb x 12 nof_prb REs */
} srsran_ue_ul_gpu_entry_t;

int srsran_ue_ul_gpu_tx_batch(uint32_t nof_ue, const srsran_ue_ul_gpu_entry_t* entries, void* stream);

/* added, read-only: device pointers to the last encode on this object (the last batch entry naming it): the packed
 * scrambled bits (nof_bits / 8 bytes), the modulation symbols (nof_re) and the subframe grid (nof_grid REs); after a
 * PUCCH or an SRS-only subframe the grid alone, with nof_bits = nof_re = 0.
 * Valid until the next encode on the object or on the object whose scratch served the batch; SRSRAN_ERROR before
 * the first. */
int srsran_ue_ul_gpu_last(srsran_ue_ul_t* q,
                          const uint8_t** d_scrambled,
                          uint32_t*       nof_bits,
                          const cf_t**    d_symbols,
                          uint32_t*       nof_re,
                          const cf_t**    d_grid,
                          uint32_t*       nof_grid);

#ifdef __cplusplus
}
#endif
#endif
