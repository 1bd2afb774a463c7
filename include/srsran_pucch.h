/*
 * include/srsran_pucch.h -- MI355X PUCCH receive (eNB side) and transmit (UE side): formats
 * 1/1a/1b/2/2a/2b/3, as a C-ABI drop-in with the reference's names, argument meaning, return codes
 * and write-backs.
 *
 * Replaces:
 *   srsran_pucch_format_t, srsran_pucch_cfg_t          lib/include/srsran/phy/phch/pucch_cfg.h:29-88
 *   srsran_ack_nack_feedback_mode_t                    lib/include/srsran/phy/common/phy_common.h:313-318
 *   srsran_pucch_t, srsran_pucch_res_t, srsran_pucch_init_enb / init_ue / free / set_cell / decode /
 *   encode and the resource helpers                    lib/include/srsran/phy/phch/pucch.h:42-184
 *   srsran_pucch_proc_select_format / get_resources / get_npucch, srsran_pucch_cs_get_ack
 *                                                      lib/include/srsran/phy/phch/pucch_proc.h
 *   srsran_refsignal_dmrs_N_rs / dmrs_pucch_symbol / dmrs_pucch_gen / dmrs_pucch_put (the last two in
 *   a _cell form: there is no srsran_refsignal_ul_t)   lib/include/srsran/phy/ch_estimation/refsignal_ul.h
 *   srsran_chest_ul_estimate_pucch                     lib/include/srsran/phy/ch_estimation/chest_ul.h:127-131
 *
 * Buffers of the reference's calls are host memory (subframe grids of nof_prb * 12 * 2 * N_symb(cp)
 * REs).  Everything per RE runs on the GPU (csrc/pucch_kernel.hip): the DMRS / data gather, least
 * squares with the 2a / 2b DMRS hypotheses, EPRE / RSRP / TA / noise, the equaliser, DMRS detection
 * and the per-format decoders.  srsran_pucch_gpu_get_batch (added) does what srsran_enb_ul_get_pucch
 * does (enb_ul.c:156-273) for many UEs of one or more cells in one launch, from device grids.
 * The UE side (csrc/pucch_tx_kernel.hip) forms every RE of a transmission on the GPU from the coded
 * bits: modulation, sequences, covers, the format 3 spreading and DFT, the DMRS; srsran_ue_ul_encode
 * and srsran_ue_ul_gpu_tx_batch (srsran_ue_ul.h) run it for whole subframes.
 * Not provided: the Cedron TA estimator, SRS.
 */
#ifndef SRSRAN_AMD_PUCCH_H
#define SRSRAN_AMD_PUCCH_H

#include <stdbool.h>
#include <stdint.h>

#include "srsran_pusch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRSRAN_PUCCH_SIZE_AN_CS 4                 /* pucch_cfg.h:29 */
#define SRSRAN_PUCCH_SIZE_AN_N3 4                 /* pucch_cfg.h:30 */
#define SRSRAN_PUCCH_NOF_AN_CS 2                  /* pucch_cfg.h:31 */
#define SRSRAN_PUCCH_MAX_BITS SRSRAN_CQI_MAX_BITS /* pucch_cfg.h:32 */
#define SRSRAN_NOF_SLOTS_PER_SF 2                 /* phy_common.h:53 */
#define SRSRAN_UCI_CQI_CODED_PUCCH_B 20           /* uci.h:42 */
#define SRSRAN_UCI_MAX_CQI_LEN_PUCCH 13           /* uci.h:41 */
#define SRSRAN_UCI_MAX_ACK_SR_BITS (SRSRAN_UCI_MAX_ACK_BITS + 1) /* uci_cfg.h:28 */

#define SRSRAN_PUCCH_N_SEQ SRSRAN_NRE
#define SRSRAN_PUCCH2_NOF_BITS SRSRAN_UCI_CQI_CODED_PUCCH_B
#define SRSRAN_PUCCH2_N_SF (5)
#define SRSRAN_PUCCH_1A_2A_NOF_ACK (1)
#define SRSRAN_PUCCH_1B_2B_NOF_ACK (2)
#define SRSRAN_PUCCH3_NOF_BITS (4 * SRSRAN_NRE)
#define SRSRAN_PUCCH_MAX_SYMBOLS (SRSRAN_PUCCH_N_SEQ * SRSRAN_PUCCH2_N_SF * SRSRAN_NOF_SLOTS_PER_SF)

#define SRSRAN_PUCCH_CS_MAX_ACK 4
#define SRSRAN_PUCCH_CS_MAX_CARRIERS 2
#define SRSRAN_PUCCH_FORMAT3_MAX_CARRIERS 5
#define SRSRAN_PUCCH_MAX_ALLOC 4 /* pucch_proc.h:33 */

#define SRSRAN_PUCCH_DEFAULT_THRESHOLD_FORMAT1 (0.5f)
#define SRSRAN_PUCCH_DEFAULT_THRESHOLD_FORMAT1A (0.5f)
#define SRSRAN_PUCCH_DEFAULT_THRESHOLD_FORMAT2 (0.5f)
#define SRSRAN_PUCCH_DEFAULT_THRESHOLD_FORMAT3 (0.5f)
#define SRSRAN_PUCCH_DEFAULT_THRESHOLD_DMRS (0.4f)

typedef enum {
  SRSRAN_PUCCH_FORMAT_1 = 0,
  SRSRAN_PUCCH_FORMAT_1A,
  SRSRAN_PUCCH_FORMAT_1B,
  SRSRAN_PUCCH_FORMAT_2,
  SRSRAN_PUCCH_FORMAT_2A,
  SRSRAN_PUCCH_FORMAT_2B,
  SRSRAN_PUCCH_FORMAT_3,
  SRSRAN_PUCCH_FORMAT_ERROR
} srsran_pucch_format_t;

typedef enum {
  SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_NORMAL = 0, /* no channel selection, no format 3 */
  SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_CS,
  SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_PUCCH3,
  SRSRAN_PUCCH_ACK_NACK_FEEDBACK_MODE_ERROR
} srsran_ack_nack_feedback_mode_t;

typedef struct {
  /* input configuration for this subframe */
  uint16_t         rnti;
  srsran_uci_cfg_t uci_cfg;

  /* common configuration */
  uint32_t delta_pucch_shift;
  uint32_t n_rb_2;
  uint32_t N_cs;
  uint32_t N_pucch_1;
  bool     group_hopping_en;

  /* dedicated configuration */
  uint32_t I_sr;
  bool     sr_configured;
  uint32_t n_pucch_1[4];
  uint32_t n_pucch_2;
  uint32_t n_pucch_sr;
  bool     simul_cqi_ack;
  bool     tdd_ack_multiplex;
  bool     sps_enabled;

  /* release 10 CA */
  srsran_ack_nack_feedback_mode_t ack_nack_feedback_mode;
  uint32_t                        n1_pucch_an_cs[SRSRAN_PUCCH_SIZE_AN_CS][SRSRAN_PUCCH_NOF_AN_CS];
  uint32_t                        n3_pucch_an_list[SRSRAN_PUCCH_SIZE_AN_N3];

  /* other configuration */
  float threshold_format1;
  float threshold_data_valid_format1a;
  float threshold_data_valid_format2;
  float threshold_data_valid_format3;
  float threshold_dmrs_detection;
  bool  meas_ta_en;
  bool  use_cedron_alg; /* with meas_ta_en: not provided, SRSRAN_ERROR */

  /* written during a call */
  srsran_pucch_format_t format;
  uint16_t              n_pucch;
  uint8_t               pucch2_drs_bits[SRSRAN_PUCCH_MAX_BITS];
} srsran_pucch_cfg_t;

typedef struct {
  srsran_cell_t cell;
  bool          is_ue;
  uint32_t      n_cs_cell[SRSRAN_NSLOTS_X_FRAME][SRSRAN_CP_NORM_NSYMB];
  uint32_t      f_gh[SRSRAN_NSLOTS_X_FRAME];
  void*         gpu; /* added: stream, descriptor / result / grid buffers, per-cell tables of the batch */
} srsran_pucch_t;

typedef struct {
  srsran_uci_value_t uci_data;
  float              dmrs_correlation;
  float              snr_db;
  float              rssi_dbFs;
  float              ni_dbFs;
  float              correlation;
  bool               detected;
  bool               ta_valid;
  float              ta_us;
} srsran_pucch_res_t;

/* ---- host helpers, value-exact (pucch.c:943-1264, pucch_proc.c, refsignal_ul.c:360-429) ---- */
uint32_t srsran_pucch_n_prb(const srsran_cell_t* cell, const srsran_pucch_cfg_t* cfg, uint32_t ns);
uint32_t srsran_pucch_m(const srsran_pucch_cfg_t* cfg, srsran_cp_t cp);
int      srsran_pucch_n_cs_cell(srsran_cell_t cell, uint32_t n_cs_cell[SRSRAN_NSLOTS_X_FRAME][SRSRAN_CP_NORM_NSYMB]);
float    srsran_pucch_alpha_format1(const uint32_t            n_cs_cell[SRSRAN_NSLOTS_X_FRAME][SRSRAN_CP_NORM_NSYMB],
                                    const srsran_pucch_cfg_t* cfg,
                                    srsran_cp_t               cp,
                                    bool                      is_dmrs,
                                    uint32_t                  ns,
                                    uint32_t                  l,
                                    uint32_t*                 n_oc,
                                    uint32_t*                 n_prime_ns);
float    srsran_pucch_alpha_format2(const uint32_t            n_cs_cell[SRSRAN_NSLOTS_X_FRAME][SRSRAN_CP_NORM_NSYMB],
                                    const srsran_pucch_cfg_t* cfg,
                                    uint32_t                  ns,
                                    uint32_t                  l);
int      srsran_pucch_format2ab_mod_bits(srsran_pucch_format_t format, uint8_t bits[2], cf_t* d_10);
uint32_t srsran_pucch_nof_ack_format(srsran_pucch_format_t format);
bool     srsran_pucch_cfg_isvalid(srsran_pucch_cfg_t* cfg, uint32_t nof_prb);
int      srsran_pucch_cfg_assert(const srsran_cell_t* cell, const srsran_pucch_cfg_t* cfg);
int   srsran_pucch_collision(const srsran_cell_t* cell, const srsran_pucch_cfg_t* cfg1, const srsran_pucch_cfg_t* cfg2);
char* srsran_pucch_format_text(srsran_pucch_format_t format);
char* srsran_pucch_format_text_short(srsran_pucch_format_t format);
srsran_pucch_format_t srsran_pucch_proc_select_format(const srsran_cell_t*      cell,
                                                      const srsran_pucch_cfg_t* cfg,
                                                      const srsran_uci_cfg_t*   uci_cfg,
                                                      const srsran_uci_value_t* uci_value);
int srsran_pucch_proc_get_resources(const srsran_cell_t*      cell,
                                    const srsran_pucch_cfg_t* cfg,
                                    const srsran_uci_cfg_t*   uci_cfg,
                                    const srsran_uci_value_t* uci_value,
                                    uint32_t*                 n_pucch_i);
/* the UE's choice of resource and b(0) b(1) (format 1b with channel selection); 0 in a TDD cell, as the reference */
uint32_t srsran_pucch_proc_get_npucch(const srsran_cell_t*      cell,
                                      const srsran_pucch_cfg_t* cfg,
                                      const srsran_uci_cfg_t*   uci_cfg,
                                      const srsran_uci_value_t* uci_value,
                                      uint8_t                   b[SRSRAN_UCI_MAX_ACK_BITS]);
int srsran_pucch_cs_get_ack(const srsran_pucch_cfg_t* cfg,
                            const srsran_uci_cfg_t*   uci_cfg,
                            uint32_t                  j,
                            const uint8_t             b[2],
                            srsran_uci_value_t*       uci_value);
uint32_t srsran_refsignal_dmrs_N_rs(srsran_pucch_format_t format, srsran_cp_t cp);
uint32_t srsran_refsignal_dmrs_pucch_symbol(uint32_t m, srsran_pucch_format_t format, srsran_cp_t cp);

/* ---- host-synchronous receive, host buffers (pucch.c:48-132, 797-872; chest_ul.c:462-610) ---- */
int  srsran_pucch_init_enb(srsran_pucch_t* q);
void srsran_pucch_free(srsran_pucch_t* q);
int  srsran_pucch_set_cell(srsran_pucch_t* q, srsran_cell_t cell);
/* Writes cfg->pucch2_drs_bits for 2a / 2b, ce in both slots' PRBs over all symbols, epre, rsrp,
 * noise_estimate, snr, their dB forms and (meas_ta_en) ta_us.  cfg->use_cedron_alg with
 * cfg->meas_ta_en is not provided (FFTW-based in the reference): SRSRAN_ERROR. */
int srsran_chest_ul_estimate_pucch(srsran_chest_ul_t*     q,
                                   srsran_ul_sf_cfg_t*    sf,
                                   srsran_pucch_cfg_t*    cfg,
                                   cf_t*                  input,
                                   srsran_chest_ul_res_t* res);
int srsran_pucch_decode(srsran_pucch_t*        q,
                        srsran_ul_sf_cfg_t*    sf,
                        srsran_pucch_cfg_t*    cfg,
                        srsran_chest_ul_res_t* channel,
                        cf_t*                  sf_symbols,
                        srsran_pucch_res_t*    data);

/* ---- transmit, UE side (pucch.c:83, 768-794; refsignal_ul.c:432-552) ---- */
int srsran_pucch_init_ue(srsran_pucch_t* q);
/* Host grid in and out: only the data REs of cfg->format / cfg->n_pucch are written, the rest of sf_symbols is
 * left as it is.  Writes cfg->pucch2_drs_bits for 2a / 2b.  SRSRAN_ERROR for a PRB outside the cell or an
 * unsupported format, SRSRAN_ERROR_INVALID_INPUTS for NULL. */
int srsran_pucch_encode(srsran_pucch_t*     q,
                        srsran_ul_sf_cfg_t* sf,
                        srsran_pucch_cfg_t* cfg,
                        srsran_uci_value_t* uci_data,
                        cf_t*               sf_symbols);
/* r_pucch: 2 * N_rs * 12 values, [(slot * N_rs + m) * 12 + n]; d(10) of 2a / 2b from cfg->pucch2_drs_bits */
int srsran_refsignal_dmrs_pucch_gen_cell(const srsran_cell_t* cell,
                                         srsran_ul_sf_cfg_t*  sf,
                                         srsran_pucch_cfg_t*  cfg,
                                         cf_t*                r_pucch);
int srsran_refsignal_dmrs_pucch_put_cell(const srsran_cell_t* cell, srsran_pucch_cfg_t* cfg, cf_t* r_pucch, cf_t* output);

/* ---- added: srsran_enb_ul_get_pucch for many UEs in one launch ----
 * Per entry: the cell's chest object (cell, smoothing filter), the subframe, the PUCCH configuration
 * and the device subframe grid of that cell.  Each entry gets the full sequence of enb_ul.c:233-273:
 * CQI drop on collision with ACK, format selection, candidate resources, estimate + decode per
 * candidate, channel-selection mapping, the first-or-strictly-greater pick, the TA / SNR / RSSI / NI
 * copies and the second pass without SR.  cfg keeps what the reference leaves in it (format, n_pucch,
 * pucch2_drs_bits[0..1], uci_cfg.is_scheduling_request_tti, uci_cfg.cqi.data_enable); results go to
 * host res[i].  Returns SRSRAN_SUCCESS when every entry ran; an invalid entry returns the
 * reference's error code before anything is launched or written to res. */
typedef struct {
  srsran_chest_ul_t*  chest;
  srsran_ul_sf_cfg_t* sf;
  srsran_pucch_cfg_t* cfg;
  const cf_t*         d_sf_symbols; /* device */
} srsran_pucch_gpu_ue_t;

int srsran_pucch_gpu_get_batch(srsran_pucch_t*              q,
                               uint32_t                     nof_ue,
                               const srsran_pucch_gpu_ue_t* ues,
                               srsran_pucch_res_t*          res);

#ifdef __cplusplus
}
#endif
#endif
