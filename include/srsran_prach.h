/*
 * include/srsran_prach.h -- MI355X PRACH: preamble detection for the eNB and preamble generation for the
 * UE, preamble formats 0-3, as a C-ABI drop-in with the reference's names, argument meaning and return
 * codes.
 *
 * Replaces:
 *   srsran_prach_t, srsran_prach_cfg_t, srsran_prach_sf_config_t, srsran_prach_sfn_t and
 *   srsran_prach_init / set_cfg / gen / detect / detect_offset / set_detect_factor / free and the FDD
 *   occasion helpers                                   lib/include/srsran/phy/phch/prach.h:56-251
 *
 * Buffers of the reference's calls are host memory.  The transforms run on the GPU
 * (csrc/prach_kernel.hip): the 12 N-point spectrum of the received window as twelve N-point FFTs and a
 * 12-term combine of the 839 PRACH bins, one 839-point inverse DFT per root sequence, the windowed peak
 * search.  srsran_prach_gpu_detect_batch (added) runs many occasions of one or more cells in one launch
 * from device buffers.
 *
 * Not provided (srsran_prach_set_cfg returns SRSRAN_ERROR and says why): preamble format 4 (config_idx >= 48
 * of a TDD cell, 36.211 Table 5.7.1-3; for FDD 48..63 are format 3, as config_idx / 16 says), the high-speed
 * flag (restricted sets), successive cancellation (asked for with zero_corr_zone 0; with any other zone the
 * reference switches it off itself and so does this), the TDD
 * location helpers (srsran_prach_f_ra_tdd, f_id_tdd, nof_f_idx_tdd, tti_opportunity_config_tdd) and the
 * srsran_prach_nr_* tables.  Detection itself does not depend on the duplex mode; is_nr only moves the
 * first PRACH bin by half a data subcarrier.
 */
#ifndef SRSRAN_AMD_PRACH_H
#define SRSRAN_AMD_PRACH_H

#include <stdbool.h>
#include <stdint.h>

#include "srsran_ue_dl.h" /* cf_t, srsran_tdd_config_t, srsran_symbol_sz, srsran_nof_prb, SRSRAN_ERROR... */

#ifdef __cplusplus
extern "C" {
#endif

#define SRSRAN_PRACH_MAX_LEN (2 * 24576 + 21024) /* prach.h:42: maximum Tcp + Tseq */
#define SRSRAN_PRACH_N_ZC_LONG 839               /* prach.h:45 */

/* prach.h:62-122.  The parameter fields keep the reference's names and types; the FFTW plans, the scratch
 * pointers, the DFT-precoded sequences (device memory here) and the cancellation state are gone; gpu is added. */
typedef struct {
  /* parameters from higher layers (SIB2) */
  bool     is_nr;
  uint32_t config_idx;
  uint32_t f;            /* preamble format */
  uint32_t rsi;          /* rootSequenceIndex */
  bool     hs;           /* highSpeedFlag: always false */
  uint32_t zczc;         /* zeroCorrelationZoneConfig */
  uint32_t N_ifft_ul;    /* uplink symbol size */
  uint32_t N_ifft_prach; /* 12 * N_ifft_ul */
  uint32_t max_N_ifft_ul;

  /* working parameters */
  uint32_t N_zc;  /* 839 */
  uint32_t N_cs;  /* cyclic shift size */
  uint32_t N_seq; /* preamble length in samples */
  float    T_seq; /* preamble length in seconds */
  float    T_tot; /* cyclic prefix + preamble in seconds */
  uint32_t N_cp;  /* cyclic prefix length in samples */

  /* generated tables */
  cf_t     seqs[64][SRSRAN_PRACH_N_ZC_LONG]; /* the 64 preamble sequences */
  uint32_t root_seqs_idx[64];                /* index in seqs of every root sequence */
  uint32_t N_roots;                          /* root sequences of this configuration */

  float               detect_factor;
  uint32_t            deadzone; /* always 0, as prach.c:710 */
  uint32_t            num_ra_preambles;
  bool                successive_cancellation; /* always false */
  bool                freq_domain_offset_calc;
  srsran_tdd_config_t tdd_config;
  uint32_t            current_prach_idx;

  void* gpu; /* added: device tables, stream, the last detect's metrics */
} srsran_prach_t;

typedef struct {
  int      nof_sf;
  uint32_t sf[5];
} srsran_prach_sf_config_t;

typedef enum {
  SRSRAN_PRACH_SFN_EVEN = 0,
  SRSRAN_PRACH_SFN_ANY,
} srsran_prach_sfn_t;

/* prach.h:149-160 */
typedef struct {
  bool                is_nr;
  uint32_t            config_idx;
  uint32_t            root_seq_idx;
  uint32_t            zero_corr_zone;
  uint32_t            freq_offset;
  uint32_t            num_ra_preambles;
  bool                hs_flag;
  srsran_tdd_config_t tdd_config;
  bool                enable_successive_cancellation;
  bool                enable_freq_domain_offset_calc;
} srsran_prach_cfg_t;

/* host only (prach.c:108-186, 293): 36.211 Table 5.7.1-2 */
uint32_t           srsran_prach_get_preamble_format(uint32_t config_idx);
srsran_prach_sfn_t srsran_prach_get_sfn(uint32_t config_idx);
/* FDD objects only: with p->tdd_config.configured (or p->is_nr) this returns false, the TDD and NR occasion
 * tables are not provided */
bool srsran_prach_tti_opportunity(srsran_prach_t* p, uint32_t current_tti, int allowed_subframe);
bool srsran_prach_tti_opportunity_config_fdd(uint32_t config_idx, uint32_t current_tti, int allowed_subframe);
bool srsran_prach_in_window_config_fdd(uint32_t config_idx, uint32_t current_tti, int allowed_subframe);
void srsran_prach_sf_config(uint32_t config_idx, srsran_prach_sf_config_t* sf_config);

/* prach.c:553-617: max_N_ifft_ul <= 2048; SRSRAN_ERROR without a HIP device (no CPU fallback) */
int srsran_prach_init(srsran_prach_t* p, uint32_t max_N_ifft_ul);
/* prach.c:619-747: builds the 64 sequences (p->seqs) and their 839-point transforms (device) */
int srsran_prach_set_cfg(srsran_prach_t* p, srsran_prach_cfg_t* cfg, uint32_t nof_prb);
/* prach.c:749-793: signal receives N_cp + N_seq host samples */
int srsran_prach_gen(srsran_prach_t* p, uint32_t seq_index, uint32_t freq_offset, cf_t* signal);
/* prach.c:800-808, 969-1012: the first N_ifft_prach host samples of signal are used; a shorter sig_len returns
 * SRSRAN_ERROR_INVALID_INPUTS.  An index is root * n_wins + window and can exceed 63 (at most 110 entries are
 * written, zero_corr_zone 2).  6 + freq_offset above the cell's PRBs, where the reference reads outside its
 * spectrum, returns SRSRAN_ERROR_INVALID_INPUTS. */
int srsran_prach_detect(srsran_prach_t* p,
                        uint32_t        freq_offset,
                        cf_t*           signal,
                        uint32_t        sig_len,
                        uint32_t*       indices,
                        uint32_t*       ind_len);
int srsran_prach_detect_offset(srsran_prach_t* p,
                               uint32_t        freq_offset,
                               cf_t*           signal,
                               uint32_t        sig_len,
                               uint32_t*       indices,
                               float*          t_offsets,
                               float*          peak_to_avg,
                               uint32_t*       ind_len);
void srsran_prach_set_detect_factor(srsran_prach_t* p, float factor);
int  srsran_prach_free(srsran_prach_t* p);

/* ---- added: many PRACH occasions in one launch, signals on the device ----
 * Each entry names its own srsran_prach_t (cells and symbol sizes may differ), the frequency offset and a device
 * buffer of at least N_ifft_prach samples.  An invalid entry returns the code srsran_prach_detect_offset returns
 * for it before anything is launched or written to res.  res[i] lists the detections of entry i in the
 * reference's order (root, then window).  The work runs on the first entry's stream; the call returns when
 * the results are in res.  It also writes the metrics of every object it names: from the call until its return
 * no other thread may use any of those objects (detect, gen, set_cfg, get_metrics or another batch). */
#define SRSRAN_PRACH_GPU_MAX_DET 128
typedef struct {
  srsran_prach_t* prach;
  uint32_t        freq_offset;
  const cf_t*     d_signal; /* device */
  uint32_t        sig_len;
} srsran_prach_gpu_occ_t;
typedef struct {
  uint32_t nof_det;
  uint32_t indices[SRSRAN_PRACH_GPU_MAX_DET];
  float    t_offsets[SRSRAN_PRACH_GPU_MAX_DET];
  float    peak_to_avg[SRSRAN_PRACH_GPU_MAX_DET];
} srsran_prach_gpu_res_t;
int srsran_prach_gpu_detect_batch(uint32_t nof_occ, const srsran_prach_gpu_occ_t* occ, srsran_prach_gpu_res_t* res);
/* srsran_prach_gen with a device output buffer of N_cp + N_seq samples; returns once it is written */
int srsran_prach_gpu_gen(srsran_prach_t* p, uint32_t seq_index, uint32_t freq_offset, cf_t* d_signal);
/* the last detect on p (either entry point): peak / average and the peak's offset in its window for every
 * (root, window) searched, detected or not, at [root * nof_wins + window]; the arrays hold
 * SRSRAN_PRACH_GPU_MAX_DET entries.  SRSRAN_ERROR before the first detect. */
int srsran_prach_gpu_get_metrics(srsran_prach_t* p, float* ratio, uint32_t* offset, uint32_t* nof_roots, uint32_t* nof_wins);
/* measurement hook (tools/prach_bench.py): *device_us receives the time between two events recorded on p's stream
 * around the two kernels of the last detect that ran on it while the hook was enabled (a batch runs on its first
 * entry's object), -1 if there was none; then the hook is switched on or off for the detects that follow.  Off by
 * default: the events cost two more stream operations a call. */
int srsran_prach_gpu_detect_time(srsran_prach_t* p, bool enable, float* device_us);

#ifdef __cplusplus
}
#endif
#endif
