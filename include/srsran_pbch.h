/*
 * include/srsran_pbch.h -- PBCH receive and the UE's MIB decoder on the MI355X PHY: an aligned subframe 0 goes in,
 * a MIB comes out.
 *
 * Drop-in for lib/include/srsran/phy/phch/pbch.h (pbch.c:136-553, the receiver) and lib/include/srsran/phy/ue/ue_mib.h
 * (ue_mib.c:36-172): the reference's names, arguments and return conventions; the structs keep the fields a caller
 * reads, their buffers live on the device behind `gpu`.  srsran_pbch_mib_pack stays declared in srsran_enb_dl.h, next
 * to the transmitter that uses it.
 *
 * GPU work (pbch_kernel.hip), three launches for any number of objects:
 *   LLR stage: one workgroup per (object, port-count hypothesis): RE gather of slot 1 (srsran_pbch_cp), predecoding
 *     for 1 / 2 / 4 ports on rx antenna 0, QPSK soft demapping;
 *   hypothesis stage: one 64-lane workgroup per (object, port count, frames combined, position in the 40 ms period,
 *     first stored frame) -- up to 30 per port count, 90 with nof_ports = 0, which the reference runs one after the
 *     other: descrambling, srsran_rm_conv_rx, the 16-bit tail-biting Viterbi decoder with lane = trellis state,
 *     CRC16 under the port mask;
 *   selection stage: the first accepted hypothesis in the reference's order, and the object's history.
 *
 * State.  Each object's LLR history (4 x 2 nof_symbols floats) and its frame counter live on the device, so that a
 * batch stays asynchronous.  q->frame_idx (and srsran_ue_mib_t's frame_cnt) is the host mirror of the device counter:
 * the synchronous calls below write it before they return; after a batch it is brought up to date, once the caller has
 * synchronised the batch's stream, by srsran_pbch_gpu_last_llr / srsran_ue_mib_gpu_sync or by the next synchronous
 * call on the object.  A caller must not run a synchronous call on an object while a batch that names it is in flight.
 *
 * Still refused, because it needs synchronisation: PSS / SSS, srsran_sync_*, srsran_ue_sync_*, srsran_ue_mib_sync_*
 * and srsran_ue_cell_search_*; also srsran_pbch_encode as a stand-alone call (the transmitter is srsran_enb_dl's),
 * NB-IoT, sidelink and NR PBCH.
 */
#ifndef SRSRAN_AMD_PBCH_H
#define SRSRAN_AMD_PBCH_H

#include "srsran_ue_dl.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRSRAN_BCH_PAYLOAD_LEN 24
#define SRSRAN_BCH_PAYLOADCRC_LEN (SRSRAN_BCH_PAYLOAD_LEN + 16)
#define SRSRAN_BCH_ENCODED_LEN (3 * (SRSRAN_BCH_PAYLOADCRC_LEN))

typedef struct {
  srsran_cell_t cell;        /* nof_ports = 4 when every port count is searched */
  uint32_t      nof_symbols; /* 240, or 216 with the extended CP */
  uint32_t      frame_idx;   /* stored frames: host mirror of the device counter (see above) */
  bool          search_all_ports;
  void*         gpu; /* added: RE table, sequence, LLR history, counters, scratch, stream */
} srsran_pbch_t;

/* SRSRAN_ERROR without a HIP device. */
int  srsran_pbch_init(srsran_pbch_t* q);
void srsran_pbch_free(srsran_pbch_t* q);
/* cell.nof_ports == 0: search 1, 2 and 4 ports (never 3), q->cell.nof_ports stored as 4.  As pbch.c:247-252, the
 * stored cell and the scrambling sequence change only when the cell id does (or at the first call); the RE table
 * follows the stored cell.  The history is kept. */
int  srsran_pbch_set_cell(srsran_pbch_t* q, srsran_cell_t cell);
void srsran_pbch_decode_reset(srsran_pbch_t* q);
/* Host-synchronous.  Reads sf_symbols[0] and channel->ce[port][0] (full-grid host estimates) of one subframe 0 and
 * channel->noise_estimate: rx antenna 0 alone, as the reference.  1: MIB decoded (bch_payload, *nof_tx_ports,
 * *sfn_offset = dst - src + frame_idx - 1 written where not NULL, history reset); 0: not decoded, the frame is kept
 * for combining with the next ones (after a fourth miss the oldest is dropped); SRSRAN_ERROR_INVALID_INPUTS. */
int  srsran_pbch_decode(srsran_pbch_t* q, srsran_chest_dl_res_t* channel, cf_t* sf_symbols[SRSRAN_MAX_PORTS],
                        uint8_t bch_payload[SRSRAN_BCH_PAYLOAD_LEN], uint32_t* nof_tx_ports, int* sfn_offset);
/* MIB bits -> cell->nof_prb, phich_length, phich_resources and the SFN with its two low bits cleared. */
void srsran_pbch_mib_unpack(uint8_t* msg, srsran_cell_t* cell, uint32_t* sfn);
bool srsran_pbch_exists(int nframe, int nslot);
/* Host (pbch.c:111-130): copy the PBCH symbols into / out of slot 1 of one port's grid (slot1_data points at the
 * slot's first RE); the number of symbols.  The RE walk is the table the transmitter and the decoder use. */
int srsran_pbch_put(cf_t* pbch, cf_t* slot1_data, srsran_cell_t cell);
int srsran_pbch_get(cf_t* slot1_data, cf_t* pbch, srsran_cell_t cell);
/* added: the (frames combined, position, first frame) hypotheses srsran_pbch_decode tries per port count when
 * frame_idx frames are stored (the call's own included): 4, 11, 20, 30. */
uint32_t srsran_pbch_nof_hypotheses(uint32_t frame_idx);

/* ---------------- ue_mib.h ---------------- */
#define SRSRAN_UE_MIB_NOF_PRB 6
#define SRSRAN_UE_MIB_FOUND 1
#define SRSRAN_UE_MIB_NOTFOUND 0

typedef struct {
  cf_t*                 sf_symbols; /* host grid of rx antenna 0, SRSRAN_SF_LEN_RE(max_prb, normal CP) */
  srsran_ofdm_t         fft;
  srsran_pbch_t         pbch;
  srsran_chest_dl_t     chest;
  srsran_chest_dl_res_t chest_res;
  uint32_t              frame_cnt; /* misses since the last reset: host mirror, as pbch.frame_idx */
} srsran_ue_mib_t;

/* in_buffer: host samples of one subframe.  The OFDM receiver is built with the normal CP; set_cell switches it to the
 * cell's CP and bandwidth.  SRSRAN_ERROR without a HIP device. */
int  srsran_ue_mib_init(srsran_ue_mib_t* q, cf_t* in_buffer, uint32_t max_prb);
void srsran_ue_mib_free(srsran_ue_mib_t* q);
int  srsran_ue_mib_set_cell(srsran_ue_mib_t* q, srsran_cell_t cell);
void srsran_ue_mib_reset(srsran_ue_mib_t* q);
/* ue_mib.c:128-172, host-synchronous: srsran_ofdm_rx_sf, srsran_chest_dl_estimate with subframe index 0, a reset when
 * frame_cnt > 8, srsran_pbch_decode.  SRSRAN_UE_MIB_FOUND (both objects reset), SRSRAN_UE_MIB_NOTFOUND (frame_cnt
 * incremented) or SRSRAN_ERROR. */
int  srsran_ue_mib_decode(srsran_ue_mib_t* q, uint8_t bch_payload[SRSRAN_BCH_PAYLOAD_LEN], uint32_t* nof_tx_ports,
                          int* sfn_offset);

/* ---------------- added: batches on device buffers, asynchronous on `stream` ---------------- */
typedef struct {
  srsran_pbch_t* q;          /* an object appears at most once in a batch */
  const cf_t*    d_grid;     /* subframe 0 of rx antenna 0: 2 nsymb x 12 nof_prb */
  const cf_t*    d_ce;       /* [port][rx][ce_row_len], read at grid index modulo ce_row_len: rows of 12 nof_prb or of
                                the whole subframe (srsran_ue_dl_gpu_last_ce's two forms); rx 0 is read */
  uint32_t       ce_row_len;
  uint32_t       nof_rx;     /* rx antennas in d_ce (the stride between ports is nof_rx x ce_row_len) */
  const float*   d_noise;    /* the subframe's noise estimate */
} srsran_pbch_gpu_entry_t;

typedef struct {
  uint32_t found;
  uint32_t nof_tx_ports;
  int32_t  sfn_offset;
  uint8_t  payload[SRSRAN_BCH_PAYLOAD_LEN];
} srsran_pbch_gpu_res_t;

/* One srsran_pbch_decode per entry, one launch per stage for all of them whatever their cells.  d_out[i] and every
 * object's state afterwards are bit-identical to single calls in any order and composition.  The batch's descriptors
 * are staged in the first entry's object: batches that share it must be ordered on one stream. */
int srsran_pbch_gpu_decode_batch(uint32_t nof_entries, const srsran_pbch_gpu_entry_t* entries,
                                 srsran_pbch_gpu_res_t* d_out, void* stream);
/* Read-only: the object's LLR history on the device (*nof_llr = 4 x 2 nof_symbols floats, the first frame_idx x
 * 2 nof_symbols of them stored frames).  Waits for the device and refreshes q->frame_idx. */
int srsran_pbch_gpu_last_llr(srsran_pbch_t* q, const float** d_llr, uint32_t* nof_llr, uint32_t* frame_idx);
/* Read-only: the records of the last call's hypotheses, [i][nb, dst, src in the reference's loop order for four stored
 * frames], 3 x 30 of {uint32 accepted, uint8 bits[24]}.  i is the position in the object's list of port counts: 0, 1, 2
 * for 1, 2, 4 ports when every count is searched; with a known port count only i = 0 is written, for that count.
 * Hypotheses that did not run keep stale records. */
int srsran_pbch_gpu_last_hyp(srsran_pbch_t* q, const void** d_hyp, uint32_t* nof_hyp);

typedef struct {
  srsran_ue_mib_t* q;         /* an object appears at most once in a batch */
  const cf_t*      d_samples; /* one subframe of q->fft.sf_sz samples */
} srsran_ue_mib_gpu_entry_t;

/* One srsran_ue_mib_decode per entry from device samples: per object srsran_ofdm_rx_gpu and
 * srsran_chest_dl_gpu_estimate_batch_cfg on its one subframe with srsran_chest_dl_estimate's configuration (AVERAGE,
 * REFS noise, the automatic Gauss filter, which with REFS carries no state between calls), then the three PBCH
 * launches for all of them with the miss-counter rules applied on the device.  Results, counters and LLR history are
 * bit-identical to srsran_ue_mib_decode on the same samples, in any order and composition, so an object may be fed by
 * either call in turn. */
int srsran_ue_mib_gpu_decode_batch(uint32_t nof_entries, const srsran_ue_mib_gpu_entry_t* entries,
                                   srsran_pbch_gpu_res_t* d_out, void* stream);
/* Waits for the device and refreshes q->frame_cnt and q->pbch.frame_idx. */
int srsran_ue_mib_gpu_sync(srsran_ue_mib_t* q);

#ifdef __cplusplus
}
#endif
#endif /* SRSRAN_AMD_PBCH_H */
