// srsran_4g_amd/csrc/sch_api.cpp -- the srsran_sch_t object and the DL-SCH on it (include/srsran_sch.h):
//   sch object, its staging ring       sch.c:140-230
//   DL-SCH decode                      sch.c:371-609: host-synchronous, batched, with per-TB iteration limits
//   DL-SCH encode                      sch.c:240-359, 621-652
// Both run entirely on the GPU (sch_kernel.hip + the turbo decoders, enc_kernel.hip); the host only segments,
// builds descriptors and copies.  No CPU fallback.  The other parts of srsran_sch.h: fec_host.cpp (segmentation,
// CRC), rm_turbo_api.cpp (rate matching tables), softbuffer_api.cpp (soft buffers), uci_host.cpp and ulsch_api.cpp
// (UCI, UL-SCH); what these units share is in sch_units.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/srsran_sch.h"
#include "dev_buf.h"
#include "sch_kernel.h"
#include "tdec_kernel.h"
#include "tdec8bit_kernel.h"
#include "enc_kernel.h"
#include "pdsch_internal.h"
#include "sch_internal.h"
#include "sch_units.h"
#include "tdec_internal.h"
#include "stage_copy.h"
#include "stage_timing.h"

using namespace srsran_amd;

namespace {

constexpr uint32_t kWideStride = 4096;  // int16 values a widened row (>= 3 (800 + 32) + 12 and the decoders' reads)

constexpr size_t kDataCap = (size_t)SCH_MAX_CB * SCH_SLOT_BYTES;

bool init_ring(SchCtx* x)
{
  for (StageSlot& st : x->ring) {
    if (srsran_amd::ring_event_create(&st.staged) != hipSuccess ||
        srsran_amd::ring_event_create(&st.done) != hipSuccess) {
      return false;
    }
  }
  return srsran_amd::stage_fence_init(x->fence, kStageRing);
}

// the object's previous batches are done with its shared device state (grow paths)
void drain_batches(SchCtx* x)
{
  if (srsran_amd::stage_side_copy()) {
    if (x->used) {
      hipEventSynchronize(x->done);
    }
  } else {
    srsran_amd::handoff_drain(x->ho);
  }
}

struct Plan {
  srsran_cbsegm_t s{};
  int32_t         status = 1;
  uint32_t        slot0  = 0;
};

// decode_tb's checks (sch.c:509-546, decode_tb_cb 383-386), in the reference's order.
int32_t check_tb(const srsran_dlsch_gpu_tb_t& tb, srsran_cbsegm_t* s)
{
  if (srsran_cbsegm(s, tb.tbs)) {
    return SRSRAN_ERROR;  // srsran_dlsch_decode2: segmentation error (sch.c:592-595)
  }
  if (!tb.d_data || !tb.softbuffer || !tb.softbuffer->gpu || !tb.d_e_bits || tb.Qm == 0) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (s->tbs == 0 || s->C == 0) {
    return SRSRAN_SUCCESS;
  }
  if (s->F || s->C > tb.softbuffer->max_cb || tb.rv > 3) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (s->C > SRSRAN_MAX_CODEBLOCKS) {
    return SRSRAN_ERROR;
  }
  return 1;
}

// Enqueue the three-kernel DL-SCH decode of ntb transport blocks on `stream`.
// out_idx (optional): TB i's result / average-iterations slot is d_result[out_idx[i]] (default i).
int enqueue_batch(srsran_sch_t* q, uint32_t ntb, const srsran_dlsch_gpu_tb_t* tbs, int32_t* d_result, float* d_avg,
                  hipStream_t stream, bool early_copy = false, const uint32_t* out_idx = nullptr)
{
  srsran_amd::HostScope desc(srsran_amd::HP_SCH_DESC);
  SchCtx*           x  = (SchCtx*)q->gpu;
  const bool        b8 = q->llr_is_8bit;  // int8 e bits / soft buffers (sch.c:409-428)
  std::vector<Plan> plan(ntb);
  uint32_t          nslots = 0;
  for (uint32_t i = 0; i < ntb; i++) {
    plan[i].status = check_tb(tbs[i], &plan[i].s);
    if (plan[i].status == 1) {
      plan[i].slot0 = nslots;
      nslots += plan[i].s.C;
    }
  }
  // per-slot de-matching descriptors, and turbo descriptors grouped by K
  std::vector<RmSlot>                         rm(nslots);
  std::map<uint32_t, std::vector<uint32_t>>   by_k;
  std::vector<uint8_t>                        slot_crc_a(nslots);
  uint32_t                                    max_len = 0, max_e = 0;
  for (uint32_t i = 0; i < ntb; i++) {
    if (plan[i].status != 1) {
      continue;
    }
    const srsran_cbsegm_t& s  = plan[i].s;
    const SbGpu*           sb = (const SbGpu*)tbs[i].softbuffer->gpu;
    const uint32_t         Qm = tbs[i].Qm;
    InvTable               tk[2];  // the de-matching tables of K1 and K2 (looked up once per TB)
    // the soft buffer layout of the decoder that takes K: the 16-bit AUTO one, or with llr_is_8bit the 8-bit one
    // (rm_turbo_rx_lut_8bit: srsran_tdec_autoimp_get_subblocks_8bit)
    auto table = [&](uint32_t idx, InvTable* t) {
      return b8 ? inv_table_nsb(idx, tbs[i].rv, srsran_tdec_autoimp_get_subblocks_8bit(srsran_cbsegm_cbsize(idx)), t)
                : inv_table(idx, tbs[i].rv, true, t);
    };
    if (!table(s.K1_idx, &tk[0]) || (s.C2 && !table(s.K2_idx, &tk[1]))) {
      return SRSRAN_ERROR;
    }
    for (uint32_t cb = 0; cb < s.C; cb++) {
      const uint32_t K     = cb < s.C1 ? s.K1 : s.K2;
      // E split over the CBs, including the reference's '>' (sch.c:398-407).  Not enc_push_cbs' split: the
      // transmitter's 'i <= C - gamma - 1' differs from this at cb == C - gamma, as in the reference.
      const uint32_t Gp    = tbs[i].nof_e_bits / Qm;
      const uint32_t gamma = Gp % s.C;
      const uint32_t n_e   = Qm * (Gp / s.C);
      uint32_t       rp = cb * n_e, n_e2 = n_e;
      if (cb > s.C - gamma) {
        n_e2 = n_e + Qm;
        rp   = (s.C - gamma) * n_e + (cb - (s.C - gamma)) * n_e2;
      }
      const InvTable& t    = tk[cb < s.C1 ? 0 : 1];
      const uint32_t slot = plan[i].slot0 + cb;
      RmSlot&        r    = rm[slot];
      r.e                 = b8 ? (const short*)((const int8_t*)tbs[i].d_e_bits + rp) : tbs[i].d_e_bits + rp;
      r.sb                = sb->d_buf + (size_t)cb * sb->stride;
      r.skip              = sb->d_flags + cb;
      r.inv               = t.d;
      r.E                 = n_e2;
      r.len               = t.len;
      r.N                 = t.N;
      r.overwrite         = tbs[i].new_data ? 1 : 0;
      max_len             = std::max(max_len, t.len);
      max_e               = std::max(max_e, n_e2);
      by_k[K].push_back(slot);
      slot_crc_a[slot] = s.C == 1;  // single-CB TB: CRC24A over tbs + 24 (sch.c:440-446)
    }
  }
  // turbo descriptors by K; every two consecutive blocks of a group (one lane-pair workgroup) lie
  // within TDEC_PAIR_SPAN of each other, padded where the soft buffers are far apart
  // llr_is_8bit with K <= 800: the reference widens the block for a 16-bit decoder (tdec_iteration_8,
  // turbodecoder.c:470-481); those rows are widened into d_wide first
  std::vector<Widen8> wide;
  uint32_t            max_wide = 0;
  if (b8) {
    for (auto& kv : by_k) {
      if (srsran_tdec_autoimp_get_subblocks_8bit(kv.first) < 16) {
        for (uint32_t slot : kv.second) {
          wide.push_back(Widen8{(const int8_t*)rm[slot].sb, nullptr, rm[slot].len});
          max_wide = std::max(max_wide, rm[slot].len);
        }
      }
    }
    if (wide.size() > x->wide_cap) {
      drain_batches(x);
      const size_t rows = std::max(wide.size() * 2, (size_t)16);
      x->wide_cap       = 0;
      if (!x->d_wide.reserve(rows * kWideStride)) {
        return SRSRAN_ERROR;
      }
      x->wide_cap = rows;
    }
    for (size_t j = 0; j < wide.size(); j++) {
      wide[j].dst = x->d_wide + j * kWideStride;
    }
  }
  std::vector<TdecCb> cbs;
  cbs.reserve(nslots + 16);
  std::vector<std::pair<uint32_t, uint32_t>> groups;  // (K, first index into cbs)
  std::vector<TdecCb>                        kcbs;
  uint32_t                                   nw = 0;
  for (auto& kv : by_k) {
    groups.emplace_back(kv.first, (uint32_t)cbs.size());
    kcbs.clear();
    const bool widened = b8 && srsran_tdec_autoimp_get_subblocks_8bit(kv.first) < 16;
    for (uint32_t slot : kv.second) {
      TdecCb c;
      c.in    = widened ? wide[nw++].dst : rm[slot].sb;
      c.skip  = rm[slot].overwrite ? x->d_zero : rm[slot].skip;  // a new transmission decodes every CB
      c.slot  = slot;
      c.crc_a = slot_crc_a[slot];
      kcbs.push_back(c);
    }
    tdec_pair_cbs(kcbs.data(), (uint32_t)kcbs.size(), cbs.size(), &cbs);
  }
  const uint32_t ncbs = (uint32_t)cbs.size();
  std::vector<SchTb> tbd(ntb);
  for (uint32_t i = 0; i < ntb; i++) {
    SchTb& t = tbd[i];
    memset(&t, 0, sizeof(t));
    t.result = d_result + (out_idx ? out_idx[i] : i);
    t.avg    = d_avg + (out_idx ? out_idx[i] : i);
    t.status = plan[i].status;
    const srsran_softbuffer_rx_t* sbh = tbs[i].softbuffer;
    if (sbh && sbh->gpu) {
      const SbGpu* sb = (const SbGpu*)sbh->gpu;
      t.cb_crc        = sb->d_flags;
      t.tb_crc        = sb->d_flags + sbh->max_cb;
      t.saved         = sb->d_data;
      t.saved_stride  = sb->data_stride;
      t.sbuf          = sb->d_buf;
      t.sb_stride     = sb->stride;
      t.max_cb        = sbh->max_cb;
      t.nof_cb_reset  = std::min((tbs[i].tbs + 24) / (SRSRAN_TCOD_MAX_LEN_CB - 24) + 1, sbh->max_cb);
      t.new_data      = tbs[i].new_data ? 1 : 0;
    }
    if (plan[i].status != 1) {
      continue;
    }
    t.data          = tbs[i].d_data;
    t.cbout         = nullptr;  // filled below once the scratch is sized
    t.slot0         = plan[i].slot0;
    t.C             = plan[i].s.C;
    t.C1            = plan[i].s.C1;
    t.K1            = plan[i].s.K1;
    t.K2            = plan[i].s.K2;
    t.tbs           = plan[i].s.tbs;
  }

  // the previous batch of this object must be done with the shared scratch: ordered by the stream, or by the
  // hand-over when this batch comes on another stream (side staging: the round-3 event)
  const bool side = srsran_amd::stage_side_copy();
  if (side) {
    if (x->used) {
      hipStreamWaitEvent(stream, x->done, 0);
    }
  } else if (srsran_amd::handoff(x->ho, stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  const size_t off_cbs  = align16(nslots * sizeof(RmSlot));
  const size_t off_tb   = off_cbs + align16(ncbs * sizeof(TdecCb));
  const size_t off_wide = off_tb + align16(ntb * sizeof(SchTb));
  const size_t bytes    = off_wide + align16(wide.size() * sizeof(Widen8));
  desc.stop();
  srsran_amd::HostScope wait(srsran_amd::HP_SCH_WAIT);
  const int  slot   = (int)x->ring_next;
  StageSlot& st     = x->ring[slot];
  x->ring_next = (x->ring_next + 1) % kStageRing;
  if (st.used) {
    if (side) {
      hipEventSynchronize(st.staged);
    } else if (!srsran_amd::stage_fence_wait(x->fence, slot, st.seq)) {
      return SRSRAN_ERROR;
    }
  }
  wait.stop();
  srsran_amd::HostScope launch(srsran_amd::HP_SCH_LAUNCH);
  if (bytes > st.d.cap()) {  // every slot of the ring grows now: no allocation when the others come round
    const size_t cap = std::max(bytes * 2, (size_t)4096);
    for (StageSlot& r : x->ring) {
      if (r.d.cap() >= cap) {
        continue;
      }
      if (r.used) {
        if (side) {
          hipEventSynchronize(r.done);
        } else {
          srsran_amd::handoff_drain(x->ho);
        }
      }
      hipHostFree(r.h);  // stage_host_alloc's memory (stage_copy.h)
      r.d.reset();
      r.h = (char*)srsran_amd::stage_host_alloc(cap, (void**)&r.hd);
      if (!r.h || !r.d.reserve(cap)) {
        return SRSRAN_ERROR;
      }
    }
  }
  if (nslots * (size_t)SCH_SLOT_BYTES > x->d_cbout.cap() || nslots > x->d_noi.cap() ||
      nslots > x->d_crc_ok.cap()) {
    drain_batches(x);
    const size_t cap = std::max((size_t)nslots * 2, (size_t)64);
    if (!x->d_cbout.reserve(cap * SCH_SLOT_BYTES) || !x->d_noi.reserve(cap) || !x->d_crc_ok.reserve(cap)) {
      return SRSRAN_ERROR;
    }
  }
  uint32_t max_tbs = 0;
  for (uint32_t i = 0; i < ntb; i++) {
    SchTb& t = tbd[i];
    if (t.status == 1) {
      t.cbout  = x->d_cbout;
      t.noi    = x->d_noi;
      t.crc_ok = x->d_crc_ok;
      max_tbs  = std::max(max_tbs, t.tbs);
    }
  }
  memcpy(st.h, rm.data(), nslots * sizeof(RmSlot));
  memcpy(st.h + off_cbs, cbs.data(), ncbs * sizeof(TdecCb));
  memcpy(st.h + off_tb, tbd.data(), ntb * sizeof(SchTb));
  if (!wide.empty()) {
    memcpy(st.h + off_wide, wide.data(), wide.size() * sizeof(Widen8));
  }
  // SRSRAN_AMD_STAGE=side, early_copy (the PDSCH chain, whose stream runs OFDM ... LLR before the de-matching): the upload runs on
  // the copy stream as soon as the slot's previous batch is done with it, beside those stages, and the
  // launches below wait for it instead of having the copy's latency in line in front of them (chain
  // 243-246 k -> 250-255 k subframes/s, gpurun_out r03ah).  A batch with nothing in front of it keeps the
  // in-stream upload (the cross-stream wait costs a standalone DL-SCH batch ~10 us).
  // Default: a copy kernel in the launch stream reads the pinned slot (stage_copy.h) -- no copy-engine launch
  // and no cross-stream waits, each of which left the GPU idle ~10-15 us (r04j trace).
  if (!side) {
    st.seq = ++x->fence.seq;
    if (srsran_amd::stage_copy_or_record(st.d, st.hd, bytes, stream, nullptr, 0, &x->fence, slot, st.seq) !=
        hipSuccess) {
      return SRSRAN_ERROR;
    }
  } else {
    hipStream_t up = stream;
    if (early_copy) {
      up = x->copy;
      if (st.used) {
        hipStreamWaitEvent(up, st.done, 0);
      }
    }
    if (hipMemcpyAsync(st.d, st.h, bytes, hipMemcpyHostToDevice, up) != hipSuccess) {
      return SRSRAN_ERROR;
    }
    hipEventRecord(st.staged, up);
    if (early_copy) {
      hipStreamWaitEvent(stream, st.staged, 0);
    }
  }
  x->used  = true;
  st.used  = true;
  char* ds = st.d;

  // the launches (recorded instead when a UE DL batch defers them, stage_copy.h)
  int ret = SRSRAN_SUCCESS;
  if (nslots) {
    const RmSlot*  slots = (const RmSlot*)ds;
    const Widen8*  wd    = (const Widen8*)(ds + off_wide);
    const uint32_t nwide = (uint32_t)wide.size();
    if (srsran_amd::launch_or_record([=] {
          const hipError_t e = b8 ? rm8_rx_slots_launch(slots, nslots, max_len, stream)
                                  : rm_rx_launch(slots, nslots, max_len, max_e, stream);
          return e != hipSuccess ? e : widen8_launch(wd, nwide, max_wide, stream);
        }) != hipSuccess) {
      ret = SRSRAN_ERROR;
    }
    const int n_end = q->max_iterations > 0 ? (int)q->max_iterations : 1;
    for (size_t g = 0; g < groups.size() && ret == SRSRAN_SUCCESS; g++) {
      const uint32_t first  = groups[g].second;
      const uint32_t count  = (g + 1 < groups.size() ? groups[g + 1].second : (uint32_t)cbs.size()) - first;
      const uint32_t K      = groups[g].first;
      const TdecCb*  dcb    = (const TdecCb*)(ds + off_cbs) + first;
      const bool     dec8   = b8 && srsran_tdec_autoimp_get_subblocks_8bit(K) >= 16;
      uint8_t*       cbout  = x->d_cbout;
      uint8_t*       noi    = x->d_noi;
      uint8_t*       crc_ok = x->d_crc_ok;
      if (srsran_amd::launch_or_record([=] {
            const int r = dec8 ? tdec8_sch_enqueue(K, dcb, count, cbout, SCH_SLOT_BYTES, noi, crc_ok, n_end, stream)
                               : tdec_sch_enqueue(K, dcb, count, cbout, SCH_SLOT_BYTES, noi, crc_ok, n_end, stream);
            return r == SRSRAN_SUCCESS ? hipSuccess : hipErrorLaunchFailure;
          }) != hipSuccess) {
        ret = SRSRAN_ERROR;
      }
    }
  }
  const SchTb* d_tbs = (const SchTb*)(ds + off_tb);
  if (ret == SRSRAN_SUCCESS &&
      srsran_amd::launch_or_record([=] { return tb_launch(d_tbs, ntb, max_tbs, stream); }) != hipSuccess) {
    ret = SRSRAN_ERROR;
  }
  if (side) {
    hipEventRecord(x->done, stream);
    hipEventRecord(st.done, stream);
  }
  return ret;
}

// What a batch entry point answers before it looks at a TB: an error, SUCCESS for an empty batch, or 1 to go on.
int batch_entry(const srsran_sch_t* q, uint32_t nof_tb, bool have_args)
{
  if (!q || !q->gpu || (nof_tb && !have_args)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  return nof_tb == 0 ? SRSRAN_SUCCESS : 1;
}

}  // namespace

extern "C" {

// ---------------- sch.c:140-230 ----------------
int srsran_sch_init(srsran_sch_t* q)
{
  if (!q) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  memset(q, 0, sizeof(*q));
  if (srsran_tdec_init(&q->decoder, SRSRAN_TCOD_MAX_LEN_CB)) {
    return SRSRAN_ERROR;
  }
  q->max_iterations = 10;  // SRSRAN_PDSCH_MAX_TDEC_ITERS (sch.c:36)
  SchCtx* x         = new SchCtx();
  q->gpu            = x;
  if (hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&x->copy, hipStreamNonBlocking) != hipSuccess ||
      srsran_amd::ring_event_create(&x->done) != hipSuccess || !init_ring(x) ||
      !x->d_data.reserve(kDataCap) || !x->d_res.reserve(4) || !x->d_avg.reserve(4) || !x->h_io.reserve(256) ||
      !x->d_zero.reserve(8) || hipMemset(x->d_zero, 0, 8) != hipSuccess) {
    srsran_sch_free(q);
    return SRSRAN_ERROR;
  }
  return SRSRAN_SUCCESS;
}

void srsran_sch_free(srsran_sch_t* q)
{
  if (!q) {
    return;
  }
  SchCtx* x = (SchCtx*)q->gpu;
  if (x) {
    srsran_amd::handoff_drain(x->ho);  // batches on the caller's streams
    if (x->stream) {
      hipStreamSynchronize(x->stream);
      hipStreamDestroy(x->stream);
    }
    if (x->copy) {
      hipStreamSynchronize(x->copy);
      hipStreamDestroy(x->copy);
    }
    if (x->done) {
      hipEventDestroy(x->done);
    }
    for (StageSlot& st : x->ring) {
      if (st.staged) {
        hipEventDestroy(st.staged);
      }
      if (st.done) {
        hipEventDestroy(st.done);
      }
      hipHostFree(st.h);  // stage_host_alloc's memory (stage_copy.h)
    }
    srsran_amd::stage_fence_free(x->fence);
    srsran_amd::handoff_free(x->ho);
    if (x->uldesc_used) {
      hipEventDestroy(x->uldesc_used);
    }
    delete x;
  }
  srsran_tdec_free(&q->decoder);
  memset(q, 0, sizeof(*q));
}

void srsran_sch_set_max_noi(srsran_sch_t* q, uint32_t max_iterations)
{
  if (q) {
    q->max_iterations = max_iterations ? max_iterations : 10;
  }
}

float srsran_sch_last_noi(srsran_sch_t* q) { return q ? q->avg_iterations : 0.0f; }

}  // extern "C"

// ---------------- sch.c:509-609 (host-synchronous) ----------------
int srsran_amd::dlsch_decode_sync(srsran_sch_t*       q,
                                  srsran_pdsch_cfg_t* cfg,
                                  const int16_t*      e_bits,
                                  const int16_t*      d_e_bits,
                                  uint8_t*            data,
                                  int                 tb_idx,
                                  uint32_t            nof_layers)
{
  if (!q || !q->gpu || !cfg || tb_idx < 0 || tb_idx >= SRSRAN_MAX_CODEWORDS) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  SchCtx*                 x  = (SchCtx*)q->gpu;
  const uint32_t          Nl = nof_layers != cfg->grant.nof_tb ? 2 : 1;
  srsran_softbuffer_rx_t* sb = cfg->softbuffers.rx[tb_idx];
  // the TB as the batch path takes it, refused by the same checks (no message for a segmentation error any more:
  // srsran_cbsegm cannot fail on a non-null s)
  srsran_dlsch_gpu_tb_t tb;
  tb.tbs        = (uint32_t)cfg->grant.tb[tb_idx].tbs;
  tb.Qm         = srsran_mod_bits_x_symbol(cfg->grant.tb[tb_idx].mod) * Nl;
  tb.rv         = (uint32_t)cfg->grant.tb[tb_idx].rv;
  tb.nof_e_bits = cfg->grant.tb[tb_idx].nof_bits;
  tb.d_e_bits   = d_e_bits ? d_e_bits : e_bits;  // host LLRs: the pointer stands in until they are uploaded
  tb.d_data     = data ? x->d_data.get() : nullptr;
  tb.softbuffer = sb;
  tb.new_data   = 0;
  srsran_cbsegm_t s;
  const int32_t   status = check_tb(tb, &s);
  if (status != 1) {
    return status;
  }
  const uint32_t nbe = tb.nof_e_bits;
  const size_t   esz = q->llr_is_8bit ? sizeof(int8_t) : sizeof(int16_t);  // e_bits are int8 with llr_is_8bit
  hipStreamSynchronize(x->stream);
  if (!d_e_bits) {
    if (!x->d_e.reserve((std::max<size_t>(nbe, 1) * esz + 1) / 2)) {
      return SRSRAN_ERROR;
    }
    tb.d_e_bits = x->d_e;
  }
  // the host cb_crc mirror is authoritative for the synchronous API
  SbGpu* g = (SbGpu*)sb->gpu;
  for (uint32_t i = 0; i < s.C; i++) {
    x->h_io[i] = sb->cb_crc[i] ? 1 : 0;
  }
  hipMemcpyAsync(g->d_flags, x->h_io, s.C, hipMemcpyHostToDevice, x->stream);
  if (!d_e_bits) {
    hipMemcpyAsync(x->d_e, e_bits, (size_t)nbe * esz, hipMemcpyHostToDevice, x->stream);
  }
  uint32_t end = 0;  // bytes of `data` the reference writes (sch.c:425-431, 476-480)
  for (uint32_t cb = 0; cb < s.C; cb++) {
    const uint32_t K    = cb < s.C1 ? s.K1 : s.K2;
    const uint32_t rlen = s.C == 1 ? K : K - 24;
    end                 = std::max(end, cb * rlen / 8 + (sb->cb_crc[cb] ? rlen / 8 : K / 8));
  }
  hipStreamSynchronize(x->stream);  // h_io is reused below
  int ret = enqueue_batch(q, 1, &tb, x->d_res, x->d_avg, x->stream);
  if (ret != SRSRAN_SUCCESS) {
    hipStreamSynchronize(x->stream);
    return ret;
  }
  uint8_t* h_flags = x->h_io;
  int32_t* h_res   = (int32_t*)(x->h_io + 128);
  float*   h_avg   = (float*)(x->h_io + 136);
  hipMemcpyAsync(data, x->d_data, end, hipMemcpyDeviceToHost, x->stream);
  hipMemcpyAsync(h_flags, g->d_flags, s.C, hipMemcpyDeviceToHost, x->stream);
  hipMemcpyAsync(h_flags + 64, g->d_flags + sb->max_cb, 1, hipMemcpyDeviceToHost, x->stream);
  hipMemcpyAsync(h_res, x->d_res, sizeof(int32_t), hipMemcpyDeviceToHost, x->stream);
  hipMemcpyAsync(h_avg, x->d_avg, sizeof(float), hipMemcpyDeviceToHost, x->stream);
  if (hipStreamSynchronize(x->stream) != hipSuccess) {
    fprintf(stderr, "[srsran_sch] decode failed: %s\n", hipGetErrorString(hipGetLastError()));
    return SRSRAN_ERROR;
  }
  for (uint32_t i = 0; i < s.C; i++) {
    sb->cb_crc[i] = h_flags[i] != 0;
  }
  sb->tb_crc        = h_flags[64] != 0;
  q->avg_iterations = *h_avg;
  return *h_res;
}

extern "C" {

int srsran_dlsch_decode2(srsran_sch_t*       q,
                         srsran_pdsch_cfg_t* cfg,
                         int16_t*            e_bits,
                         uint8_t*            data,
                         int                 tb_idx,
                         uint32_t            nof_layers)
{
  return dlsch_decode_sync(q, cfg, e_bits, nullptr, data, tb_idx, nof_layers);
}

/* added: srsran_dlsch_decode2 with the LLRs already in device memory (complete before the call) */
int srsran_dlsch_decode2_dev(srsran_sch_t*       q,
                             srsran_pdsch_cfg_t* cfg,
                             const int16_t*      d_e_bits,
                             uint8_t*            data,
                             int                 tb_idx,
                             uint32_t            nof_layers)
{
  if (!d_e_bits) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  return dlsch_decode_sync(q, cfg, nullptr, d_e_bits, data, tb_idx, nof_layers);
}

int srsran_dlsch_decode(srsran_sch_t* q, srsran_pdsch_cfg_t* cfg, int16_t* e_bits, uint8_t* data)
{
  return srsran_dlsch_decode2(q, cfg, e_bits, data, 0, 1);
}

int srsran_dlsch_gpu_decode_batch(srsran_sch_t*                q,
                                  uint32_t                     nof_tb,
                                  const srsran_dlsch_gpu_tb_t* tbs,
                                  int32_t*                     d_result,
                                  float*                       d_avg_noi,
                                  void*                        stream)
{
  const int go = batch_entry(q, nof_tb, tbs && d_result && d_avg_noi);
  return go != 1 ? go : enqueue_batch(q, nof_tb, tbs, d_result, d_avg_noi, (hipStream_t)stream);
}

}  // extern "C"

namespace srsran_amd {
int dlsch_gpu_decode_batch_early_copy(srsran_sch_t* q, uint32_t nof_tb, const srsran_dlsch_gpu_tb_t* tbs,
                                      int32_t* d_result, float* d_avg_noi, void* stream)
{
  const int go = batch_entry(q, nof_tb, tbs && d_result && d_avg_noi);
  return go != 1 ? go : enqueue_batch(q, nof_tb, tbs, d_result, d_avg_noi, (hipStream_t)stream, true);
}

int dlsch_gpu_decode_batch_limits(srsran_sch_t* q, uint32_t nof_tb, const srsran_dlsch_gpu_tb_t* tbs,
                                  const uint32_t* max_noi, int32_t* d_result, float* d_avg_noi, void* stream)
{
  const int go = batch_entry(q, nof_tb, tbs && max_noi && d_result && d_avg_noi);
  if (go != 1) {
    return go;
  }
  // distinct limits in first-appearance order; 0 keeps the limit in force, as pdsch.c:815-817 does
  std::vector<uint32_t> lim(nof_tb);
  std::vector<uint32_t> order;
  for (uint32_t i = 0; i < nof_tb; i++) {
    lim[i] = max_noi[i] ? max_noi[i] : (i ? lim[i - 1] : q->max_iterations);
    if (std::find(order.begin(), order.end(), lim[i]) == order.end()) {
      order.push_back(lim[i]);
    }
  }
  if (order.size() == 1) {
    srsran_sch_set_max_noi(q, order[0]);
    return enqueue_batch(q, nof_tb, tbs, d_result, d_avg_noi, (hipStream_t)stream, true);
  }
  std::vector<srsran_dlsch_gpu_tb_t> sub;
  std::vector<uint32_t>              idx;
  for (uint32_t l : order) {
    sub.clear();
    idx.clear();
    for (uint32_t i = 0; i < nof_tb; i++) {
      if (lim[i] == l) {
        sub.push_back(tbs[i]);
        idx.push_back(i);
      }
    }
    srsran_sch_set_max_noi(q, l);
    const int r = enqueue_batch(q, (uint32_t)sub.size(), sub.data(), d_result, d_avg_noi, (hipStream_t)stream, true,
                                idx.data());
    if (r != SRSRAN_SUCCESS) {
      return r;
    }
  }
  srsran_sch_set_max_noi(q, lim[nof_tb - 1]);  // as after the last TB's sequential decode
  return SRSRAN_SUCCESS;
}

hipStream_t sch_stream(srsran_sch_t* q) { return q && q->gpu ? ((SchCtx*)q->gpu)->stream : nullptr; }

// The object's decode stream moved to a hardware queue of its own (own_queue_stream, stage_copy.h).  srsENB runs one PUSCH object
// per PHY worker, several batches at once: two workers' streams that the runtime maps to one queue run their
// batches one after the other (least-used queue assignment, which depends on the streams created and freed before:
// 424 k UE-subframes/s with two workers standalone, 284 k after a PDSCH run in the same process, 422 k with this;
// tools/r06as_pusch_order.py).  SRSRAN_AMD_PUSCH_OWN_QUEUE=0 (read once) keeps the shared queue.
int sch_own_queue(srsran_sch_t* q)
{
  static const bool on = [] {
    const char* e = getenv("SRSRAN_AMD_PUSCH_OWN_QUEUE");
    return !e || atoi(e) != 0;
  }();
  SchCtx* x = q && q->gpu ? (SchCtx*)q->gpu : nullptr;
  if (!x) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (!on) {
    return SRSRAN_SUCCESS;
  }
  hipStream_t s = nullptr;
  if (own_queue_stream(&s) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  hipStreamSynchronize(x->stream);
  hipStreamDestroy(x->stream);
  x->stream = s;
  return SRSRAN_SUCCESS;
}

// ---------------- DL-SCH transmit (sch.c:240-359, 621-652) ----------------
int enc_push_cbs(std::vector<EncCb>& cb, EncFwdMap& fwd, const srsran_cbsegm_t& s, uint32_t Qm, uint32_t rv,
                 uint32_t nof_e_bits, const uint8_t* d_data, uint32_t tbs, size_t e_off, uint32_t t, uint32_t* wp_out)
{
  const uint32_t Gp = nof_e_bits / Qm, gamma = Gp % s.C;
  uint32_t       rp = 0, wp = 0;
  for (uint32_t i = 0; i < s.C; i++) {
    const uint32_t K   = i < s.C2 ? s.K2 : s.K1;
    const uint32_t idx = i < s.C2 ? s.K2_idx : s.K1_idx;
    EncCb          c;
    memset(&c, 0, sizeof(c));
    c.rlen = s.C > 1 ? K - 24 : K;
    // the transmitter's split (sch.c:271-305).  Not enqueue_batch's: the receiver's 'cb > C - gamma' differs from
    // this at i == C - gamma, as in the reference.
    c.E    = i <= s.C - gamma - 1 ? Qm * (Gp / s.C) : Qm * ((Gp + s.C - 1) / s.C);
    c.K    = K;
    c.rp   = rp;
    c.cb_crc   = s.C > 1;
    c.tb_bytes = tbs / 8;
    c.data     = d_data;
    qpp_coeffs(idx, &c.f1, &c.f2);
    auto it = fwd.find(idx * 4 + rv);
    if (it == fwd.end()) {
      std::pair<const uint16_t*, uint32_t> v;
      if (!rm_fwd_table(idx, rv, &v.first, &v.second)) {
        return SRSRAN_ERROR;
      }
      it = fwd.emplace(idx * 4 + rv, v).first;
    }
    c.fwd = it->second.first;
    c.N   = it->second.second;
    c.e    = (uint8_t*)(uintptr_t)(e_off + wp);  // offsets: fixed up after the allocation
    c.tb_crc = (const uint32_t*)(uintptr_t)t;
    cb.push_back(c);
    rp += c.rlen;
    wp += c.E;
  }
  *wp_out = wp;
  return SRSRAN_SUCCESS;
}
}  // namespace srsran_amd

extern "C" {

int srsran_dlsch_gpu_encode_batch(srsran_sch_t* q, uint32_t nof_tb, const srsran_dlsch_gpu_enc_t* tbs, void* stream)
{
  if (!q || !q->gpu || (nof_tb && !tbs)) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (nof_tb == 0) {
    return SRSRAN_SUCCESS;
  }
  SchCtx*              x  = (SchCtx*)q->gpu;
  hipStream_t          st = (hipStream_t)stream;
  std::vector<EncTb>   tb(nof_tb);
  std::vector<EncCb>   cb;
  std::vector<size_t>  e_off(nof_tb);
  size_t               e_tot = 0;
  uint32_t             max_bytes = 0;
  EncFwdMap            fwd;
  for (uint32_t t = 0; t < nof_tb; t++) {
    const srsran_dlsch_gpu_enc_t& in = tbs[t];
    srsran_cbsegm_t               s;
    if (!in.d_data || !in.d_e_bits || in.Qm == 0 || in.rv > 3 || srsran_cbsegm(&s, in.tbs) || s.tbs == 0) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    if (s.F) {
      fprintf(stderr, "[srsran_sch] Error filler bits are not supported. Use standard TBS\n");
      return SRSRAN_ERROR;
    }
    e_off[t] = e_tot;
    e_tot += (in.nof_e_bits + 15) & ~15u;
    max_bytes = std::max(max_bytes, (in.nof_e_bits + 7) / 8);
    uint32_t wp = 0;
    const int r = enc_push_cbs(cb, fwd, s, in.Qm, in.rv, in.nof_e_bits, in.d_data, in.tbs, e_off[t], t, &wp);
    if (r != SRSRAN_SUCCESS) {
      return r;
    }
    if (wp > in.nof_e_bits) {
      return SRSRAN_ERROR_INVALID_INPUTS;
    }
    tb[t] = {in.d_data, nullptr, nullptr, in.d_e_bits, in.tbs / 8, in.nof_e_bits};
  }
  // device scratch: [EncTb x ntb][EncCb x ncb][crc x ntb][unpacked e bits]
  const size_t o_cb = align16(nof_tb * sizeof(EncTb)), o_crc = o_cb + align16(cb.size() * sizeof(EncCb));
  const size_t o_e = o_crc + align16(nof_tb * sizeof(uint32_t)), need = o_e + e_tot;
  if (!x->d_enc.reserve(need)) {
    return SRSRAN_ERROR;
  }
  uint32_t* d_crc = (uint32_t*)(x->d_enc + o_crc);
  uint8_t*  d_e   = x->d_enc + o_e;
  for (uint32_t t = 0; t < nof_tb; t++) {
    tb[t].crc    = d_crc + t;
    tb[t].e_bits = d_e + e_off[t];
  }
  for (EncCb& c : cb) {
    c.e      = d_e + (size_t)(uintptr_t)c.e;
    c.tb_crc = d_crc + (size_t)(uintptr_t)c.tb_crc;
  }
  const EncTb* d_tb = (const EncTb*)x->d_enc.get();
  const EncCb* d_cb = (const EncCb*)(x->d_enc + o_cb);
  if (hipMemcpyAsync(x->d_enc, tb.data(), nof_tb * sizeof(EncTb), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(x->d_enc + o_cb, cb.data(), cb.size() * sizeof(EncCb), hipMemcpyHostToDevice, st) != hipSuccess ||
      enc_tb_crc_launch(d_tb, nof_tb, st) != hipSuccess || enc_cb_launch(d_cb, (uint32_t)cb.size(), st) != hipSuccess ||
      enc_pack_launch(d_tb, nof_tb, max_bytes, st) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  // x->d_enc is reused by the next call in stream order (one stream per object)
  return SRSRAN_SUCCESS;
}

int srsran_dlsch_encode2(srsran_sch_t*       q,
                         srsran_pdsch_cfg_t* cfg,
                         uint8_t*            data,
                         uint8_t*            e_bits,
                         int                 tb_idx,
                         uint32_t            nof_layers)
{
  if (!q || !q->gpu || !cfg || !e_bits || tb_idx < 0 || tb_idx >= SRSRAN_MAX_CODEWORDS) {
    return SRSRAN_ERROR_INVALID_INPUTS;
  }
  if (!data) {
    fprintf(stderr, "[srsran_sch] encoding from the soft buffer (data == NULL) is not provided\n");
    return SRSRAN_ERROR;
  }
  const srsran_ra_tb_t& t  = cfg->grant.tb[tb_idx];
  const uint32_t        Nl = nof_layers != cfg->grant.nof_tb ? 2 : 1;  // sch.c:633-636
  const uint32_t        Qm = srsran_mod_bits_x_symbol(t.mod) * Nl;
  if (t.tbs <= 0) {
    return t.tbs == 0 ? SRSRAN_SUCCESS : SRSRAN_ERROR_INVALID_INPUTS;
  }
  SchCtx*        x      = (SchCtx*)q->gpu;
  const uint32_t nbytes = (uint32_t)t.tbs / 8, ebytes = (t.nof_bits + 7) / 8;
  uint8_t*       d_io   = nullptr;
  if (hipMallocAsync((void**)&d_io, nbytes + ebytes + 16, x->stream) != hipSuccess) {
    return SRSRAN_ERROR;
  }
  srsran_dlsch_gpu_enc_t e = {(uint32_t)t.tbs, Qm, (uint32_t)t.rv, t.nof_bits, d_io, d_io + nbytes};
  int                    r = SRSRAN_ERROR;
  if (hipMemcpyAsync(d_io, data, nbytes, hipMemcpyHostToDevice, x->stream) == hipSuccess) {
    r = srsran_dlsch_gpu_encode_batch(q, 1, &e, x->stream);
    if (r == SRSRAN_SUCCESS &&
        (hipMemcpyAsync(e_bits, d_io + nbytes, ebytes, hipMemcpyDeviceToHost, x->stream) != hipSuccess ||
         hipStreamSynchronize(x->stream) != hipSuccess)) {
      r = SRSRAN_ERROR;
    }
  }
  hipFreeAsync(d_io, x->stream);
  hipStreamSynchronize(x->stream);
  return r;
}

int srsran_dlsch_encode(srsran_sch_t* q, srsran_pdsch_cfg_t* cfg, uint8_t* data, uint8_t* e_bits)
{
  return srsran_dlsch_encode2(q, cfg, data, e_bits, 0, 1);
}

}  // extern "C"

