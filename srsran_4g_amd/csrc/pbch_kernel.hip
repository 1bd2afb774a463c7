// srsran_4g_amd/csrc/pbch_kernel.hip -- PBCH receive (pbch.c:395-553) for gfx950, three launches for any number of
// entries (one entry = one srsran_pbch_t and the subframe 0 it receives).
//
//   pbch_llr_kernel     one workgroup per (entry, port-count hypothesis): gathers the PBCH REs of slot 1 from the grid
//                       of rx antenna 0 and from the estimates of ports 0 .. nant - 1 through the cell's RE table
//                       (srsran_pbch_cp), equalises as the reference does for 240 / 216 symbols and one rx antenna --
//                       srsran_predecoding_single's vector body (1 port, precoding.c:182-272: the noise estimate is
//                       added only when it is positive), srsran_predecoding_diversity2_sse (2 ports) or the generic
//                       SFBC + FSTD loop (4 ports, precoding.c:465-498) with srsran_layerdemap_diversity's order --
//                       and demaps QPSK softly (demod_soft.c:120-123) into the hypothesis' slot.
//   pbch_hyp_kernel     one 64-lane workgroup per (entry, nant, nb, dst, src): decode_frame (pbch.c:395-430).  The grid
//                       is 90 workgroups an entry whatever the object's history; those outside nb < frame_idx,
//                       src < frame_idx - nb and the object's port counts leave at once.  n = nb + 1 stored frames are
//                       descrambled at bit offset dst x nof_bits, the rest of the 40 ms period is SRSRAN_RX_NULL,
//                       srsran_rm_conv_rx from 4 nof_bits to 120, x float(1 / 2n), the AVX2 build's 16-bit
//                       quantisation, viterbi37_tb16 with lane = trellis state, CRC16 under the port mask, and the
//                       all-zero payload refused (pbch.c:374-393).
//   pbch_select_kernel  one workgroup per entry: the first accepted hypothesis in the reference's loop order (nant,
//                       nb, dst, src ascending), the result, and the object's state: the LLRs of the accepted port
//                       count (of the last one tried on a miss, pbch.c:497-511) go to history slot frame_idx - 1; the
//                       counter is reset on success; after a fourth miss the history moves down one frame and the
//                       counter becomes 3 (pbch.c:546-550).  With mib_rule also srsran_ue_mib_decode's miss counter.
//
// The reference stops at its first success.  Here every hypothesis runs and the first accepted one in the same order
// is taken, so the hypotheses the reference would have skipped change nothing observable: they write only their own
// result slot, which the selection does not read past the first success.
#include "pbch_kernel.h"

#include "ctrl_dev.h"
#include "viterbi_dev.h"

namespace srsran_amd {
namespace {

#pragma clang fp contract(off)

constexpr float NSQRT2 = -1.41421356237309504880f;  // (float)(-M_SQRT2)

// frames stored before this call, after srsran_ue_mib_decode's reset rule; at most 3 (pbch.c:547-550)
__device__ __forceinline__ uint32_t frames_before(const PbchEntry& e, uint32_t& miss)
{
  const PbchState s = *e.state;
  const bool      r = e.mib_rule && s.miss_cnt > 8;
  miss              = r ? 0u : s.miss_cnt;
  return min(r ? 0u : s.frame_idx, 3u);
}

__device__ __forceinline__ float2 sc(cpx x, float hh, bool dbl)
{
  if (dbl) {  // x / hh * M_SQRT2, the product in double (precoding.c:493-496)
    const double s2 = 1.41421356237309504880;
    return make_float2((float)((double)__fdiv_rn(x.r, hh) * s2), (float)((double)__fdiv_rn(x.i, hh) * s2));
  }
  const float s2 = 1.41421356237309504880f;  // _mm_set1_ps(M_SQRT2 / scaling), scaling = 1
  return make_float2(__fdiv_rn(x.r, hh) * s2, __fdiv_rn(x.i, hh) * s2);
}

// the NANT symbols of unit u (one symbol, an SFBC pair, or an SFBC + FSTD quadruple)
template <uint32_t NANT>
__device__ __forceinline__ void llr_unit(const PbchEntry& e, uint32_t u, float2* out)
{
  uint32_t gi[NANT];
  cpx      r[NANT];
  float2   d[NANT];
#pragma unroll
  for (uint32_t j = 0; j < NANT; j++) {
    gi[j] = e.re[NANT * u + j] - e.re_off;
    r[j]  = ldc(e.grid, gi[j]);
    gi[j] = gi[j] % e.ce_row;
  }
  if constexpr (NANT == 1) {
    const cpx   h  = ldc(e.ce, gi[0]);
    float       hh = h.r * h.r + h.i * h.i;
    const float n0 = *e.noise;
    if (n0 > 0.0f) {
      hh = hh + n0;
    }
    const cpx x = cmulf(r[0], conjf(h));
    d[0]        = make_float2(__fdiv_rn(x.r, hh), __fdiv_rn(x.i, hh));  // x 1 / scaling, scaling = 1
  } else if constexpr (NANT == 2) {
    const float2 *h0 = e.ce, *h1 = e.ce + e.ce_port;
    const cpx    h00 = ldc(h0, gi[0]), h01 = ldc(h0, gi[1]), h10 = ldc(h1, gi[0]), h11 = ldc(h1, gi[1]);
    const float  hh  = (h00.r * h00.r + h00.i * h00.i) + (h11.r * h11.r + h11.i * h11.i);
    const cpx    a0 = cmulf(conjf(h00), r[0]), b0 = cmulf(h11, conjf(r[1]));
    const cpx    a1 = cmulf(conjf(h01), r[1]), b1 = cmulf(h10, conjf(r[0]));
    d[0] = sc(cpx{a0.r + b0.r, a0.i + b0.i}, hh, false);
    d[1] = sc(cpx{a1.r - b1.r, a1.i - b1.i}, hh, false);
  } else {
    const cpx h0 = ldc(e.ce, gi[0]), h1 = ldc(e.ce + e.ce_port, gi[2]);
    const cpx h2 = ldc(e.ce + 2 * (size_t)e.ce_port, gi[0]), h3 = ldc(e.ce + 3 * (size_t)e.ce_port, gi[2]);
    const float hh02 = 0.0f + (((h0.r * h0.r + h0.i * h0.i) + h2.r * h2.r) + h2.i * h2.i);
    const float hh13 = 0.0f + (((h1.r * h1.r + h1.i * h1.i) + h3.r * h3.r) + h3.i * h3.i);
    const cpx a0 = cmulf(conjf(h0), r[0]), b0 = cmulf(h2, conjf(r[1]));
    const cpx a1 = cmulf(cpx{-h2.r, -h2.i}, conjf(r[0])), b1 = cmulf(conjf(h0), r[1]);
    const cpx a2 = cmulf(conjf(h1), r[2]), b2 = cmulf(h3, conjf(r[3]));
    const cpx a3 = cmulf(cpx{-h3.r, -h3.i}, conjf(r[2])), b3 = cmulf(conjf(h1), r[3]);
    d[0] = sc(cpx{0.0f + (a0.r + b0.r), 0.0f + (a0.i + b0.i)}, hh02, true);
    d[1] = sc(cpx{0.0f + (a1.r + b1.r), 0.0f + (a1.i + b1.i)}, hh02, true);
    d[2] = sc(cpx{0.0f + (a2.r + b2.r), 0.0f + (a2.i + b2.i)}, hh13, true);
    d[3] = sc(cpx{0.0f + (a3.r + b3.r), 0.0f + (a3.i + b3.i)}, hh13, true);
  }
#pragma unroll
  for (uint32_t j = 0; j < NANT; j++) {  // srsran_layerdemap_diversity: d[NANT u + j] = x_j[u]; then QPSK demapping
    out[NANT * u + j] = make_float2(d[j].x * NSQRT2, d[j].y * NSQRT2);
  }
}

}  // namespace

__global__ __launch_bounds__(256) void pbch_llr_kernel(const PbchEntry* __restrict__ entries)
{
  const PbchEntry& e = entries[blockIdx.y];
  const uint32_t   a = blockIdx.x;
  if (a >= e.nof_nant) {
    return;
  }
  const uint32_t nant = e.nant[a], nsym = e.nsym;
  float2*        out  = (float2*)(e.tr + (size_t)a * 2 * nsym);  // LLR pair of symbol i at out[i]
  for (uint32_t u = threadIdx.x; u < nsym / nant; u += blockDim.x) {
    if (nant == 1) {
      llr_unit<1>(e, u, out);
    } else if (nant == 2) {
      llr_unit<2>(e, u, out);
    } else {
      llr_unit<4>(e, u, out);
    }
  }
}

__global__ __launch_bounds__(64) void pbch_hyp_kernel(const PbchEntry* __restrict__ entries)
{
  __shared__ float    rm[120];
  __shared__ uint16_t sym[120];
  __shared__ uint64_t dec[5 * 40 + 6];
  __shared__ uint8_t  data[40];
  __shared__ uint8_t  dcb[CTRL_NCOLS];

  const PbchEntry& e = entries[blockIdx.y];
  const uint32_t   a = blockIdx.x / PBCH_FRAME_HYP;
  if (a >= e.nof_nant) {
    return;
  }
  uint32_t nb, dst, src, miss;
  pbch_hyp_decode(blockIdx.x % PBCH_FRAME_HYP, nb, dst, src);
  const uint32_t fi = frames_before(e, miss) + 1;  // pbch.c:485
  if (!pbch_hyp_valid(fi, nb, src)) {
    return;
  }
  const int       lane  = threadIdx.x;
  const uint32_t  nbits = 2 * e.nsym, n = nb + 1, nant = e.nant[a];
  const float*    hist  = e.hist;
  const float*    cur   = e.tr + (size_t)a * nbits;  // the frame this call received, equalised for nant ports
  const uint32_t* seq   = e.seq;

  // temp[] of decode_frame, never stored: frames dst .. dst + n - 1 of the period hold stored frames src .. src + n - 1
  // descrambled at their bit offset (scrambling.c: x * c, c = +-1); every other frame is SRSRAN_RX_NULL
  auto temp = [=](int k) -> float {
    const uint32_t f = (uint32_t)k / nbits, i = (uint32_t)k - f * nbits;
    if (f < dst || f >= dst + n) {
      return CTRL_RX_NULL;
    }
    const uint32_t fr = src + (f - dst);
    float          v  = fr == fi - 1 ? cur[i] : hist[fr * nbits + i];
    if ((seq[k >> 5] >> (k & 31)) & 1u) {
      v = v * -1.0f;
    }
    return v;
  };
  rm_conv_rx_gather(120, 4 * nbits, temp, rm, dcb, lane);
  const float norm = (float)(1.0 / (double)((float)2 * n));  // pbch.c:416
  for (uint32_t i = lane; i < 120; i += 64) {
    rm[i] = rm[i] * norm;
  }
  __syncthreads();
  vit_quantise(rm, 120, sym, lane);
  viterbi37_tb16(sym, 40, dec, data, lane);
  if (lane == 0) {  // srsran_pbch_crc_check: LTE CRC16 of the payload against the parity under srsran_crc_mask
    uint32_t crc = 0, any = 0;
    for (uint32_t i = 0; i < 24; i++) {
      const uint32_t fb = ((crc >> 15) & 1u) ^ data[i];
      crc               = (crc << 1) & 0xffffu;
      if (fb) {
        crc ^= 0x1021u;
      }
      any |= data[i];
    }
    uint32_t p = 0;
    for (int i = 0; i < 16; i++) {
      p = (p << 1) | data[24 + i];
    }
    const uint32_t mask         = nant == 2 ? 0xffffu : nant == 4 ? 0x5555u : 0u;
    e.hyp[blockIdx.x].ok        = ((p ^ mask) == crc && any) ? 1u : 0u;
  }
  if (lane < 24) {
    e.hyp[blockIdx.x].bits[lane] = data[lane];
  }
}

__global__ __launch_bounds__(64) void pbch_select_kernel(const PbchEntry* __restrict__ entries, PbchOut* __restrict__ outs)
{
  __shared__ int sel;
  const PbchEntry& e    = entries[blockIdx.x];
  const uint32_t   lane = threadIdx.x, nbits = 2 * e.nsym;
  uint32_t         miss;
  const uint32_t   fi = frames_before(e, miss) + 1;
  if (lane == 0) {
    int s = -1;
    for (uint32_t h = 0; h < e.nof_nant * PBCH_FRAME_HYP && s < 0; h++) {
      uint32_t nb, dst, src;
      pbch_hyp_decode(h % PBCH_FRAME_HYP, nb, dst, src);
      if (pbch_hyp_valid(fi, nb, src) && e.hyp[h].ok) {
        s = (int)h;
      }
    }
    sel = s;
  }
  __syncthreads();
  const int      s = sel;
  const uint32_t a = s >= 0 ? (uint32_t)s / PBCH_FRAME_HYP : e.nof_nant - 1;
  // history: this frame into slot fi - 1; after a fourth miss every column moves down one frame (a lane owns its
  // columns, so the move needs no synchronisation)
  const float* cur = e.tr + (size_t)a * nbits;
  for (uint32_t i = lane; i < nbits; i += 64) {
    e.hist[(fi - 1) * nbits + i] = cur[i];
    if (s < 0 && fi == 4) {
      for (uint32_t f = 0; f < 3; f++) {
        e.hist[f * nbits + i] = e.hist[(f + 1) * nbits + i];
      }
    }
  }
  if (lane < 24) {
    outs[blockIdx.x].payload[lane] = s >= 0 ? e.hyp[s].bits[lane] : 0;
  }
  if (lane == 0) {
    PbchOut* o = outs + blockIdx.x;
    if (s >= 0) {
      uint32_t nb, dst, src;
      pbch_hyp_decode((uint32_t)s % PBCH_FRAME_HYP, nb, dst, src);
      o->found        = 1;
      o->nof_tx_ports = e.nant[a];
      o->sfn_offset   = (int32_t)dst - (int32_t)src + (int32_t)fi - 1;
      e.state->frame_idx = 0;
      e.state->miss_cnt  = e.mib_rule ? 0u : miss;
    } else {
      o->found           = 0;
      o->nof_tx_ports    = 0;
      o->sfn_offset      = 0;
      e.state->frame_idx = fi == 4 ? 3u : fi;
      e.state->miss_cnt  = e.mib_rule ? miss + 1 : miss;
    }
  }
}

hipError_t pbch_llr_launch(const PbchEntry* d_entries, uint32_t n, hipStream_t stream)
{
  if (n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pbch_llr_kernel, dim3(PBCH_NANT_HYP, n), dim3(256), 0, stream, d_entries);
  return hipGetLastError();
}

hipError_t pbch_hyp_launch(const PbchEntry* d_entries, uint32_t n, hipStream_t stream)
{
  if (n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pbch_hyp_kernel, dim3(PBCH_HYP, n), dim3(64), 0, stream, d_entries);
  return hipGetLastError();
}

hipError_t pbch_select_launch(const PbchEntry* d_entries, uint32_t n, PbchOut* d_out, hipStream_t stream)
{
  if (n == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pbch_select_kernel, dim3(n), dim3(64), 0, stream, d_entries, d_out);
  return hipGetLastError();
}

}  // namespace srsran_amd
