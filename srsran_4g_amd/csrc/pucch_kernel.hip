// srsran_4g_amd/csrc/pucch_kernel.hip -- PUCCH receive for gfx950: formats 1/1a/1b/2/2a/2b/3.
//
// One candidate (UE, resource, hypothesis pass) is a few hundred REs, so each runs as one 64-lane
// workgroup that keeps everything in registers and ~3 KB of LDS; the grid is the candidates of the
// whole batch.  Per candidate, as chest_ul.c:462-610 and pucch.c:506-567, 625-872:
//   1. gather the DMRS REs, least squares against r_u,v(alpha) w-bar (for 2a / 2b the 2 / 4 d(10)
//      hypotheses, ">=" so the last maximum wins)
//   2. EPRE / RSRP, TA from the per-symbol lag-1 correlation, slot average over the n_rs symbols,
//      3-tap smoothing with the extrapolated edges of srsran_conv_same_cf, noise from smoothed
//      minus raw (symbol 0 of each slot holds the slot average by then, as in the reference)
//   3. gather the data REs, srsran_predecoding_single with the noise estimate
//   4. optional DMRS detection on the first 12 estimates
//   5. format 1x: correlation with the 1 / 2 / 4 hypotheses (first maximum); format 2x: despread,
//      int16 QPSK demap, descramble, ML over the (20, A) code with the reference's integer widths;
//      format 3: 12-point DFT per symbol, w_n_oc / cell shift de-spreading, 48 LLRs, (32, O) ML.
// Every reduction is a fixed xor-shuffle tree or a fixed-order loop of one lane: no atomics, a
// result never depends on what else is in the batch.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_dev.h"
#include "pucch_kernel.h"

namespace srsran_amd {
namespace {

enum { F1 = 0, F1A, F1B, F2, F2A, F2B, F3 };

struct c2 {
  float r, i;
};
__device__ __forceinline__ c2 mk(float2 v) { return {v.x, v.y}; }
__device__ __forceinline__ float2 f2(c2 v) { return make_float2(v.r, v.i); }
__device__ __forceinline__ c2 add(c2 a, c2 b) { return {a.r + b.r, a.i + b.i}; }
__device__ __forceinline__ c2 sub(c2 a, c2 b) { return {a.r - b.r, a.i - b.i}; }
__device__ __forceinline__ c2 mul(c2 a, c2 b) { return {a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
__device__ __forceinline__ c2 mulconj(c2 a, c2 b) { return {a.r * b.r + a.i * b.i, a.i * b.r - a.r * b.i}; }  // a conj(b)
__device__ __forceinline__ c2 scl(c2 a, float s) { return {a.r * s, a.i * s}; }
__device__ __forceinline__ float nrm(c2 a) { return a.r * a.r + a.i * a.i; }
// a * j^q
__device__ __forceinline__ c2 rot90(c2 a, uint32_t q)
{
  switch (q & 3u) {
    case 1:
      return {-a.i, a.r};
    case 2:
      return {-a.r, -a.i};
    case 3:
      return {a.i, -a.r};
    default:
      return a;
  }
}

// cos(pi k / 12), k = 0..6
__constant__ float kCos12[7] = {1.0f, 0.96592582628906829f, 0.86602540378443865f, 0.70710678118654752f,
                                0.5f, 0.25881904510252076f, 0.0f};
// (20, A) basis sequences, 36.212 Table 5.2.3.3-1: bit 12 - n of word i is M_{i,n}
__constant__ uint16_t kCqiBasis[20] = {0b1100000000110, 0b1110000001110, 0b1001001011111, 0b1011000010111,
                                       0b1111000100111, 0b1100101110111, 0b1010101011111, 0b1001100110111,
                                       0b1101100101111, 0b1011101001111, 0b1010011101111, 0b1110011010111,
                                       0b1001010111111, 0b1101010101111, 0b1000110100101, 0b1100111101101,
                                       0b1110111001011, 0b1001110010011, 0b1101111100000, 0b1000011000000};

// exp(j pi k / 12)
__device__ __forceinline__ c2 tw24(int k)
{
  k %= 24;
  k += k < 0 ? 24 : 0;
  const int r = k % 6;
  return rot90(c2{kCos12[r], kCos12[6 - r]}, (uint32_t)(k / 6));
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v += __shfl_xor(v, off, 64);
  }
  return v;
}

// x86 float -> int32 conversion (out of range or NaN: INT32_MIN), then the 16-bit pack
__device__ __forceinline__ int32_t cvt_tz(float x) { return __builtin_fabsf(x) < 2147483648.0f ? (int32_t)x : INT32_MIN; }
__device__ __forceinline__ int16_t sat16(int32_t v) { return (int16_t)max(-32768, min(32767, v)); }
__device__ __forceinline__ int16_t wrap16(int32_t v) { return (int16_t)(uint16_t)(uint32_t)v; }

// srsran_demod_soft_demodulate_s(QPSK) value `idx` of `n` (srsran_vec_convert_fi: the 16-value
// vector body saturates, the scalar tail wraps), then srsran_scrambling_s with bit c
__device__ __forceinline__ int16_t qpsk_llr(float v, uint32_t idx, uint32_t n, uint32_t c)
{
  const float   scale = (float)(-100.0 * 1.41421356237309504880);
  const int32_t t     = cvt_tz(v * scale);
  const int16_t l     = idx < 16 * (n / 16) ? sat16(t) : wrap16(t);
  return c ? wrap16(-(int32_t)l) : l;
}

// d(10) of 2a / 2b for hypothesis i (bits[0] = i % 2, bits[1] = i / 2), as a power of j
__device__ __forceinline__ uint32_t d10_rot(uint32_t format, uint32_t i)
{
  if (format == F2A) {
    return (i & 1u) ? 2u : 0u;
  }
  const uint32_t b0 = i & 1u, b1 = i >> 1;
  return b0 ? (b1 ? 2u : 1u) : (b1 ? 3u : 0u);  // 00: 1, 01: -j, 10: j, 11: -1
}

__global__ __launch_bounds__(64) void pucch_kernel(const PucchCand* __restrict__ cands, PucchCandOut* __restrict__ outs)
{
  const PucchCand& d    = cands[blockIdx.x];
  const uint32_t   lane = threadIdx.x;
  __shared__ float2  pe[2 * PUCCH_MAX_RS * 12];  // least-squares estimates per DMRS symbol
  __shared__ float2  av[24];                     // slot averages
  __shared__ float2  hs[24];                     // smoothed estimate of each slot's PRB
  __shared__ float2  zs[PUCCH_MAX_RE];           // equalised data REs
  __shared__ float2  ys[PUCCH_MAX_RE];
  __shared__ int16_t llr[48];
  __shared__ int16_t acc32[32];
  __shared__ uint8_t bits[16];

  const uint32_t format = d.format, n_rs = d.n_rs, nrefs = 2 * n_rs * 12;
  const uint32_t n_sf0 = d.n_sf[0], nre = (d.n_sf[0] + d.n_sf[1]) * 12;
  PucchCandOut   o;
  o.epre = o.rsrp = o.ta_us = o.corr = o.dmrs_corr = 0.0f;
  o.noise        = d.noise_in;
  o.dmrs_checked = o.dmrs_failed = o.found = 0;
  o.drs_bits[0] = o.drs_bits[1] = 0;
  if (lane < 16) {
    bits[lane] = 0;
  }

  if (!d.compact) {
    // ---- least squares; the m == 1 symbols (which carry d(10) in 2a / 2b) are summed apart
    float s0r = 0.f, s0i = 0.f, s1r = 0.f, s1i = 0.f, pw = 0.f;
    for (uint32_t k = lane; k < nrefs; k += 64) {
      const uint32_t s = k / (n_rs * 12), m = (k / 12) % n_rs, n = k % 12;
      const c2 rx = mk(d.grid[(size_t)(s * d.nsym_slot + d.rs_sym[m]) * d.ncell_re + d.n_prb[s] * 12 + n]);
      const int ph = 3 * (int)d.phi[s][n] + 2 * (int)d.rs_ncs[s][m] * (int)n + (int)d.rs_ph[s][m];
      const c2  e  = mulconj(rx, tw24(ph));
      pe[k]        = f2(e);
      if (m == 1) {
        s1r += e.r, s1i += e.i;
      } else {
        s0r += e.r, s0i += e.i;
      }
      pw += nrm(e);
    }
    s0r = wave_sum(s0r), s0i = wave_sum(s0i), s1r = wave_sum(s1r), s1i = wave_sum(s1i), pw = wave_sum(pw);
    __syncthreads();
    c2 sum = {s0r + s1r, s0i + s1i};
    if (format == F2A || format == F2B) {
      const uint32_t nh   = format == F2A ? 2u : 4u;
      float          mx   = -1e9f;
      uint32_t       imax = 0;
      for (uint32_t i = 0; i < nh; i++) {
        const c2    t = rot90(c2{s1r, s1i}, 4u - d10_rot(format, i));  // conj(d(10)) * sum
        const float x = hypotf(s0r + t.r, s0i + t.i);
        if (x >= mx) {
          mx   = x;
          imax = i;
        }
      }
      const uint32_t rq = 4u - d10_rot(format, imax);
      for (uint32_t k = lane; k < nrefs; k += 64) {
        if ((k / 12) % n_rs == 1) {
          pe[k] = f2(rot90(mk(pe[k]), rq));
        }
      }
      const c2 t    = rot90(c2{s1r, s1i}, rq);
      sum           = c2{s0r + t.r, s0i + t.i};
      o.drs_bits[0] = (uint8_t)(imax % 2);
      o.drs_bits[1] = (uint8_t)(imax / 2);
      __syncthreads();
    }
    const float nr = (float)nrefs;
    const float cr = sum.r / nr, ci = sum.i / nr;
    o.epre = pw / nr;
    o.rsrp = fminf(cr * cr + ci * ci, o.epre);

    // ---- time alignment: srsran_vec_estimate_frequency of each DMRS symbol, averaged
    if (d.meas_ta) {
      float ta = 0.0f;
      for (uint32_t sym = 0; sym < 2 * n_rs; sym++) {
        c2 c = {0.f, 0.f};
        if (lane >= 1 && lane < 12) {
          c = mulconj(mk(pe[sym * 12 + lane]), mk(pe[sym * 12 + lane - 1]));
        }
        const float ar = wave_sum(c.r), ai = wave_sum(c.i);
        const float f  = (float)((double)-atan2f(ai, ar) * 0.31830988618379067154 * 0.5);
        ta += f / (float)(2 * n_rs);
      }
      if (isnormal(ta)) {
        ta /= 15e3f;
        ta *= 1e6f;
        ta = roundf(ta * 10.0f) / 10.0f;
      } else {
        ta = 0.0f;
      }
      o.ta_us = ta;
    }

    // ---- slot average (kept in the slot's first symbol, as the reference does in place)
    if (lane < 24) {
      const uint32_t s = lane / 12, n = lane % 12;
      c2             a = mk(pe[(s * n_rs) * 12 + n]);
      for (uint32_t i = 1; i < n_rs; i++) {
        a = add(a, mk(pe[(s * n_rs + i) * 12 + n]));
      }
      a        = scl(a, 1.0f / (float)n_rs);
      av[lane] = f2(a);
    }
    __syncthreads();
    // ---- 3-tap smoothing, edges extrapolated as srsran_conv_same_cf does
    if (lane < 24) {
      const uint32_t s = lane / 12, n = lane % 12;
      const float2*  p = av + s * 12;
      const c2       x = mk(p[n]);
      const c2       l = n == 0 ? sub(scl(mk(p[1]), 3.0f), scl(mk(p[0]), 2.0f)) : mk(p[n - 1]);
      const c2       r = n == 11 ? sub(scl(mk(p[11]), 3.0f), scl(mk(p[10]), 2.0f)) : mk(p[n + 1]);
      hs[lane]         = f2(add(add(scl(l, d.filt[0]), scl(x, d.filt[1])), scl(r, d.filt[2])));
    }
    __syncthreads();
    if (d.ce) {
      for (uint32_t k = lane; k < 2 * d.nsym_slot * 12; k += 64) {
        const uint32_t s = k / (d.nsym_slot * 12), i = (k / 12) % d.nsym_slot, n = k % 12;
        d.ce[(size_t)(s * d.nsym_slot + i) * d.ncell_re + d.n_prb[s] * 12 + n] = hs[s * 12 + n];
      }
    }
    // ---- noise: smoothed minus noisy estimates of every DMRS symbol
    float np = 0.f;
    for (uint32_t k = lane; k < nrefs; k += 64) {
      const uint32_t s = k / (n_rs * 12), m = (k / 12) % n_rs, n = k % 12;
      const c2       noisy = m == 0 ? mk(av[s * 12 + n]) : mk(pe[k]);
      np += nrm(sub(mk(hs[s * 12 + n]), noisy));
    }
    np                = wave_sum(np);
    const float power = np / 12.0f / (float)(2 * n_rs);
    float       noise = (float)((double)power / d.noise_div);
    if (noise == 0.0f) {
      noise = FLT_MIN;
    }
    o.noise = noise;
  }

  if (d.do_decode) {
    // ---- pucch_get + srsran_predecoding_single (the 8-wide body adds the noise only when it is
    // positive, the scalar tail always)
    const uint32_t nvec = 8 * (nre / 8);
    for (uint32_t k = lane; k < nre; k += 64) {
      c2 y, h;
      if (d.compact) {
        y = mk(d.grid[k]);
        h = mk(d.ce_in[k]);
      } else {
        const uint32_t s = k >= n_sf0 * 12 ? 1u : 0u, kk = k - s * n_sf0 * 12, i = kk / 12, n = kk % 12;
        y = mk(d.grid[(size_t)(s * d.nsym_slot + d.data_sym[i]) * d.ncell_re + d.n_prb[s] * 12 + n]);
        h = mk(hs[s * 12 + n]);
      }
      const float hh = nrm(h);
      const float dn = k < nvec ? (o.noise > 0.0f ? hh + o.noise : hh) : hh + o.noise;
      const c2    z  = mulconj(y, h);
      zs[k]          = make_float2(z.r / dn, z.i / dn);
    }
    __syncthreads();

    // ---- DMRS detection on the first 12 estimates
    bool go = true;
    if (isnormal(d.thr_dmrs)) {
      c2 h = {0.f, 0.f};
      if (lane < 12) {
        h = d.compact ? mk(d.ce_in[lane]) : mk(hs[lane]);
      }
      const float sr = wave_sum(h.r) / 12.0f, si = wave_sum(h.i) / 12.0f;
      const float power = wave_sum(nrm(h)) / 12.0f;
      o.dmrs_corr       = (sr * sr + si * si) / power;
      o.dmrs_checked    = 1;
      if (!isnormal(o.dmrs_corr) || o.dmrs_corr < d.thr_dmrs) {
        o.dmrs_failed = 1;
        go            = false;
      }
    }

    if (go && format <= F1B) {
      float sr = 0.f, si = 0.f, px = 0.f;
      for (uint32_t k = lane; k < nre; k += 64) {
        const uint32_t s = k >= n_sf0 * 12 ? 1u : 0u, kk = k - s * n_sf0 * 12, i = kk / 12, n = kk % 12;
        const int ph = 3 * (int)d.phi[s][n] + 2 * (int)d.data_ncs[s][i] * (int)n + (int)d.data_ph[s][i];
        const c2  z  = mk(zs[k]);
        const c2  c  = mulconj(z, tw24(ph));
        sr += c.r, si += c.i, px += nrm(z);
      }
      sr = wave_sum(sr), si = wave_sum(si), px = wave_sum(px);
      const float len = (float)nre;
      const float den = sqrtf((px / len) * 1.0f);  // the hypothesis has unit power
      const float cre = (sr / len) / den, cim = (si / len) / den;
      if (format == F1) {
        o.corr  = cre;
        o.found = cre >= d.thr_format1;
      } else {
        // Re(conj(d(0)) S) of d(0) = 1, -j, j, -1 in the reference's order; strict ">": first maximum
        const float    h4[4] = {cre, -cim, cim, -cre};
        const uint32_t nh    = format == F1A ? 2u : 4u;
        float          cm    = -1e9f;
        uint32_t       bm    = 0;
        for (uint32_t b = 0; b < nh; b++) {
          const float c = format == F1A ? (b ? -cre : cre) : h4[b];
          if (c > cm) {
            cm = c;
            bm = b;
          }
        }
        o.corr  = cm;
        o.found = cm > d.thr_format1;
        if (lane == 0) {
          if (format == F1A) {
            bits[0] = (uint8_t)bm;
          } else {
            bits[0] = (uint8_t)(bm >> 1);
            bits[1] = (uint8_t)(bm & 1u);
          }
        }
      }
    } else if (go && format <= F2B) {
      for (uint32_t k = lane; k < 120; k += 64) {
        const uint32_t s = k / 60, i = (k / 12) % 5, n = k % 12;
        const int      ph = 3 * (int)d.phi[s][n] + 2 * (int)d.data_ncs[s][i] * (int)n;
        ys[k]             = f2(mulconj(mk(zs[k]), tw24(ph)));
      }
      __syncthreads();
      if (lane < 10) {
        c2 a = {0.f, 0.f};
        for (uint32_t n = 0; n < 12; n++) {
          a = add(a, mk(ys[lane * 12 + n]));
        }
        a.r /= 12.0f, a.i /= 12.0f;
        llr[2 * lane]     = qpsk_llr(a.r, 2 * lane, 20, (uint32_t)(d.scr >> (2 * lane)) & 1u);
        llr[2 * lane + 1] = qpsk_llr(a.i, 2 * lane + 1, 20, (uint32_t)(d.scr >> (2 * lane + 1)) & 1u);
      }
      __syncthreads();
      float lp = 0.0f;
      for (uint32_t i = 0; i < 20; i++) {
        const float t = (float)llr[i];
        lp += t * t;
      }
      lp /= 20.0f;
      o.found = 1;
      if (isnormal(lp)) {
        const float rms = sqrtf(lp) * 20.0f;
        int32_t     mc;
        uint32_t    mw = 0;
        const uint32_t A = d.nof_uci_bits;
        if (A < 13) {  // srsran_uci_decode_cqi_pucch: codewords with stride 1 << (13 - A)
          mc = INT32_MIN;
          for (uint32_t idx = lane; idx < (1u << A); idx += 64) {
            const uint32_t w = idx << (13 - A);
            int32_t        c = 0;
            for (uint32_t j = 0; j < 20; j++) {
              const int32_t sgn = (int32_t)(__builtin_popcount(w & kCqiBasis[j]) & 1) * 2 - 1;
              const int32_t p   = sgn * (int32_t)llr[j];
              c += j < 16 ? (int32_t)wrap16(p) : p;  // the 16-bit lanes of srsran_vec_dot_prod_sss
            }
            if (c > mc) {
              mc = c;
              mw = w;
            }
          }
          for (int off = 32; off > 0; off >>= 1) {
            const int32_t  oc = __shfl_xor(mc, off, 64);
            const uint32_t ow = (uint32_t)__shfl_xor((int)mw, off, 64);
            if (oc > mc || (oc == mc && ow < mw)) {
              mc = oc;
              mw = ow;
            }
          }
          if (lane < 13) {
            bits[lane] = (uint8_t)((mw >> (12 - lane)) & 1u);
          }
        } else {
          mc = -2;  // SRSRAN_ERROR_INVALID_INPUTS, nothing decoded
        }
        o.corr = (float)wrap16(mc) / rms;  // the reference returns its 32-bit maximum as int16_t
      } else {
        o.corr = 0.0f;
      }
    } else if (go && format == F3) {
      const uint32_t nsym = d.n_sf[0] + d.n_sf[1];
      for (uint32_t k = lane; k < nsym * 12; k += 64) {
        const uint32_t n = k / 12, kk = k % 12;
        c2             a = {0.f, 0.f};
        for (uint32_t i = 0; i < 12; i++) {
          a = add(a, mul(mk(zs[n * 12 + i]), tw24((int)(2 * i * kk))));
        }
        const float sq = sqrtf(12.0f);
        ys[k]          = make_float2(a.r / sq, a.i / sq);
      }
      __syncthreads();
      if (lane < 24) {
        const uint32_t sl = lane / 12, j = lane % 12, n0 = sl ? n_sf0 : 0u;
        c2             a  = {0.f, 0.f};
        for (uint32_t t = 0; t < d.n_sf[sl]; t++) {
          const uint32_t ncs = d.data_ncs[sl][t], i = (j + 12 - ncs % 12) % 12;
          c2             w;
          if (sl == 0 || d.n_sf[1] == 5) {  // exp(j 2 pi n_oc t / 5)
            float sn, cs;
            sincospif(0.4f * (float)((d.f3_noc[sl] * t) % 5), &sn, &cs);
            w = c2{cs, sn};
          } else {  // the +-1 sequences of length 4
            w = c2{(__builtin_popcount(d.f3_noc[1] & t) & 1) ? -1.0f : 1.0f, 0.0f};
          }
          a = add(a, mul(rot90(w, 4u - (ncs / 64) % 4u), mk(ys[(n0 + t) * 12 + i])));
        }
        a = scl(a, 2.0f / (float)nsym);
        llr[2 * lane]     = qpsk_llr(a.r, 2 * lane, 48, (uint32_t)(d.scr >> (2 * lane)) & 1u);
        llr[2 * lane + 1] = qpsk_llr(a.i, 2 * lane + 1, 48, (uint32_t)(d.scr >> (2 * lane + 1)) & 1u);
      }
      __syncthreads();
      if (lane < 32) {  // srsran_block_decode_i16: the 32-periodic copies summed with 16-bit wrap
        acc32[lane] = wrap16((int32_t)llr[lane] + (lane < 16 ? (int32_t)llr[32 + lane] : 0));
      }
      __syncthreads();
      const int32_t corr = block_ml(acc32, 11, bits, (int)lane);
      o.corr             = (float)corr / 4800.0f;
      o.found            = o.corr > d.thr_format3;
    }
  }
  __syncthreads();
  if (lane == 0) {
    for (int i = 0; i < 16; i++) {
      o.bits[i] = bits[i];
    }
    outs[blockIdx.x] = o;
  }
}

}  // namespace

hipError_t pucch_launch(const PucchCand* d_cand, PucchCandOut* d_out, uint32_t ncand, hipStream_t stream)
{
  if (ncand == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pucch_kernel, dim3(ncand), dim3(64), 0, stream, d_cand, d_out);
  return hipGetLastError();
}

}  // namespace srsran_amd
