// srsran_4g_amd/csrc/prach_kernel.hip -- PRACH preamble detection and generation for CDNA4.
//
// srsran_prach_detect_offset (prach.c:969-1012, srsran_prach_process 870-967) takes one 12 N-point DFT of the
// received window, keeps 839 bins of it, and for every root sequence multiplies them by the conjugate of the
// root's transform, takes an 839-point inverse DFT and searches |.|^2 window by window.
//
// prach_bins_kernel: only 839 of the 12 N bins are wanted, so the long transform is never formed.  With
// n = n1 + 12 n2, X[k] = sum_{n1 < 12} W_{12N}^{n1 k} F_{n1}[k mod N], F_{n1} the N-point DFT of x[n1 + 12 n2]:
// one workgroup per (occasion, n1) runs ofdm_kernel.hip's Stockham stages in LDS and writes its twiddled term of
// the 839 bins; the twelve terms are added in the order n1 = 0..11 by the search kernel (no atomics: a result does
// not depend on what else is in the batch).
//
// prach_search_kernel: one workgroup per (occasion, root).  839 is prime; the inverse DFT is the direct sum over
// an exact 839-entry table (704 k complex MACs a root, all in LDS), one output a thread, accumulated in double.
// Then the lag-1 product sum (prach.c:890), |.|^2, its mean by a fixed tree and, one wave per window, the first
// maximum (strict >, prach.c:917-926).  The threshold compare and the index / offset arithmetic are the host's.
//
// prach_seq_dft_kernel: the forward 839-point DFT of the sequences, scaled by 1 / sqrt(839) (prach.c:574-578).
// prach_gen_kernel (prach.c:749-793): the decomposition backwards -- per n1 the 839 bins folded mod N with their
// twiddles, an inverse N-point FFT, out[12 n2 + n1]; the cyclic prefix and the repetition of formats 2 / 3 are
// written with it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prach_kernel.h"
#include "fft_stockham.h"

namespace srsran_amd {

static constexpr int PRACH_THREADS = OFDM_THREADS;  // the Stockham stages are written for this workgroup size

__global__ __launch_bounds__(PRACH_THREADS) void prach_bins_kernel(const PrachOcc* __restrict__ occ,
                                                                   float2* __restrict__ part)
{
  __shared__ float2 buf[OFDM_MAX_N];
  const PrachOcc&   d  = occ[blockIdx.y];
  const uint32_t    n1 = blockIdx.x, N = d.fft.N, M = PRACH_K * N, b0 = d.b0;
  const float2*     sig = d.sig;
  const float2*     twm = d.tw_m;
  for (uint32_t n2 = threadIdx.x; n2 < N; n2 += PRACH_THREADS) {
    buf[n2] = sig[n1 + PRACH_K * n2];
  }
  __syncthreads();
  fft_ip(buf, d.fft);
  float2* dst = part + ((size_t)blockIdx.y * PRACH_K + n1) * PRACH_NZC;
  for (uint32_t k = threadIdx.x; k < PRACH_NZC; k += PRACH_THREADS) {
    uint32_t kk = b0 + k;  // b0 < M and 839 < M
    if (kk >= M) {
      kk -= M;
    }
    dst[k] = cmul(buf[kk % N], twm[(n1 * kk) % M]);
  }
}

// The 839-point kernels: one output per thread (839 of 1024 lanes), so a root's transform is sixteen short wave
// programs instead of four long ones (the single-occasion call's latency is one workgroup's).
static constexpr int PRACH_DFT_THREADS = 1024;

// y[n] = sum_k c[k] tw[(k n) mod 839]; c holds 840 entries, the last one zero.  Products and sums in double (c kept as
// doubles in LDS: its reads are broadcasts; the twiddle table as floats, converted after the gather, which halves the
// bytes the gathers move: 87 against 96 us for one root on the MI355X): an 839-term float sum would carry about sqrt(839) roundings
// where the reference's FFT carries about log2(839), and CDNA4's FP64 FMA rate is half its FP32 rate.  Even and odd k
// go to separate accumulators (two independent FMA chains per component).
__device__ __forceinline__ float2 dft839(const double2* c, const float2* tw, uint32_t n)
{
  uint32_t idx = 0;
  double   re0 = 0.0, im0 = 0.0, re1 = 0.0, im1 = 0.0;
  for (uint32_t k = 0; k < PRACH_NZC + 1; k += 2) {
    const double2 c0 = c[k], c1 = c[k + 1];
    const float2 f0 = tw[idx];
    idx += n;
    idx = idx >= PRACH_NZC ? idx - PRACH_NZC : idx;
    const float2 f1 = tw[idx];
    idx += n;
    idx = idx >= PRACH_NZC ? idx - PRACH_NZC : idx;
    const double2 w0 = make_double2((double)f0.x, (double)f0.y), w1 = make_double2((double)f1.x, (double)f1.y);
    re0 = fma(c0.x, w0.x, re0);
    im0 = fma(c0.x, w0.y, im0);
    re1 = fma(c1.x, w1.x, re1);
    im1 = fma(c1.x, w1.y, im1);
    re0 = fma(-c0.y, w0.y, re0);
    im0 = fma(c0.y, w0.x, im0);
    re1 = fma(-c1.y, w1.y, re1);
    im1 = fma(c1.y, w1.x, im1);
  }
  return make_float2((float)(re0 + re1), (float)(im0 + im1));
}

// sum of red[0..1023] by a fixed tree, result in red[0] (barriers included)
__device__ __forceinline__ void tree_sum(float2* red)
{
  for (uint32_t s = PRACH_DFT_THREADS / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[threadIdx.x] = cadd(red[threadIdx.x], red[threadIdx.x + s]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PRACH_DFT_THREADS) void prach_search_kernel(const PrachOcc* __restrict__ occ,
                                                                         const float2* __restrict__ part,
                                                                         const float2* __restrict__ tw839,
                                                                         PrachOccOut* __restrict__ out)
{
  __shared__ double2 c[PRACH_NZC + 1];
  __shared__ float2  tw[PRACH_NZC];
  __shared__ float   corr[PRACH_NZC];
  __shared__ float2  red[PRACH_DFT_THREADS];
  const uint32_t     o = blockIdx.y, r = blockIdx.x;
  const PrachOcc&    d = occ[o];
  if (r >= d.n_roots || r >= PRACH_MAX_ROOTS) {  // uniform over the workgroup
    return;
  }
  const uint32_t n_cs = d.n_cs, n_wins = d.n_wins, k = threadIdx.x;
  float2         ck = make_float2(0.f, 0.f);
  if (k < PRACH_NZC) {
    const float2* p  = part + (size_t)o * PRACH_K * PRACH_NZC;
    const float2* rs = d.root_spec + (size_t)d.root_idx[r] * PRACH_NZC;
    float2        s  = p[k];
#pragma unroll
    for (uint32_t n1 = 1; n1 < PRACH_K; n1++) {
      s = cadd(s, p[n1 * PRACH_NZC + k]);
    }
    s               = make_float2(s.x * d.scale, s.y * d.scale);
    const float2 q  = rs[k];
    ck              = make_float2(s.x * q.x + s.y * q.y, s.y * q.x - s.x * q.y);  // bins conj(root_spec), in float
    const float2 w  = tw839[k];
    tw[k]           = w;
  }
  if (k <= PRACH_NZC) {
    c[k] = make_double2((double)ck.x, (double)ck.y);  // c[839] = 0
  }
  __syncthreads();
  {  // prach.c:890: cross[k] = c[k] conj(c[k+1]), k < 838, summed (prach.c:851)
    float2 acc = make_float2(0.f, 0.f);
    if (k < PRACH_NZC - 1) {
      const float2 y = make_float2((float)c[k + 1].x, (float)c[k + 1].y);
      acc            = make_float2(ck.x * y.x + ck.y * y.y, ck.y * y.x - ck.x * y.y);
    }
    red[k] = acc;
    __syncthreads();
    tree_sum(red);
    if (k == 0) {
      out[o].cross[r] = red[0];
    }
    __syncthreads();
  }
  float v = 0.f;
  if (k < PRACH_NZC) {
    const float2 y = dft839(c, tw, k);
    v              = y.x * y.x + y.y * y.y;
    corr[k]        = v;
  }
  red[k] = make_float2(v, 0.f);
  __syncthreads();
  tree_sum(red);
  if (k == 0) {
    out[o].avg[r] = red[0].x / (float)PRACH_NZC;
  }
  // one wave per window: every lane's first maximum, then the larger value (the smaller offset on a tie)
  const uint32_t wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const uint32_t winsize = n_cs ? n_cs : PRACH_NZC;
  for (uint32_t j = wave; j < n_wins; j += PRACH_DFT_THREADS / 64) {
    const uint32_t start = (PRACH_NZC - j * n_cs) % PRACH_NZC;  // j n_cs < 839: start + winsize <= 839
    float          best  = 0.f;
    uint32_t       bi    = 0;
    for (uint32_t i = lane; i < winsize && start + i < PRACH_NZC; i += 64) {
      const float x = corr[start + i];
      if (x > best) {
        best = x;
        bi   = i;
      }
    }
    for (int s = 32; s > 0; s >>= 1) {
      const float    ov = __shfl_down(best, s, 64);
      const uint32_t oi = __shfl_down(bi, s, 64);
      if (ov > best || (ov == best && oi < bi)) {
        best = ov;
        bi   = oi;
      }
    }
    const uint32_t w = r * n_wins + j;
    if (lane == 0 && w < PRACH_MAX_WIN) {
      out[o].peak[w] = best;
      out[o].off[w]  = bi;
    }
  }
}

__global__ __launch_bounds__(PRACH_DFT_THREADS) void prach_seq_dft_kernel(const float2* __restrict__ seqs,
                                                                          const float2* __restrict__ tw839,
                                                                          float2* __restrict__ spec)
{
  __shared__ double2 c[PRACH_NZC + 1];
  __shared__ float2  tw[PRACH_NZC];
  const float2*      src = seqs + (size_t)blockIdx.x * PRACH_NZC;
  const uint32_t     k   = threadIdx.x;
  if (k < PRACH_NZC) {
    const float2 x = src[k], w = tw839[k];
    c[k]  = make_double2((double)x.x, (double)x.y);
    tw[k] = make_float2(w.x, -w.y);  // forward
  } else if (k == PRACH_NZC) {
    c[k] = make_double2(0.0, 0.0);
  }
  __syncthreads();
  if (k < PRACH_NZC) {
    const float2 y    = dft839(c, tw, k);
    const float  norm = (float)(1.0 / __builtin_sqrt(839.0));
    spec[(size_t)blockIdx.x * PRACH_NZC + k] = make_float2(y.x * norm, y.y * norm);
  }
}

__global__ __launch_bounds__(PRACH_THREADS) void prach_gen_kernel(PrachGenArgs g)
{
  __shared__ float2 buf[OFDM_MAX_N];
  const uint32_t    n1 = blockIdx.x, N = g.fft.N, M = PRACH_K * N, b0 = g.b0;
  // G[m] = sum over the bins b = m (mod N) of D_b exp(+2 pi i b n1 / 12N), conjugated: the inverse transform is
  // conj(FFT(conj(G))) as in the OFDM modulator
  for (uint32_t m = threadIdx.x; m < N; m += PRACH_THREADS) {
    float2 acc = make_float2(0.f, 0.f);
    for (uint32_t k = (m + N - b0 % N) % N; k < PRACH_NZC; k += N) {
      uint32_t b = b0 + k;
      if (b >= M) {
        b -= M;
      }
      const float2 D = g.spec[k], w = g.tw_m[(b * n1) % M];
      acc = cadd(acc, cmul(make_float2(D.x, -D.y), w));
    }
    buf[m] = acc;
  }
  __syncthreads();
  fft_ip(buf, g.fft);
  const uint32_t cp0 = M - g.n_cp;  // n_cp < 12 N for formats 0-3
  for (uint32_t n2 = threadIdx.x; n2 < N; n2 += PRACH_THREADS) {
    const uint32_t n = PRACH_K * n2 + n1;
    const float2   v = make_float2(buf[n2].x * g.scale, -(buf[n2].y * g.scale));
    for (uint32_t i = n; i < g.n_seq; i += M) {
      g.out[g.n_cp + i] = v;
    }
    if (n >= cp0) {
      g.out[n - cp0] = v;
    }
  }
}

hipError_t prach_bins_launch(const PrachOcc* d_occ, float2* part, uint32_t nocc, hipStream_t stream)
{
  if (nocc == 0) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(prach_bins_kernel, dim3(PRACH_K, nocc), dim3(PRACH_THREADS), 0, stream, d_occ, part);
  return hipGetLastError();
}

hipError_t prach_search_launch(const PrachOcc* d_occ, const float2* part, const float2* tw839, PrachOccOut* out,
                               uint32_t nocc, uint32_t max_roots, hipStream_t stream)
{
  if (nocc == 0 || max_roots == 0 || max_roots > PRACH_MAX_ROOTS) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(prach_search_kernel, dim3(max_roots, nocc), dim3(PRACH_DFT_THREADS), 0, stream, d_occ, part, tw839,
                     out);
  return hipGetLastError();
}

hipError_t prach_seq_dft_launch(const float2* seqs, const float2* tw839, float2* spec, uint32_t nseq,
                                hipStream_t stream)
{
  if (nseq == 0) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(prach_seq_dft_kernel, dim3(nseq), dim3(PRACH_DFT_THREADS), 0, stream, seqs, tw839, spec);
  return hipGetLastError();
}

hipError_t prach_gen_launch(const PrachGenArgs& a, hipStream_t stream)
{
  if (a.fft.N == 0 || a.fft.N > (uint32_t)OFDM_MAX_N || a.fft.nstages <= 0 || a.n_cp >= PRACH_K * a.fft.N ||
      (a.n_seq != PRACH_K * a.fft.N && a.n_seq != 2 * PRACH_K * a.fft.N)) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(prach_gen_kernel, dim3(PRACH_K), dim3(PRACH_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace srsran_amd
