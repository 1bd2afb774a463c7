// srsran_4g_amd/csrc/fft_stockham.h -- the workgroup-wide mixed-radix (8/4/3/2) Stockham FFT in one LDS buffer,
// moved verbatim out of ofdm_kernel.hip so that the PRACH kernels (prach_kernel.hip) run the same stages:
// complex helpers, the radix butterflies, one in-place stage (stage_ip) and the runtime plan (fft_ip) of an
// OfdmArgs (N, tw, nstages, radix, ns_magic as ofdm_plan gives them).  Device code only; include after
// ofdm_kernel.h, from a .hip file, inside no namespace.
#ifndef SRSRAN_AMD_FFT_STOCKHAM_H
#define SRSRAN_AMD_FFT_STOCKHAM_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ofdm_kernel.h"

namespace srsran_amd {

#ifndef OFDM_THREADS_CFG
#define OFDM_THREADS_CFG 256
#endif
static constexpr int OFDM_THREADS = OFDM_THREADS_CFG;  // a workgroup per symbol

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // * (-i)
// srsran_simd_cf_prod of the AVX2 + FMA build (simd.h:898-901) and gcc's contraction of the scalar
// complex products around it: re = fma(a.re, b.re, -(a.im b.im)), im = fma(a.re, b.im, a.im b.re), the inner
// products rounded on their own
__device__ __forceinline__ float2 ref_cprod(float2 a, float2 b)
{
  return make_float2(__fmaf_rn(a.x, b.x, -__fmul_rn(a.y, b.y)), __fmaf_rn(a.x, b.y, __fmul_rn(a.y, b.x)));
}

__device__ __forceinline__ void dft2(float2* v)
{
  const float2 a = v[0];
  v[0]           = cadd(a, v[1]);
  v[1]           = csub(a, v[1]);
}
__device__ __forceinline__ void dft4(float2* v)
{
  const float2 a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]);
  const float2 a2 = cadd(v[1], v[3]), a3 = mul_mi(csub(v[1], v[3]));
  v[0]            = cadd(a0, a2);
  v[2]            = csub(a0, a2);
  v[1]            = cadd(a1, a3);
  v[3]            = csub(a1, a3);
}
__device__ __forceinline__ void dft3(float2* v)
{
  const float  s   = 0.86602540378443864676f;  // sqrt(3)/2
  const float2 sum = cadd(v[1], v[2]);
  const float2 t1  = make_float2(v[0].x - 0.5f * sum.x, v[0].y - 0.5f * sum.y);
  const float2 d   = csub(v[1], v[2]);
  const float2 t2  = make_float2(d.y * s, -d.x * s);  // (x1 - x2) * (-i sqrt(3)/2)
  v[0]             = cadd(v[0], sum);
  v[1]             = cadd(t1, t2);
  v[2]             = csub(t1, t2);
}
__device__ __forceinline__ void dft8(float2* v)
{
  float2 e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
  dft4(e);
  dft4(o);
  const float r = 0.70710678118654752440f;
  o[1]          = make_float2((o[1].x + o[1].y) * r, (o[1].y - o[1].x) * r);    // * e^{-i pi/4}
  o[2]          = mul_mi(o[2]);                                                  // * e^{-i pi/2}
  o[3]          = make_float2((-o[3].x + o[3].y) * r, (-o[3].y - o[3].x) * r);  // * e^{-3i pi/4}
#pragma unroll
  for (int k = 0; k < 4; k++) {
    v[k]     = cadd(e[k], o[k]);
    v[k + 4] = csub(e[k], o[k]);
  }
}

// j / Ns for j < 2^16 and Ns <= 2^12 with m = ceil(2^32 / Ns) (exact in that range)
__device__ __forceinline__ uint32_t divm(uint32_t j, uint32_t m) { return __umulhi(j, m); }

// One Stockham stage of radix R (natural-order output), in place in one LDS buffer: every thread holds its butterflies' inputs in registers
// across a barrier (at most N / OFDM_THREADS values), so a symbol needs 16 KB of LDS
// instead of the 32 KB of a ping-pong pair -- 8 workgroups a CU instead of 5 (the launch is ~2200 symbols)
template <int R>
__device__ __forceinline__ void stage_ip(float2* buf, const float2* __restrict__ tw, uint32_t N, uint32_t Ns,
                                         uint32_t mNs)
{
  // butterflies per thread: N / R <= J * OFDM_THREADS (radix 3 only divides N = 3 * 2^k <= 1536)
  constexpr int  J  = ((R == 3 ? 1536 : OFDM_MAX_N) / R + OFDM_THREADS - 1) / OFDM_THREADS;
  const uint32_t nb = N / R, tstep = N / (Ns * R);
  float2 v[J][R], w[J][R];  // w: twiddles, loaded first (independent of the data) so their latency overlaps
#pragma unroll
  for (int jj = 0; jj < J; jj++) {
    const uint32_t j = threadIdx.x + jj * OFDM_THREADS;
    if (j < nb && Ns > 1) {
      const uint32_t k = j - divm(j, mNs) * Ns;
#pragma unroll
      for (int r = 1; r < R; r++) {
        w[jj][r] = tw[r * k * tstep];
      }
    }
  }
#pragma unroll
  for (int jj = 0; jj < J; jj++) {
    const uint32_t j = threadIdx.x + jj * OFDM_THREADS;
    if (j < nb) {
#pragma unroll
      for (int r = 0; r < R; r++) {
        v[jj][r] = buf[j + r * nb];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int jj = 0; jj < J; jj++) {
    const uint32_t j = threadIdx.x + jj * OFDM_THREADS;
    if (j < nb) {
      const uint32_t q = Ns > 1 ? divm(j, mNs) : j;
      const uint32_t k = j - q * Ns;
      if (Ns > 1) {
#pragma unroll
        for (int r = 1; r < R; r++) {
          v[jj][r] = cmul(v[jj][r], w[jj][r]);
        }
      }
      if constexpr (R == 8) {
        dft8(v[jj]);
      } else if constexpr (R == 4) {
        dft4(v[jj]);
      } else if constexpr (R == 3) {
        dft3(v[jj]);
      } else {
        dft2(v[jj]);
      }
      const uint32_t base = q * Ns * R + k;
#pragma unroll
      for (int r = 0; r < R; r++) {
        buf[base + r * Ns] = v[jj][r];
      }
    }
  }
  __syncthreads();
}

// the plan's stages in place on buf (barriers included)
__device__ __forceinline__ void fft_ip(float2* buf, const OfdmArgs& a)
{
  uint32_t Ns = 1;
  for (int st = 0; st < a.nstages; st++) {
    const int      R   = a.radix[st];
    const uint32_t mNs = a.ns_magic[st];
    if (R == 8) {
      stage_ip<8>(buf, a.tw, a.N, Ns, mNs);
    } else if (R == 4) {
      stage_ip<4>(buf, a.tw, a.N, Ns, mNs);
    } else if (R == 3) {
      stage_ip<3>(buf, a.tw, a.N, Ns, mNs);
    } else {
      stage_ip<2>(buf, a.tw, a.N, Ns, mNs);
    }
    Ns *= (uint32_t)R;
  }
}

}  // namespace srsran_amd
#endif
