// srsran_4g_amd/csrc/csi_kernel.hip -- RI / PMI / SINR selection of a 2-port x 2-rx cell as one reduction over the
// device-resident channel estimate (csi_kernel.h), one workgroup a subframe.
//
// What is computed (mimo/precoding.c of the reference, its AVX2 release build):
//  * sinr_1l[4]: srsran_precoding_pmi_select_1l_simd (precoding.c:2350-2465), sinr_2l[2]: ..._2l_simd (:2595-2745)
//    with its 1e-10 determinant floor and 1e-9 gamma floor, on the SIMD sample set: indices 192 b + 24 k, k < 8, of
//    every whole block b of 192 -- that is 24 s for s < 8 floor(nof_symbols / 192); the tail is dropped.  The
//    reference averages the 8 samples of a block (/ 8) before it accumulates; the scaling by 1/8 is exact in
//    float, so it is applied to the sum.  Plain float division where the SIMD code uses rcp, as the equaliser
//    (eq_dev.h) does.
//  * cn: srsran_precoding_2x2_cn_gen + srsran_mat_2x2_cn (precoding.c:2798-2822, mat.c:128-160) on every 24th index
//    of all nof_symbols: 24 s for s < ceil(nof_symbols / 24); a sample whose eigenvalues are NaN / Inf is skipped
//    and not counted.  The SINR set is a prefix of this one, not the same set (696 and 700 points at 100 PRB).
//  * the decisions: first strict maximum from 0 (pmi_1l, pmi_2l), cn < 17 (ue_dl.c:838), select_ri_pmi's rule
//    (ue_dl.c:778-822).
// Sums: every thread adds its samples (s = tid, tid + 1024, ...: one a thread up to 110 PRB, so the workgroup's 16
// waves work side by side rather than one sample after another), then a fixed tree: xor shuffles over the 64 lanes,
// then the 16 waves' values through LDS, pairwise ((w0 + w1) + (w2 + w3)) + ...  The block size is a constant of
// the kernel, so a result does not depend on how it is launched; no float atomics.
#include <float.h>
#include <math.h>

#include "csi_kernel.h"

namespace srsran_amd {
namespace {

constexpr int      CSI_THREADS = 1024; // 16 waves: the tree's shape
constexpr int      CSI_WAVES   = CSI_THREADS / 64;
constexpr int      CSI_NV      = 8;    // sums: sinr_1l[4], sinr_2l[2], condition number, its sample count
constexpr uint32_t CSI_STEP    = 24;   // PMI_SEL_PRECISION
constexpr uint32_t CSI_SIMD    = 8;    // SRSRAN_SIMD_CF_SIZE of the AVX2 build

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 cmulj(float2 a) { return make_float2(-a.y, a.x); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cscale(float2 a, float s) { return make_float2(a.x * s, a.y * s); }

// 2 (gamma0 + gamma1) terms of one two-layer codebook: C = 0.25 [c00 c01; c10 c11] + noise I (precoding.c:2678-2704)
__device__ __forceinline__ float gamma_2l(float2 c00, float2 c01, float2 c10, float2 c11, float noise)
{
  c00 = cscale(c00, 0.25f);
  c01 = cscale(c01, 0.25f);
  c10 = cscale(c10, 0.25f);
  c11 = cscale(c11, 0.25f);
  c00.x += noise;
  c11.x += noise;
  float det = cmul(c00, c11).x - cmul(c01, c10).x;
  det       = det < 1e-10f ? 1e-10f : det;
  const float inv = noise * (1.0f / det);
  float       g0  = 1.0f / (c00.x * inv) - 1.0f;
  float       g1  = 1.0f / (c11.x * inv) - 1.0f;
  g0              = g0 < 1e-9f ? 1e-9f : g0;
  g1              = g1 < 1e-9f ? 1e-9f : g1;
  return g0 + g1;
}

// srsran_mat_2x2_cn: false where the reference returns SRSRAN_ERROR (mat.c:146-149)
__device__ __forceinline__ bool cn_2x2(float2 h00, float2 h01, float2 h10, float2 h11, float& cn)
{
  const float  a00 = h00.x * h00.x + h01.x * h01.x + h00.y * h00.y + h01.y * h01.y;
  const float2 a01 = cadd(cmul(h00, cconj(h10)), cmul(h01, cconj(h11)));
  const float  a11 = h10.x * h10.x + h11.x * h11.x + h10.y * h10.y + h11.y * h11.y;
  const float  b   = a00 + a11;
  const float  c   = a00 * a11 - (a01.x * a01.x + a01.y * a01.y);
  const float  sqr = sqrtf(b * b - 4.0f * c);
  float        xmax = b + sqr, xmin = b - sqr;
  if (!isfinite(xmin) || !isfinite(xmax)) {
    return false;
  }
  xmin = fmaxf(xmin, 1e-9f);
  xmax = fminf(xmax, 1e+9f);
  cn   = 10.0f * log10f(xmax / xmin);
  return true;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    v += __shfl_xor(v, o, 64);
  }
  return v;
}

__global__ __launch_bounds__(CSI_THREADS) void csi_kernel(CsiArgs a)
{
  const uint32_t sf = blockIdx.x, tid = threadIdx.x;
  // h[port][rx] rows; the reference's names: h00 = h[0][0], h01 = h[1][0], h10 = h[0][1], h11 = h[1][1]
  const float2* r00 = a.ce + (size_t)sf * a.sf_stride;
  const float2* r10 = r00 + a.row_stride;
  const float2* r01 = r00 + 2 * a.row_stride;
  const float2* r11 = r00 + 3 * a.row_stride;
  float         noise = a.noise ? a.noise[(size_t)sf * a.noise_stride] : a.noise_val;
  if (!(noise >= 1e-9f && noise <= FLT_MAX)) {  // !isnormal(noise) || noise < 1e-9 (precoding.c:2781-2783)
    noise = 1e-9f;
  }
  const uint32_t nblk = a.nof_symbols / (CSI_STEP * CSI_SIMD);
  const uint32_t npmi = nblk * CSI_SIMD, ncn = (a.nof_symbols + CSI_STEP - 1) / CSI_STEP;
  float          v[CSI_NV] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (uint32_t s = tid; s < ncn; s += CSI_THREADS) {
    const uint32_t j   = (CSI_STEP * s) % a.row_len;  // CSI_STEP * s < nof_symbols
    const float2   h00 = r00[j], h01 = r01[j], h10 = r10[j], h11 = r11[j];
    float          cn;
    if (cn_2x2(h00, h01, h10, h11, cn)) {
      v[6] += cn;
      v[7] += 1.0f;
    }
    if (s >= npmi) {
      continue;
    }
    // B = W' H' H of the four one-layer precoders w = [1, q] / sqrt 2, q = +1, -1, +j, -j (precoding.c:2383-2406)
    float2 b0[4], b1[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const float2 t0 = i < 2 ? cconj(h01) : cmulj(cconj(h01)), t1 = i < 2 ? cconj(h11) : cmulj(cconj(h11));
      const bool   add = i == 0 || i == 3;
      const float2 a0 = add ? cadd(cconj(h00), t0) : csub(cconj(h00), t0);
      const float2 a1 = add ? cadd(cconj(h10), t1) : csub(cconj(h10), t1);
      b0[i]           = cadd(cmul(a0, h00), cmul(a1, h10));
      b1[i]           = cadd(cmul(a0, h01), cmul(a1, h11));
    }
    // one layer: gamma = Re(B w) / 2 (precoding.c:2408-2427)
    v[0] += (b0[0].x + b1[0].x) * 0.5f;
    v[1] += (b0[1].x - b1[1].x) * 0.5f;
    v[2] += (b0[2].x - b1[2].y) * 0.5f;
    v[3] += (b0[3].x + b1[3].y) * 0.5f;
    // two layers: codebook 0 has the rows of precoders 0 and 1, codebook 1 those of 2 and 3 (precoding.c:2635-2677)
    v[4] += gamma_2l(cadd(b0[0], b1[0]), csub(b0[0], b1[0]), cadd(b0[1], b1[1]), csub(b0[1], b1[1]), noise);
    v[5] += gamma_2l(cadd(b0[2], cmulj(b1[2])), csub(b0[2], cmulj(b1[2])), cadd(b0[3], cmulj(b1[3])),
                     csub(b0[3], cmulj(b1[3])), noise);
  }
  __shared__ float red[CSI_WAVES][CSI_NV];
  __shared__ float tot[CSI_NV];
#pragma unroll
  for (int k = 0; k < CSI_NV; k++) {
    v[k] = wave_sum(v[k]);
  }
  if ((tid & 63u) == 0) {
#pragma unroll
    for (int k = 0; k < CSI_NV; k++) {
      red[tid >> 6][k] = v[k];
    }
  }
  __syncthreads();
  if (tid < CSI_NV) {  // thread k: the pairwise tree over the waves' sums of value k
    float w[CSI_WAVES];
#pragma unroll
    for (int i = 0; i < CSI_WAVES; i++) {
      w[i] = red[i][tid];
    }
#pragma unroll
    for (int stride = 1; stride < CSI_WAVES; stride *= 2) {
#pragma unroll
      for (int i = 0; i < CSI_WAVES; i += 2 * stride) {
        w[i] += w[i + stride];
      }
    }
    tot[tid] = w[0];
  }
  __syncthreads();
  if (tid != 0) {
    return;
  }
  float t[CSI_NV];
#pragma unroll
  for (int k = 0; k < CSI_NV; k++) {
    t[k] = tot[k];
  }
  srsran_csi_gpu_t o;
  const float      count = (float)nblk;
#pragma unroll
  for (int i = 0; i < 4; i++) {  // sinr_acc /= noise_estimate * count; 1e9 without a whole block (:2446-2450)
    o.sinr_1l[i] = nblk ? (t[i] * 0.125f) / (noise * count) : 1e+9f;
  }
#pragma unroll
  for (int i = 0; i < 2; i++) {
    o.sinr_2l[i] = nblk ? (t[4 + i] * 0.125f) / count : 1e+9f;
  }
  o.cn       = t[7] > 0.0f ? t[6] / t[7] : 0.0f;
  o.cn_count = (uint32_t)t[7];
  // first strict maximum from 0; at1 / at2: the SINR at the chosen entry (entry 0 where none is above 0).  Unrolled
  // with the values in registers: an index computed at run time would move the record into scratch or LDS
  float best = 0.0f, at1 = o.sinr_1l[0], at2 = o.sinr_2l[0];
  o.pmi_1l   = 0;
#pragma unroll
  for (uint32_t i = 0; i < 4; i++) {
    if (o.sinr_1l[i] > best) {
      best     = o.sinr_1l[i];
      at1      = o.sinr_1l[i];
      o.pmi_1l = i;
    }
  }
  best     = 0.0f;
  o.pmi_2l = 0;
#pragma unroll
  for (uint32_t i = 0; i < 2; i++) {
    if (o.sinr_2l[i] > best) {
      best     = o.sinr_2l[i];
      at2      = o.sinr_2l[i];
      o.pmi_2l = i;
    }
  }
  o.ri_cn = o.cn < 17.0f ? 1u : 0u;
  // select_ri_pmi (ue_dl.c:778-822): the larger rank if its SINR in dB exceeds the best by 0.1 (a double sum
  // there) or is above 20
  const float db1 = 10.0f * log10f(at1), db2 = 10.0f * log10f(at2);
  float       best_db = -INFINITY;
  o.ri  = 0;
  o.pmi = 0;
  if ((double)db1 > (double)best_db + 0.1 || db1 > 20.0f) {
    best_db = db1;
    o.pmi   = o.pmi_1l;
  }
  if ((double)db2 > (double)best_db + 0.1 || db2 > 20.0f) {
    best_db = db2;
    o.pmi   = o.pmi_2l;
    o.ri    = 1;
  }
  o.sinr_db     = best_db;
  o.reserved[0] = o.reserved[1] = 0;
  a.out[sf]                     = o;
}

}  // namespace

hipError_t csi_launch(const CsiArgs& a, uint32_t nsf, hipStream_t stream)
{
  if (nsf == 0) {
    return hipSuccess;
  }
  if (!a.ce || !a.out || a.row_len == 0 || a.nof_symbols == 0) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(csi_kernel, dim3(nsf), dim3(CSI_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace srsran_amd
