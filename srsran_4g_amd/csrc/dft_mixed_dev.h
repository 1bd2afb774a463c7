// srsran_4g_amd/csrc/dft_mixed_dev.h -- the mixed-radix Stockham stages of the SC-FDMA transform (de-)precoder
// (dft_precoding.c:114-126), shared by the receive kernels (pusch_kernel.hip, backward transform) and the transmit
// kernels (pusch_tx_kernel.hip, which runs the forward transform as the conjugate of the backward one of the
// conjugate).  M = 12 L with L = 2^a 3^b 5^c <= 100: radices 4, 2, 3, 5; every stage reads and writes LDS once,
// PU_THREADS threads cover the <= 600 butterflies of a stage, twiddles come from sincospif.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace srsran_amd {

static constexpr int PU_THREADS = 256;

struct c2 {
  float r, i;
};
__device__ __forceinline__ c2 mk(float2 v) { return {v.x, v.y}; }
__device__ __forceinline__ c2 add(c2 a, c2 b) { return {a.r + b.r, a.i + b.i}; }
__device__ __forceinline__ c2 sub(c2 a, c2 b) { return {a.r - b.r, a.i - b.i}; }
__device__ __forceinline__ c2 mul(c2 a, c2 b) { return {a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
__device__ __forceinline__ c2 mulconj(c2 a, c2 b) { return {a.r * b.r + a.i * b.i, a.i * b.r - a.r * b.i}; }  // a conj(b)
__device__ __forceinline__ c2 scl(c2 a, float s) { return {a.r * s, a.i * s}; }
__device__ __forceinline__ c2 mulj(c2 a) { return {-a.i, a.r}; }

// one radix-R Stockham stage (backward transform: twiddles and butterflies e^{+j...})
template <int R>
__device__ __forceinline__ void stage(const float2* __restrict__ in, float2* __restrict__ out, uint32_t N, uint32_t Ns)
{
  const uint32_t nb = N / R;
  for (uint32_t j = threadIdx.x; j < nb; j += PU_THREADS) {
    const uint32_t k = j % Ns;
    c2             v[R];
    v[0] = mk(in[j]);
#pragma unroll
    for (int r = 1; r < R; r++) {
      float sn, cs;
      sincospif(2.0f * (float)(r * k) / (float)(Ns * R), &sn, &cs);
      v[r] = mul(mk(in[j + r * nb]), c2{cs, sn});
    }
    c2 y[R];
    if (R == 2) {
      y[0] = add(v[0], v[1]);
      y[1] = sub(v[0], v[1]);
    } else if (R == 4) {
      const c2 s02 = add(v[0], v[2]), d02 = sub(v[0], v[2]);
      const c2 s13 = add(v[1], v[3]), d13 = mulj(sub(v[1], v[3]));
      y[0] = add(s02, s13);
      y[1] = add(d02, d13);
      y[2] = sub(s02, s13);
      y[3] = sub(d02, d13);
    } else if (R == 3) {
      const float h = 0.86602540378443864676f;  // sin(2 pi / 3)
      const c2    t = add(v[1], v[2]);
      const c2    m = sub(v[0], scl(t, 0.5f));
      const c2    d = mulj(scl(sub(v[1], v[2]), h));
      y[0]          = add(v[0], t);
      y[1]          = add(m, d);
      y[2]          = sub(m, d);
    } else {  // R == 5
      const float c1 = 0.30901699437494742410f, c2c = -0.80901699437494742410f;
      const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
      const c2    t1 = add(v[1], v[4]), t2 = add(v[2], v[3]);
      const c2    d1 = sub(v[1], v[4]), d2 = sub(v[2], v[3]);
      const c2    a1 = add(v[0], add(scl(t1, c1), scl(t2, c2c)));
      const c2    a2 = add(v[0], add(scl(t1, c2c), scl(t2, c1)));
      const c2    b1 = mulj(add(scl(d1, s1), scl(d2, s2)));
      const c2    b2 = mulj(sub(scl(d1, s2), scl(d2, s1)));
      y[0]           = add(v[0], add(t1, t2));
      y[1]           = add(a1, b1);
      y[4]           = sub(a1, b1);
      y[2]           = add(a2, b2);
      y[3]           = sub(a2, b2);
    }
    const uint32_t o = (j / Ns) * Ns * R + k;
#pragma unroll
    for (int r = 0; r < R; r++) {
      out[o + r * Ns] = make_float2(y[r].r, y[r].i);
    }
  }
}

}  // namespace srsran_amd
