// srsran_4g_amd/csrc/chest_ul_dev.h -- device pieces the uplink estimators share (chest_ul_kernel of
// pusch_kernel.hip for the PUSCH DMRS, srs_chest_kernel of srs_kernel.hip for the SRS): the block reduction, the
// 3-tap smoothing with the extrapolated edges of srsran_conv_same_cf (convolution.c:182-219), and the time alignment
// of srsran_vec_estimate_frequency from the neighbour correlation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dft_mixed_dev.h"

namespace srsran_amd {

// sum over the block of NV floats per thread; every thread gets the totals
template <int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* red)
{
#pragma unroll
  for (int k = 0; k < NV; k++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      v[k] += __shfl_xor(v[k], off, 64);
    }
  }
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NV; k++) {
      red[w * NV + k] = v[k];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; k++) {
    float s = 0.f;
    for (int i = 0; i < nw; i++) {
      s += red[i * NV + k];
    }
    v[k] = s;
  }
}

// pilot j of the M least-squares estimates p through the 3-tap filter (f0, f1, f2); the neighbours beyond the edges
// are the linear extrapolations 3 p[0] - 2 p[1] ... as srsran_conv_same_cf's caller pads them
__device__ __forceinline__ c2 smooth3(const float2* p, uint32_t j, uint32_t M, float f0, float f1, float f2)
{
  const c2 x = mk(p[j]);
  c2       l, r;
  if (j == 0) {
    l = sub(scl(mk(p[1]), 3.0f), scl(mk(p[0]), 2.0f));
  } else {
    l = mk(p[j - 1]);
  }
  if (j == M - 1) {
    r = sub(scl(mk(p[M - 1]), 3.0f), scl(mk(p[M - 2]), 2.0f));
  } else {
    r = mk(p[j + 1]);
  }
  return add(add(scl(l, f0), scl(x, f1)), scl(r, f2));
}

// srsran_vec_estimate_frequency from the sum of x[j] conj(x[j - 1]): normalised frequency, -arg / (2 pi)
__device__ __forceinline__ float freq_from_corr(float re, float im)
{
  return (float)((double)-atan2f(im, re) * 0.31830988618379067154 * 0.5);
}

// chest_ul.c:332-340: normalised frequency to microseconds on the 0.1 us grid (0 for a value that is not normal)
__device__ __forceinline__ float ta_us_from_freq(float ta)
{
  if (!isnormal(ta)) {
    return 0.0f;
  }
  ta /= 15e3f;
  ta *= 1e6f;
  return roundf(ta * 10.0f) / 10.0f;
}

}  // namespace srsran_amd
