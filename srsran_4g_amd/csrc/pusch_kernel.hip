// srsran_4g_amd/csrc/pusch_kernel.hip -- PUSCH receive kernels for CDNA4.
//
//   chest_ul_kernel      srsran_chest_ul_estimate_pusch (chest_ul.c:298-433): DMRS least squares
//                        (srsran_vec_prod_conj_ccc), 3-tap smoothing with the extrapolated edges of
//                        srsran_conv_same_cf (convolution.c:182-219), copy to every symbol of the slot
//                        (interpolate_pilots without DO_LINEAR_INTERPOLATION), noise from the
//                        smoothed-vs-raw difference (estimate_noise_pilots), CFO from the slot-to-slot
//                        correlation, TA from srsran_vec_estimate_frequency, RSRP / EPRE.
//   pusch_eq_idft_kernel pusch_get + srsran_predecoding_single (precoding.c:182-305, ZF / MMSE with
//                        the chest noise) + srsran_dft_precoding (dft_precoding.c:114-126): the
//                        M-point backward DFT normalised by 1 / sqrt(M) of every data symbol.
//
// Layout: one workgroup per UE for the estimator (2M <= 2400 pilots, all reductions in one pass),
// one workgroup per (data symbol, UE) for the de-precoder.  The DFT is a mixed-radix Stockham
// autosort transform in LDS (radices 4, 2, 3, 5; M = 12 L with L = 2^a 3^b 5^c <= 100): every
// stage reads and writes LDS once, 256 threads cover the <= 600 butterflies of a stage, twiddles
// come from sincospif (no table traffic).  Both kernels are HBM-bound elementwise work (the grid
// and the estimate are read once per data RE); floating point, compared with the oracle within a
// tolerance (the reference's DFT is FFTW, absent here).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chest_ul_dev.h"
#include "dft_mixed_dev.h"
#include "pusch_kernel.h"
#include "stage_timing.h"

namespace srsran_amd {

// ---------------------------------------------------------------- channel estimation
// 16 waves a UE: 78 UEs are 78 workgroups, so each one's 2 M pilots and 14 M estimate stores spread over more
// threads (the estimate copy to every symbol of the slot is most of the kernel's bytes)
static constexpr int CHUL_THREADS = 1024;

__global__ __launch_bounds__(CHUL_THREADS) void chest_ul_kernel(const PuschUe* __restrict__ ues)
{
  const PuschUe& u = ues[blockIdx.x];
  __shared__ float2 pe[2 * PUSCH_MAX_M];
  __shared__ float  red[(CHUL_THREADS / 64) * 11];
  const uint32_t    M = u.M;

  // LS estimates; received pilot sum and power
  float acc[11] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (uint32_t k = threadIdx.x; k < 2 * M; k += CHUL_THREADS) {
    const uint32_t s = k >= M ? 1u : 0u, j = k - s * M;
    const uint32_t L = (s + 1) * u.nsym_slot - 4;
    const c2       rx = mk(u.grid[(size_t)L * u.ncell_re + u.n_tilde[s] * 12 + j]);
    const c2       e  = mulconj(rx, mk(u.dmrs[k]));
    pe[k]             = make_float2(e.r, e.i);
    acc[0] += rx.r, acc[1] += rx.i, acc[2] += rx.r * rx.r + rx.i * rx.i;
  }
  __syncthreads();

  // smoothing, estimate grid, noise, CFO and TA correlations
  const float f0 = u.filt[0], f1 = u.filt[1], f2 = u.filt[2];
  for (uint32_t k = threadIdx.x; k < 2 * M; k += CHUL_THREADS) {
    const uint32_t s = k >= M ? 1u : 0u, j = k - s * M;
    const float2*  p = pe + s * M;
    const c2       x = mk(p[j]);
    c2             a = x;
    if (u.smooth) {
      a = smooth3(p, j, M, f0, f1, f2);
      const c2 d = sub(a, x);
      acc[3 + s] += d.r * d.r + d.i * d.i;
    }
    const float2 av = make_float2(a.r, a.i);
    for (uint32_t i = 0; i < u.nsym_slot; i++) {
      u.ce[(size_t)(s * u.nsym_slot + i) * u.ncell_re + u.n_prb[s] * 12 + j] = av;
    }
    if (s == 0) {
      const c2 c = mulconj(x, mk(pe[M + j]));
      acc[5] += c.r, acc[6] += c.i;
    }
    if (u.meas_ta && j > 0) {
      const c2 c = mulconj(x, mk(p[j - 1]));
      acc[7 + 2 * s] += c.r, acc[8 + 2 * s] += c.i;
    }
  }
  block_sum<11>(acc, red);
  if (threadIdx.x == 0) {
    ChestUlOut o;
    o.cfo_hz = atan2f(acc[6], acc[5]) / (2.0f * 3.14159265358979323846f * 0.0005f);
    float ta = 0.0f;
    if (u.meas_ta) {
      for (int s = 0; s < 2; s++) {
        ta += freq_from_corr(acc[7 + 2 * s], acc[8 + 2 * s]) / 2.0f;
      }
    }
    o.ta_us = ta_us_from_freq(ta);
    if (u.smooth) {
      float power = acc[3] / (float)M;
      power += acc[4] / (float)M;
      power /= 2.0f;
      o.noise = (float)((double)power / u.noise_div);
    } else {
      o.noise = 0.0f;
    }
    const float n2   = (float)(2 * M);
    const float cr   = acc[0] / n2, ci = acc[1] / n2;
    const float epre = acc[2] / n2;
    o.rsrp           = fminf(cr * cr + ci * ci, epre);
    o.epre           = epre;
    o.data_pow       = 0.0f;
    *u.out           = o;
  }
}

hipError_t chest_ul_launch(const PuschUe* d_ues, uint32_t nue, hipStream_t stream)
{
  if (nue == 0) {
    return hipSuccess;
  }
  StageScope timing_scope(ST_CHEST_UL, stream);
  hipLaunchKernelGGL(chest_ul_kernel, dim3(nue), dim3(CHUL_THREADS), 0, stream, d_ues);
  return hipGetLastError();
}

// ---------------------------------------------------------------- equaliser + inverse DFT
// (the radix-R Stockham stages: dft_mixed_dev.h)
__global__ __launch_bounds__(PU_THREADS) void pusch_eq_idft_kernel(const PuschUe* __restrict__ ues)
{
  const PuschUe& u = ues[blockIdx.y];
  const uint32_t l = blockIdx.x;
  if (l >= u.nof_symb) {
    return;
  }
  __shared__ float2 buf[2][PUSCH_MAX_M];
  __shared__ float  red[PU_THREADS / 64];
  const uint32_t    M     = u.M;
  const uint32_t    g     = u.data_sym[l];
  const uint32_t    slot  = g >= u.nsym_slot ? 1u : 0u;
  const size_t      base  = (size_t)g * u.ncell_re + u.n_tilde[slot] * 12;
  const float       noise = u.noise_dev && u.out ? u.out->noise : u.noise;
  const uint32_t    nre   = M * u.nof_symb, nvec = 8 * (nre / 8);

  // srsran_predecoding_single: x = y conj(h) / (|h|^2 + n0); the 8-wide AVX body adds n0 only
  // when it is positive, the scalar tail always
  float pw[1] = {0.f};
  for (uint32_t j = threadIdx.x; j < M; j += PU_THREADS) {
    const c2 y = mk(u.grid[base + j]);
    if (u.ce) {
      const c2    h  = mk(u.ce[base + j]);
      const float hh = h.r * h.r + h.i * h.i;
      const float dn = (l * M + j < nvec) ? (noise > 0.0f ? hh + noise : hh) : hh + noise;
      const c2    z  = mulconj(y, h);
      buf[0][j]      = make_float2(z.r / dn, z.i / dn);
    } else {  // plain transform de-precoding (srsran_dft_precoding)
      buf[0][j] = make_float2(y.r, y.i);
    }
    pw[0] += y.r * y.r + y.i * y.i;
  }
  block_sum<1>(pw, red);
  if (threadIdx.x == 0 && u.out) {
    atomicAdd(&u.out->data_pow, pw[0]);
  }
  __syncthreads();

  uint32_t Ns = 1, cur = 0;
  for (uint32_t st = 0; st < u.nstages; st++) {
    const uint32_t R = u.radix[st];
    if (R == 4) {
      stage<4>(buf[cur], buf[cur ^ 1], M, Ns);
    } else if (R == 2) {
      stage<2>(buf[cur], buf[cur ^ 1], M, Ns);
    } else if (R == 3) {
      stage<3>(buf[cur], buf[cur ^ 1], M, Ns);
    } else {
      stage<5>(buf[cur], buf[cur ^ 1], M, Ns);
    }
    Ns *= R;
    cur ^= 1;
    __syncthreads();
  }
  float2* o = u.sym + (size_t)l * M;
  for (uint32_t j = threadIdx.x; j < M; j += PU_THREADS) {
    const float2 v = buf[cur][j];
    o[j]           = make_float2(v.x * u.dft_norm, v.y * u.dft_norm);
  }
}

hipError_t pusch_eq_idft_launch(const PuschUe* d_ues, uint32_t nue, hipStream_t stream)
{
  if (nue == 0) {
    return hipSuccess;
  }
  StageScope timing_scope(ST_PUSCH_EQ, stream);
  hipLaunchKernelGGL(pusch_eq_idft_kernel, dim3(14, nue), dim3(PU_THREADS), 0, stream, d_ues);
  return hipGetLastError();
}

}  // namespace srsran_amd
