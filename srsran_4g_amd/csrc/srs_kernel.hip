// srsran_4g_amd/csrc/srs_kernel.hip -- sounding reference signal for the UE (36.211 5.5.3.1 / 5.5.3.2;
// refsignal_ul.c:870-906 over zc_sequence.c:214-241, 282).
//
// One workgroup per transmission, all SRS-carrying transmissions of all cells in one launch.  A workgroup of an
// SRS-only subframe first zeroes every RE of its grid that is not on its comb (16-byte stores over the rows
// above the last symbol, 8-byte stores in the last one), then its threads stride over i < M_sc (M_sc reaches 576)
// and each forms r_srs(i) and stores it to the comb of the last symbol.  No LDS, no inter-lane traffic.
//
// The reference's single-precision arguments are the contract (its estimator sees them): the Zadoff-Chu argument
// -pi q m (m + 1) / N_zc is evaluated in double from single-precision q, m, N_zc and rounded to float, and
// cexpf takes fl(arg + alpha i) with one rounding of the sum: the reference as the oracle builds it (-Ofast -mfma)
// fuses the product into the sum, and that build is what the fixtures record (a build without fma rounds alpha i
// first and lies up to 2e-3 away at M_sc = 576).  The arguments reach 1e6 rad there, where one ulp is 0.0625 rad,
// so the roundings are the signal: fmaf is explicit, and sincosf is the accurate one with the full range reduction.
#include "chest_ul_dev.h"
#include "srs_kernel.h"

namespace srsran_amd {

namespace {

constexpr uint32_t SRS_THREADS = 256;
constexpr double   kPi         = 3.14159265358979323846;

// r_srs(i) = exp(j fl(fl(arg(i)) + alpha i)): one rounding of the sum
__device__ inline float2 srs_r(const SrsSeq& s, uint32_t i)
{
  float arg;
  if (s.n_zc == 0) {  // zc_sequence.c:211: phi(i) times M_PI_4 as a float
    arg = (float)s.phi[i < 24u ? i : 0u] * 0.78539816339744830962f;
  } else {  // zc_sequence.c:235-238: float m and m + 1, the product and the quotient in double, left to right
    const float m = (float)(i % s.n_zc);
    double      a = -kPi * (double)s.q;
    a             = a * (double)m;
    a             = a * (double)(m + 1.0f);
    arg           = (float)(a / (double)(float)s.n_zc);
  }
  const float x = fmaf(s.alpha, (float)i, arg);
  float       sn, cs;
  sincosf(x, &sn, &cs);
  return make_float2(cs, sn);
}

}  // namespace

__global__ __launch_bounds__(SRS_THREADS) void srs_tx_kernel(const SrsTxUe* __restrict__ ues)
{
  const SrsTxUe& u = ues[blockIdx.x];
  if (!u.grid || u.nsym == 0) {
    return;
  }
  float2*        last = u.grid + (size_t)(u.nsym - 1) * u.ncell_re;
  const uint32_t kend = u.k0 + 2 * u.m_sc;  // one past the comb's span (the RE kend - 1 is off the comb)
  if (u.zero_rest) {
    const size_t above = (size_t)(u.nsym - 1) * u.ncell_re;  // the REs of the rows above the last symbol
    if ((((uintptr_t)u.grid) & 15u) == 0 && (above & 1u) == 0) {
      float4* g4 = (float4*)u.grid;
      for (size_t j = threadIdx.x; j < above / 2; j += SRS_THREADS) {
        g4[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {
      for (size_t j = threadIdx.x; j < above; j += SRS_THREADS) {
        u.grid[j] = make_float2(0.f, 0.f);
      }
    }
    for (uint32_t k = threadIdx.x; k < u.ncell_re; k += SRS_THREADS) {
      if (k < u.k0 || k >= kend || ((k - u.k0) & 1u)) {
        last[k] = make_float2(0.f, 0.f);
      }
    }
  }
  for (uint32_t i = threadIdx.x; i < u.m_sc; i += SRS_THREADS) {
    const uint32_t k = u.k0 + 2 * i;
    if (k < u.ncell_re) {
      last[k] = srs_r(u.seq, i);
    }
  }
}

hipError_t srs_tx_launch(const SrsTxUe* d_ues, uint32_t nue, hipStream_t stream)
{
  if (nue == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(srs_tx_kernel, dim3(nue), dim3(SRS_THREADS), 0, stream, d_ues);
  return hipGetLastError();
}

// ---------------------------------------------------------------- eNB: srsran_chest_ul_estimate_srs
// One workgroup per UE: the comb REs of the last symbol (srsran_refsignal_srs_get), the known sequence from the
// transmitter's function, the least-squares product (srsran_vec_prod_conj_ccc) into LDS, then chest_ul_estimate with
// one slot: the 3-tap smoothing or the copy into the estimate row, the noise from smoothed against raw, the time
// alignment from the neighbour correlation, EPRE and RSRP.  chest_ul.c:644 hands chest_ul_estimate a pilot spacing of
// 1 although the comb has a pilot every second subcarrier: ta_us is twice the delay behind the ramp.  Kept.
__global__ __launch_bounds__(SRS_THREADS) void srs_chest_kernel(const SrsRxUe* __restrict__ ues)
{
  const SrsRxUe& u = ues[blockIdx.x];
  __shared__ float2 pe[SRS_MAX_M_SC];
  __shared__ float  red[(SRS_THREADS / 64) * 6];
  const uint32_t    M = u.m_sc <= SRS_MAX_M_SC ? u.m_sc : 0u;
  const float2*     last = u.grid + (size_t)(u.nsym - 1) * u.ncell_re;

  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // sum rx (2), sum |rx|^2, sum |avg - raw|^2, neighbour correlation (2)
  for (uint32_t i = threadIdx.x; i < M; i += SRS_THREADS) {
    const uint32_t k  = u.k0 + 2 * i;
    const c2       rx = k < u.ncell_re ? mk(last[k]) : c2{0.f, 0.f};
    const c2       e  = mulconj(rx, mk(srs_r(u.seq, i)));
    pe[i]             = make_float2(e.r, e.i);
    acc[0] += rx.r, acc[1] += rx.i, acc[2] += rx.r * rx.r + rx.i * rx.i;
  }
  __syncthreads();
  const float f0 = u.filt[0], f1 = u.filt[1], f2 = u.filt[2];
  for (uint32_t j = threadIdx.x; j < M; j += SRS_THREADS) {
    const c2 x = mk(pe[j]);
    c2       a = x;
    if (u.smooth && M >= 2) {
      a = smooth3(pe, j, M, f0, f1, f2);
      const c2 d = sub(a, x);
      acc[3] += d.r * d.r + d.i * d.i;
    }
    if (u.ce) {
      u.ce[j] = make_float2(a.r, a.i);
    }
    if (j > 0) {
      const c2 c = mulconj(x, mk(pe[j - 1]));
      acc[4] += c.r, acc[5] += c.i;
    }
  }
  block_sum<6>(acc, red);
  if (threadIdx.x == 0 && u.out) {
    ChestUlOut o;
    o.cfo_hz = __builtin_nanf("");  // one slot: no CFO (chest_ul.c:313-315)
    o.ta_us  = ta_us_from_freq(freq_from_corr(acc[4], acc[5]));  // nslots = 1, stride = 1
    o.noise  = u.smooth ? (float)((double)(acc[3] / (float)M) / u.noise_div) : 0.0f;
    const float n  = (float)M;
    const float cr = acc[0] / n, ci = acc[1] / n, epre = acc[2] / n;
    o.rsrp     = fminf(cr * cr + ci * ci, epre);
    o.epre     = epre;
    o.data_pow = 0.0f;
    *u.out     = o;
  }
}

hipError_t srs_chest_launch(const SrsRxUe* d_ues, uint32_t nue, hipStream_t stream)
{
  if (nue == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(srs_chest_kernel, dim3(nue), dim3(SRS_THREADS), 0, stream, d_ues);
  return hipGetLastError();
}

}  // namespace srsran_amd
