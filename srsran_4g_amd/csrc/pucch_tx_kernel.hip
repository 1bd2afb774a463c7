// srsran_4g_amd/csrc/pucch_tx_kernel.hip -- PUCCH transmit for the UE, formats 1/1a/1b/2/2a/2b/3 with DMRS
// (36.211 5.4, 5.5.2.2; pucch.c:136-203, 321-504, refsignal_ul.c:432-552).
//
// One workgroup per (grid symbol, transmission), all transmissions of all cells in one launch.  A workgroup
// zeroes its row of the grid outside the PUCCH PRB with 16-byte stores (UE path), then the 12 lanes of the PRB
// each form one RE from the descriptor: the modulation symbol from the coded and scrambling bits, the base
// sequence, the cover, and for format 3 the spread, shifted block through a 12-point DFT.  No LDS, no
// inter-lane traffic: what the lanes share (d, the cover, h) is a handful of operations recomputed per lane.
//
// The reference's single-precision arguments are the contract (its receiver sees them): a sequence value is
// exp(j fl(fl(phi(n) pi / 4) + alpha n)) with one rounding of the sum, a format 3 twiddle exp(-j fl(2 pi i k /
// 12)) with the unreduced argument.  sinf / cosf are the accurate ones: the arguments reach 63 rad.
#include "pucch_tx_kernel.h"

namespace srsran_amd {

namespace {

constexpr uint32_t PTX_THREADS = 256;
constexpr double   kPi         = 3.14159265358979323846;

// The reference's single-precision arguments: alpha(n_cs) = 2 pi n_cs / 12 (srsran_pucch_alpha_format1 / 2), the
// format 3 DFT arguments 2 pi i k / 12 by the product i k (not reduced), the arguments 2 pi k / 5 of the N_SF = 5
// orthogonal sequences and those of the exp(j pi floor(n_cs_cell / 64) / 2) phase.
struct TxConsts {
  float alpha[12];
  float dft[122];
  float w5[5];
  float ph[4];
};
constexpr TxConsts make_consts()
{
  TxConsts t{};
  for (int i = 0; i < 12; i++) {
    t.alpha[i] = (float)(2.0 * kPi * (double)i / 12.0);
  }
  for (int p = 0; p < 122; p++) {
    t.dft[p] = (float)(2.0 * kPi * (double)p / 12.0);
  }
  for (int k = 0; k < 5; k++) {
    t.w5[k] = (float)(2.0 * kPi * (double)k / 5.0);
  }
  for (int q = 0; q < 4; q++) {
    t.ph[q] = (float)(kPi * (double)q / 2.0);
  }
  return t;
}
#if defined(__HIP_DEVICE_COMPILE__)
__device__ const TxConsts kConsts = make_consts();
#else
const TxConsts kConsts = make_consts();
#endif
__host__ __device__ inline const TxConsts& consts() { return kConsts; }
__host__ __device__ inline float alpha_of(uint32_t n_cs) { return consts().alpha[n_cs % 12u]; }
__host__ __device__ inline float dft_arg(uint32_t p) { return consts().dft[p < 122u ? p : 0u]; }

__host__ __device__ inline float2 cmul(float2 a, float2 b)
{
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__host__ __device__ inline float2 cexp_arg(float a) { return make_float2(cosf(a), sinf(a)); }

// Tables 5.4.1-1 / 5.4.2-1: d of one or two bits
__host__ __device__ inline float2 bpsk_qpsk_f1(uint32_t format_bits, uint32_t b0, uint32_t b1)
{
  if (format_bits == 0) {
    return make_float2(1.f, 0.f);
  }
  if (format_bits == 1) {
    return make_float2(b0 ? -1.f : 1.f, 0.f);
  }
  if (!b0) {
    return b1 ? make_float2(0.f, -1.f) : make_float2(1.f, 0.f);
  }
  return b1 ? make_float2(-1.f, 0.f) : make_float2(0.f, 1.f);
}

// QPSK symbol j of the scrambled coded bits (36.211 Table 7.1.2-1)
__host__ __device__ inline float2 qpsk(uint64_t b, uint32_t j)
{
  const float a = 0.70710678118654752440f;
  return make_float2(((b >> (2 * j)) & 1u) ? -a : a, ((b >> (2 * j + 1)) & 1u) ? -a : a);
}

// r_u,0^(alpha)(n) of zc_sequence.c: the argument in single precision, one rounding of the sum
__host__ __device__ inline float2 r_uv(const PucchTxUe& u, uint32_t s, uint32_t n_cs, uint32_t n)
{
  const float base = (float)u.phi[s][n] * 0.78539816339744830962f;
  return cexp_arg(fmaf(alpha_of(n_cs), (float)n, base));
}

// Table 5.4.2A-1: w_n_oc(t) for N_SF = 5 (exp(j 2 pi n_oc t / 5)) and N_SF = 4
__host__ __device__ inline float2 f3_cover(uint32_t n_sf, uint32_t n_oc, uint32_t t)
{
  if (n_sf == 5) {
    const uint32_t k = (n_oc * t) % 5u;
    return k ? cexp_arg(consts().w5[k]) : make_float2(1.f, 0.f);
  }
  const uint32_t neg = (0x6ca0u >> (4 * (n_oc & 3u) + (t & 3u))) & 1u;  // rows ++++, +-+-, ++--, +--+
  return make_float2(neg ? -1.f : 1.f, 0.f);
}

}  // namespace

__host__ __device__ float2 pucch_tx_re(const PucchTxUe& u, uint32_t s, bool is_rs, uint32_t i, uint32_t n)
{
  const bool f1 = u.format <= 2, f3 = u.format == 6;
  if (is_rs) {  // refsignal_ul.c:458-507
    float2 z = cexp_arg(u.rs_warg[s][i]);
    if (i == 1 && (u.format == 4 || u.format == 5)) {
      z = cmul(z, bpsk_qpsk_f1(u.format - 3, u.drs[0], u.drs[1]));
    }
    return cmul(r_uv(u, s, u.rs_ncs[s][i], n), z);
  }
  if (f1) {  // pucch.c:417-436
    const float2 d0 = bpsk_qpsk_f1(u.format, (uint32_t)(u.bits & 1u), (uint32_t)((u.bits >> 1) & 1u));
    return cmul(r_uv(u, s, u.data_ncs[s][i], n), cmul(d0, cexp_arg(u.data_warg[s][i])));
  }
  const uint64_t b = u.bits ^ u.scr;
  if (!f3) {  // pucch.c:412-415: d(s N_SF + i), N_SF = 5
    return cmul(r_uv(u, s, u.data_ncs[s][i], n), qpsk(b, s * u.n_sf[s] + i));
  }
  // format 3, pucch.c:474-501: y(i') = h d((i' + n_cs_cell) mod 12 + 12 s), then the DFT bin n over sqrt(12)
  const uint32_t ncs = u.data_ncs[s][i];
  const float2   ph  = cexp_arg(consts().ph[(ncs / 64u) & 3u]);
  const float2   h   = cmul(f3_cover(s ? u.n_sf[1] : 5u, u.f3_noc[s], i), ph);
  float2         acc = make_float2(0.f, 0.f);
  for (uint32_t k = 0; k < 12; k++) {
    const float2 y  = cmul(h, qpsk(b, 12 * s + (k + ncs) % 12u));
    const float  a  = dft_arg(k * n);
    const float2 t  = cmul(y, make_float2(cosf(a), -sinf(a)));
    acc             = make_float2(acc.x + t.x, acc.y + t.y);
  }
  const float r12 = sqrtf(12.0f);
  return make_float2(acc.x / r12, acc.y / r12);
}

__global__ __launch_bounds__(PTX_THREADS) void pucch_tx_kernel(const PucchTxUe* __restrict__ ues)
{
  const PucchTxUe& u = ues[blockIdx.y];
  const uint32_t   l = blockIdx.x;
  if (l >= 2 * u.nsym_slot) {
    return;
  }
  const uint32_t s = l >= u.nsym_slot ? 1u : 0u, ls = l - s * u.nsym_slot;
  int            rs = -1, data = -1;  // which DMRS / data symbol of the slot this grid symbol is
  for (uint32_t m = 0; m < u.n_rs && m < PUCCH_MAX_RS; m++) {
    if (u.rs_sym[m] == ls) {
      rs = (int)m;
    }
  }
  for (uint32_t i = 0; i < u.n_sf[s] && i < PUCCH_MAX_SF; i++) {
    if (u.data_sym[i] == ls) {
      data = (int)i;
    }
  }
  const bool     active = rs >= 0 || data >= 0;
  const uint32_t k0     = u.n_prb[s] * 12;
  if (u.grid && u.zero_rest) {
    float2* row = u.grid + (size_t)l * u.ncell_re;
    if ((((uintptr_t)row) & 15u) == 0 && (u.ncell_re & 1u) == 0) {  // two REs a lane, the PRB is 6 such pairs
      float4*        row4 = (float4*)row;
      const uint32_t p0   = k0 / 2;
      for (uint32_t j = threadIdx.x; j < u.ncell_re / 2; j += PTX_THREADS) {
        if (!active || j < p0 || j >= p0 + 6) {
          row4[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    } else {
      for (uint32_t j = threadIdx.x; j < u.ncell_re; j += PTX_THREADS) {
        if (!active || j < k0 || j >= k0 + 12) {
          row[j] = make_float2(0.f, 0.f);
        }
      }
    }
  }
  const uint32_t n = threadIdx.x;
  if (!active || n >= 12 || k0 + 12 > u.ncell_re) {
    return;
  }
  const bool     is_rs = rs >= 0;
  const uint32_t i     = (uint32_t)(is_rs ? rs : data);
  const float2   v     = pucch_tx_re(u, s, is_rs, i, n);
  if (u.grid) {
    u.grid[(size_t)l * u.ncell_re + k0 + n] = v;
  }
  if (is_rs && u.r_out) {
    u.r_out[(s * u.n_rs + i) * 12 + n] = v;
  }
  if (!is_rs && u.z_out) {
    u.z_out[(s * u.n_sf[0] + i) * 12 + n] = v;
  }
}

hipError_t pucch_tx_launch(const PucchTxUe* d_ues, uint32_t nue, hipStream_t stream)
{
  if (nue == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pucch_tx_kernel, dim3(14, nue), dim3(PTX_THREADS), 0, stream, d_ues);
  return hipGetLastError();
}

}  // namespace srsran_amd
