// srsran_4g_amd/csrc/pusch_tx_kernel.hip -- PUSCH transmit kernels (UE side) for CDNA4.
//
//   pusch_tx_mux_kernel   UL-SCH / CQI multiplexing and the channel interleaver of 36.212 5.2.2.7-8 as a gather
//                         (ulsch_interleave, sch.c:661-991: rows outer, columns inner, RI cells skipped), the RI / ACK
//                         overrides (sch.c:1320-1333), scrambling with the placeholder / repetition rule
//                         (pusch.c:307-331) and the constellation (srsran_mod_modulate_bytes).  A thread owns
//                         PUSCH_TX_SYM_PER_THREAD = 4 consecutive symbols of q: their 4 Qm bits are Qm / 2 whole bytes of
//                         the packed q outputs, so no two threads share a byte.  The source of a symbol at (row, column)
//                         is closed form: its row-major index minus the RI cells before it; RI symbol i sits in row
//                         rows - 1 - i / 4 of column set[(3 i) mod 4] (uci.c:364-416), so column set[c] holds RI in
//                         its bottom n_c rows.
//   pusch_tx_grid_kernel  srsran_dft_precoding (forward M-point DFT / sqrt(M), M = 12 L) of a data symbol in LDS with
//                         the stages of dft_mixed_dev.h (the forward transform is the conjugate of the backward one of
//                         the conjugate), stored at n_prb_tilde[slot] (pusch_cp, pusch.c:48-95); the DMRS symbols copy
//                         their sequence (refsignal_ul.c:194-225).  One workgroup per (grid symbol, entry).
//   pusch_tx_norm_kernel  apply_norm (ue_ul.c:246-299): the peak of |re|, |im| over the subframe (a maximum, so the
//                         reduction shape does not matter), the clamped factor, the scale.  One workgroup per entry.
//
// The mux kernel reads Qm bytes of bits per symbol and writes 8 B + Qm / 4 B: it is bound by the byte-per-bit reads
// and the three table jumps of the Gold sequence per thread; the grid kernel is LDS-resident (2 x 9.6 KB at M = 1200)
// and moves 16 B per RE; the norm kernel reads the subframe twice (the second time from L2).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "dft_mixed_dev.h"
#include "llr_kernel.h"
#include "pusch_tx_kernel.h"
#include "seq_mod_dev.h"

namespace srsran_amd {

static constexpr int MUX_THREADS  = 256;
static constexpr int NORM_THREADS = 1024;

__constant__ GoldTables kGoldTx;  // this file's copy of the jump tables (gold_tables_get)

// LFSR states at bit offset `off` (< 2^24) of the sequence for `seed` (as llr_kernel.hip's gold_at)
__device__ __forceinline__ void gold_at_tx(uint32_t seed, uint32_t off, uint32_t& x1, uint32_t& x2)
{
  x1 = kGoldTx.x1_nc;
  x2 = apply(kGoldTx.x2_nc, seed & 0x7FFFFFFFu);
#pragma unroll
  for (int lvl = 0; lvl < JUMP_LVLS; lvl++) {
    const uint32_t b = (off >> (8 * lvl)) & 255u;
    if (b) {
      const uint32_t* t = kGoldTx.jump + (((size_t)lvl * 256 + b) * 2) * 32;
      x1                = apply_cols(t, x1);
      x2                = apply_cols(t + 32, x2);
    }
  }
}

static hipError_t gold_tx_init()
{
  // per device, as gold_tables_init(); hipMemcpyToSymbol is synchronous, so it runs once before the first launch
  static std::mutex mu;
  static hipError_t done[64];
  static bool       have[64];
  std::lock_guard<std::mutex> lk(mu);
  int               dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    return hipErrorInvalidDevice;
  }
  if (!have[dev]) {
    GoldTables t;
    hipError_t e = gold_tables_get(&t);
    if (e == hipSuccess) {
      e = hipMemcpyToSymbol(HIP_SYMBOL(kGoldTx), &t, sizeof(t));
    }
    done[dev] = e;
    have[dev] = true;
  }
  return done[dev];
}

// rows of column set[c] that hold RI / ACK symbols: symbols i = m, m + 4, .. < Qp with m = (3 c) mod 4
__device__ __forceinline__ uint32_t uci_rows(uint32_t Qp, uint32_t c)
{
  const uint32_t m = (3u * c) & 3u;
  return Qp > m ? (Qp - m + 3u) / 4u : 0u;
}

// ---------------------------------------------------------------- mux + interleave + scramble + map
__global__ __launch_bounds__(MUX_THREADS) void pusch_tx_mux_kernel(const PuschTxUe* __restrict__ ues)
{
  const PuschTxUe& u  = ues[blockIdx.y];
  const uint32_t   t  = blockIdx.x * MUX_THREADS + threadIdx.x;
  const uint32_t   s0 = t * PUSCH_TX_SYM_PER_THREAD;
  if (s0 >= u.H) {
    return;
  }
  const uint32_t Qm = u.Qm, rows = u.rows;

  const uint32_t nB = Qm / 2;  // bytes of q a thread owns: 4 Qm bits

  // the packed g bits (the CQI bits then the TB's): bytes [t nB, (t + 1) nB) while inside g
  if (u.g_pack) {
    const uint32_t ng = u.ncqi + u.ne, nbytes = (ng + 7u) / 8u;
    for (uint32_t j = t * nB; j < (t + 1) * nB && j < nbytes; j++) {
      uint32_t v = 0;
      for (uint32_t k = 0; k < 8; k++) {
        const uint32_t i   = 8 * j + k;
        const uint32_t bit = i < u.ncqi ? u.cqi[i] : (i < ng ? u.e[i - u.ncqi] : 0u);
        v                  = (v << 1) | (bit & 1u);
      }
      u.g_pack[j] = (uint8_t)v;
    }
  }

  // 4 Qm <= 24 sequence bits from bit s0 Qm
  uint32_t x1, x2;
  gold_at_tx(u.seed, s0 * Qm, x1, x2);
  const uint32_t clo = gold16(x1, x2), chi = gold16(x1, x2);
  const uint32_t c   = clo | (chi << 16);

  uint32_t nri[4], nack[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    nri[k]  = uci_rows(u.ri_Qp, k);
    nack[k] = uci_rows(u.ack_Qp, k);
  }

  uint32_t qw = 0, sw = 0;  // the 4 Qm bits before / after scrambling, first bit highest
  for (uint32_t k = 0; k < PUSCH_TX_SYM_PER_THREAD; k++) {
    const uint32_t s = s0 + k;  // H is a multiple of 12: all four symbols exist
    const uint32_t col = s / rows, row = s - col * rows;
    // RI cells before (row, col) in row-major order, and whether this cell is RI / ACK
    const uint8_t* types  = nullptr;
    uint32_t       before = 0;
#pragma unroll
    for (uint32_t cc = 0; cc < 4; cc++) {
      const uint32_t top = rows - nri[cc];  // first RI row of column ri_col[cc]
      if (row > top) {
        before += row - top;
      }
      if (nri[cc] && row >= top) {
        if (u.ri_col[cc] < col) {
          before += 1;
        } else if (u.ri_col[cc] == col) {
          types = u.ri + (size_t)(4u * (rows - 1u - row) + ((3u * cc) & 3u)) * Qm;
        }
      }
      if (nack[cc] && row >= rows - nack[cc] && u.ack_col[cc] == col) {
        types = u.ack + (size_t)(4u * (rows - 1u - row) + ((3u * cc) & 3u)) * Qm;
      }
    }
    const uint32_t gi0 = (row * u.cols + col - before) * Qm;
    uint32_t       idx = 0, prev = 0;
    for (uint32_t b = 0; b < Qm; b++) {
      uint32_t v, type;
      if (types) {
        type = types[b];
        v    = type == TX_BIT_1 ? 1u : 0u;
      } else {
        const uint32_t gi = gi0 + b;
        v    = gi < u.ncqi ? u.cqi[gi] : (u.e && gi - u.ncqi < u.ne ? u.e[gi - u.ncqi] : 0u);
        v &= 1u;
        type = v;
      }
      const uint32_t p  = s * Qm + b;
      uint32_t       sb = v ^ ((c >> (k * Qm + b)) & 1u);
      if (type == TX_BIT_PLACEHOLDER) {
        sb = 1u;
      } else if (type == TX_BIT_REPETITION && p > 1 && b > 0) {  // uci.c puts a repetition bit second in its symbol
        sb = prev;
      }
      prev = sb;
      idx  = (idx << 1) | sb;
      qw   = (qw << 1) | v;
      sw   = (sw << 1) | sb;
    }
    u.d[s] = modulate((int)u.mod, idx);
  }
  for (uint32_t j = 0; j < nB; j++) {
    const uint32_t sh = 8u * (nB - 1u - j);
    if (u.q_pack) {
      u.q_pack[t * nB + j] = (uint8_t)(qw >> sh);
    }
    if (u.s_pack) {
      u.s_pack[t * nB + j] = (uint8_t)(sw >> sh);
    }
  }
}

hipError_t pusch_tx_mux_launch(const PuschTxUe* d_ues, uint32_t nue, uint32_t max_H, hipStream_t stream)
{
  if (nue == 0 || max_H == 0) {
    return hipSuccess;
  }
  hipError_t e = gold_tx_init();
  if (e != hipSuccess) {
    return e;
  }
  const uint32_t per = MUX_THREADS * PUSCH_TX_SYM_PER_THREAD;
  hipLaunchKernelGGL(pusch_tx_mux_kernel, dim3((max_H + per - 1) / per, nue), dim3(MUX_THREADS), 0, stream, d_ues);
  return hipGetLastError();
}

// ---------------------------------------------------------------- transform precoding + mapping + DMRS
__global__ __launch_bounds__(PU_THREADS) void pusch_tx_grid_kernel(const PuschTxUe* __restrict__ ues)
{
  const PuschTxUe& u = ues[blockIdx.y];
  const uint32_t   l = blockIdx.x;
  if (!u.grid || l >= 2 * u.nsym_slot) {
    return;
  }
  __shared__ float2 buf[2][PUSCH_MAX_M];
  const uint32_t    M = u.M, slot = l >= u.nsym_slot ? 1u : 0u;
  const uint32_t    n0 = u.n_tilde[slot] * 12;
  float2*           row = u.grid + (size_t)l * u.ncell_re;
  int               k = -1;  // data symbol index of grid symbol l
  for (uint32_t i = 0; i < u.nof_symb; i++) {
    if (u.data_sym[i] == l) {
      k = (int)i;
    }
  }
  const bool dmrs = l == (slot + 1) * u.nsym_slot - 4;
  if (u.zero_rest) {
    const bool whole = k < 0 && !(dmrs && u.put_dmrs);  // the last symbol of a shortened subframe
    for (uint32_t j = threadIdx.x; j < u.ncell_re; j += PU_THREADS) {
      if (whole || j < n0 || j >= n0 + M) {
        row[j] = make_float2(0.f, 0.f);
      }
    }
  }
  if (dmrs) {
    if (u.put_dmrs) {
      for (uint32_t j = threadIdx.x; j < M; j += PU_THREADS) {
        row[n0 + j] = u.dmrs[slot * M + j];
      }
    }
    return;
  }
  if (k < 0) {
    return;
  }
  const float2* d = u.d + (size_t)k * M;
  for (uint32_t j = threadIdx.x; j < M; j += PU_THREADS) {
    const float2 v = d[j];
    buf[0][j]      = make_float2(v.x, -v.y);
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
  for (uint32_t j = threadIdx.x; j < M; j += PU_THREADS) {
    const float2 v = buf[cur][j];
    row[n0 + j]    = make_float2(v.x * u.dft_norm, -(v.y * u.dft_norm));
  }
}

hipError_t pusch_tx_grid_launch(const PuschTxUe* d_ues, uint32_t nue, hipStream_t stream)
{
  if (nue == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pusch_tx_grid_kernel, dim3(14, nue), dim3(PU_THREADS), 0, stream, d_ues);
  return hipGetLastError();
}

// ---------------------------------------------------------------- normalisation
__global__ __launch_bounds__(NORM_THREADS) void pusch_tx_norm_kernel(const PuschTxUe* __restrict__ ues)
{
  const PuschTxUe& u = ues[blockIdx.x];
  if (!u.samples_in) {
    return;
  }
  __shared__ float red[NORM_THREADS / 64];
  float            peak = 0.f;
  for (uint32_t n = threadIdx.x; n < u.sf_len; n += NORM_THREADS) {
    const float2 v = u.samples_in[n];
    peak           = fmaxf(peak, fmaxf(fabsf(v.x), fabsf(v.y)));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    peak = fmaxf(peak, __shfl_xor(peak, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = peak;
  }
  __syncthreads();
  peak = red[0];
  for (int i = 1; i < NORM_THREADS / 64; i++) {
    peak = fmaxf(peak, red[i]);
  }
  float f     = u.norm_factor;
  bool  scale = true;
  if (u.norm_mode == 0) {  // limit_norm_factor: the comparisons and the quotients in double
    if ((double)(peak * f) > 0.95) {
      f = (float)(0.95 / (double)peak);
    }
    if ((double)(peak * f) < 0.1) {
      f = (float)(0.1 / (double)peak);
    }
  } else {
    scale = peak != 0.0f && peak != INFINITY;
    f     = u.force_peak / peak;
  }
  for (uint32_t n = threadIdx.x; n < u.sf_len; n += NORM_THREADS) {
    const float2 v   = u.samples_in[n];
    u.samples_out[n] = scale ? make_float2(v.x * f, v.y * f) : v;
  }
}

hipError_t pusch_tx_norm_launch(const PuschTxUe* d_ues, uint32_t nue, hipStream_t stream)
{
  if (nue == 0) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pusch_tx_norm_kernel, dim3(nue), dim3(NORM_THREADS), 0, stream, d_ues);
  return hipGetLastError();
}

}  // namespace srsran_amd
