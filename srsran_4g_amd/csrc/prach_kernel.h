// srsran_4g_amd/csrc/prach_kernel.h -- PRACH detection and generation kernels (prach.c:749-1012).
#ifndef SRSRAN_AMD_PRACH_KERNEL_H
#define SRSRAN_AMD_PRACH_KERNEL_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ofdm_kernel.h"

namespace srsran_amd {

static constexpr uint32_t PRACH_NZC       = 839;
static constexpr uint32_t PRACH_K         = 12;   // DELTA_F / DELTA_F_RA: N_ifft_prach = 12 N
static constexpr uint32_t PRACH_MAX_ROOTS = 64;
static constexpr uint32_t PRACH_MAX_WIN   = 128;  // (root, window) pairs of one occasion: at most 64 + 63

// The N-point transform of an occasion is an OfdmArgs of which only the plan is set (tw, N, nstages, radix,
// ns_magic as ofdm_plan gives them): fft_ip indexes the stage arrays at run time, which stays a scalar load as long as
// the struct lives in the descriptor (global memory) or in the kernel arguments, not in a thread-local copy.

// one occasion of a detect batch
struct PrachOcc {
  OfdmArgs      fft;
  const float2* sig;        // 12 N samples
  const float2* tw_m;       // exp(-2 pi i m / 12N), m < 12 N
  const float2* root_spec;  // [64][839]: the scaled transforms of the 64 sequences
  uint32_t      root_idx[PRACH_MAX_ROOTS];  // sequence index of root i
  uint32_t      b0;         // natural-order bin of the first PRACH bin: (begin + 6 N) mod 12 N
  uint32_t      n_roots;    // roots searched (num_ra_preambles)
  uint32_t      n_cs;
  uint32_t      n_wins;
  float         scale;      // 1 / sqrt(12 N)
};

// per occasion, written by the search kernel
struct PrachOccOut {
  float    avg[PRACH_MAX_ROOTS];    // mean of the 839 |corr|^2 of root i
  float2   cross[PRACH_MAX_ROOTS];  // sum_k c[k] conj(c[k+1]), k < 838, of root i's product spectrum
  float    peak[PRACH_MAX_WIN];     // first maximum of window j of root i at [i * n_wins + j]
  uint32_t off[PRACH_MAX_WIN];      // its offset from the window's start
};

struct PrachGenArgs {
  OfdmArgs      fft;
  const float2* tw_m;
  const float2* spec;  // the sequence's scaled transform, 839 bins
  float2*       out;   // N_cp + N_seq samples
  uint32_t      b0;
  uint32_t      n_cp;
  uint32_t      n_seq;  // 12 N or 24 N
  float         scale;
};

// part: [nocc][12][839] workspace; grid (12, nocc)
hipError_t prach_bins_launch(const PrachOcc* d_occ, float2* part, uint32_t nocc, hipStream_t stream);
// grid (max_roots, nocc); tw839: exp(+2 pi i m / 839), m < 839
hipError_t prach_search_launch(const PrachOcc* d_occ, const float2* part, const float2* tw839, PrachOccOut* out,
                               uint32_t nocc, uint32_t max_roots, hipStream_t stream);
// the forward 839-point DFT of nseq sequences, scaled by 1 / sqrt(839): seqs, spec [nseq][839]
hipError_t prach_seq_dft_launch(const float2* seqs, const float2* tw839, float2* spec, uint32_t nseq,
                                hipStream_t stream);
hipError_t prach_gen_launch(const PrachGenArgs& a, hipStream_t stream);

}  // namespace srsran_amd
#endif
