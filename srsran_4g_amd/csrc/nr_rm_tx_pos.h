// srsran_4g_amd/csrc/nr_rm_tx_pos.h -- position arithmetic of the NR LDPC rate matcher, transmit side.
//
// Closed forms of what ldpc_rm.c and sch_nr.c compute with sequential walks:
//   k0 / Ncb of a redundancy version                       init_rm, ldpc_rm.c:113-167
//   the rank-th non-filler position counted from k0        bit_selection_rm_tx, ldpc_rm.c:173-193
//   the bit interleaver out[j Qm + i] = sel[i cols + j]    bit_interleaver_rm_tx, ldpc_rm.c:348-360
//   E of the j-th code block of a TB and where it starts   sch_nr_get_E, sch_nr.c:178-189
// The filler bits of a stored codeword (first 2Z bits punctured) are one range [ini, end).  Plain inline
// code for the host and the device: the fused epilogue of nr_sch_tx_kernel.hip, the stand-alone
// srsran_ldpc_rm_tx kernel and a host program (tests/nr_rm_tx_pos_check.cpp) all include it.
#ifndef SRSRAN_AMD_NR_RM_TX_POS_H
#define SRSRAN_AMD_NR_RM_TX_POS_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NR_RM_HD __host__ __device__ inline
#else
#define NR_RM_HD inline
#endif

namespace srsran_amd {

// bit selection of one code block: circle [0, Ncb) read from k0, fillers [fi, fe) (clamped to the circle)
struct NrRmTxSel {
  uint32_t k0, Ncb;
  uint32_t fi, fe;  // filler positions inside the circle
  uint32_t L;       // non-filler positions on the circle: the period of the selection
  uint32_t a1;      // lap 1 (k0 .. Ncb - 1): non-filler positions before the fillers
  uint32_t s1;      // lap 1: first position after them
  uint32_t lap1;    // non-filler positions of lap 1
  uint32_t b2;      // lap 2 (0 .. k0 - 1): non-filler positions before the fillers
};

// ldpc_rm.c:50, 126, 157-164 (bg: 0 = BG1, 1 = BG2)
NR_RM_HD void nr_rm_tx_k0_ncb(uint32_t bg, uint32_t Z, uint32_t rv, uint32_t Nref, uint32_t* k0, uint32_t* Ncb)
{
  const uint32_t basek0 = bg == 0 ? (rv == 0 ? 0u : rv == 1 ? 17u : rv == 2 ? 33u : 56u)
                                  : (rv == 0 ? 0u : rv == 1 ? 13u : rv == 2 ? 25u : 43u);
  const uint32_t N      = Z * (bg == 0 ? 66u : 50u);
  if (N <= Nref) {
    *Ncb = N;
    *k0  = Z * basek0;
  } else {
    *Ncb = Nref;
    *k0  = Z * ((basek0 * Nref) / N);
  }
}

NR_RM_HD NrRmTxSel nr_rm_tx_sel(uint32_t k0, uint32_t Ncb, uint32_t fill_ini, uint32_t fill_end)
{
  NrRmTxSel s;
  s.k0   = k0;
  s.Ncb  = Ncb;
  s.fi   = fill_ini < Ncb ? fill_ini : Ncb;
  s.fe   = fill_end < Ncb ? fill_end : Ncb;
  s.fe   = s.fe > s.fi ? s.fe : s.fi;
  s.L    = Ncb - (s.fe - s.fi);
  s.a1   = k0 < s.fi ? s.fi - k0 : 0u;
  s.s1   = k0 > s.fe ? k0 : s.fe;
  s.lap1 = s.a1 + (Ncb > s.s1 ? Ncb - s.s1 : 0u);
  s.b2   = s.fi < k0 ? s.fi : k0;
  return s;
}

// position of the rank-th selected bit, rank < L (the walk of ldpc_rm.c:185-192 for k = rank)
NR_RM_HD uint32_t nr_rm_tx_pos(const NrRmTxSel& s, uint32_t rank)
{
  if (rank < s.lap1) {
    return rank < s.a1 ? s.k0 + rank : s.s1 + (rank - s.a1);
  }
  const uint32_t r2 = rank - s.lap1;
  return r2 < s.b2 ? r2 : s.fe + (r2 - s.b2);
}

// index into the selected bits of output bit t = j Qm + i: i cols + j, cols = E / Qm (ldpc_rm.c:355-358)
NR_RM_HD uint32_t nr_rm_tx_il(uint32_t j, uint32_t i, uint32_t cols) { return i * cols + j; }

// E of the j-th transmitted code block and the sum of the earlier ones (sch_nr.c:178-189, 534-548)
struct NrSchE {
  uint32_t E0, E1, jthr;  // E_j = j <= jthr ? E0 : E1
};

NR_RM_HD NrSchE nr_sch_E(uint32_t G, uint32_t Nl, uint32_t Qm, uint32_t Cp)
{
  NrSchE         e;
  const uint32_t qn = Nl * Qm;
  e.E0              = qn * (G / (qn * Cp));
  e.E1              = qn * ((G + qn * Cp - 1) / (qn * Cp));
  e.jthr            = Cp - (G / qn) % Cp - 1;
  return e;
}

NR_RM_HD uint32_t nr_sch_E_of(const NrSchE& e, uint32_t j) { return j <= e.jthr ? e.E0 : e.E1; }

NR_RM_HD uint32_t nr_sch_E_offset(const NrSchE& e, uint32_t j)
{
  const uint32_t n0 = j <= e.jthr ? j : e.jthr + 1;
  return n0 * e.E0 + (j - n0) * e.E1;
}

}  // namespace srsran_amd
#endif
