// srsran_4g_amd/csrc/ul_internal.h -- what the uplink host units need of one another: the chest_ul objects' device
// state (chest_ul_api.cpp; the PUSCH receiver reads the estimator's DMRS table and device estimate) and their
// accessors for pucch_api.cpp, the PUSCH transmit step (pusch_api.cpp) that ue_ul_api.cpp batches, and
// srsran_pucch_encode up to the kernel (pucch_api.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/srsran_pucch.h"
#include "../../include/srsran_pusch.h"
#include "dev_buf.h"
#include "pucch_tx_kernel.h"
#include "pusch_kernel.h"
#include "pusch_tx_kernel.h"
#include "refsignal_ul_host.h"

namespace srsran_amd {

// ---------------- chest_ul device state ----------------
struct ChestUlGpu {
  hipStream_t         stream = nullptr;
  uint32_t            max_prb = 0;
  UlHopping           hop;
  bool                hop_ok = false;
  DevBuf<float2>      d_dmrs;    // [cs][sf][valid n <= cell prb] 2 * 12 n values
  std::vector<size_t> dmrs_off;  // (cs * 10 + sf) * 101 + n -> offset (values)
  DevBuf<float2>      d_grid;    // one subframe grid
  DevBuf<PuschUe>     d_desc;
  // srsran_chest_ul_pregen with an SRS configuration: the known sequence comes from these (chest_ul.c:633-634)
  bool                              srs_configured = false;
  srsran_refsignal_srs_cfg_t        srs_cfg;
  srsran_refsignal_dmrs_pusch_cfg_t srs_dmrs_cfg;
  DevBuf<uint8_t>                   d_srs_desc;  // the SRS descriptors of a batch this object's scratch serves
};

struct ChestUlResGpu {
  DevBuf<float2>     d_ce;  // nof_re values
  DevBuf<ChestUlOut> d_out;
  uint32_t    nof_re = 0;
  bool        valid  = false;   // d_ce holds the last estimate written to ce
  // an SRS estimate enqueued on the device side and not yet fetched: where its ce row lies and how long it is
  bool        srs_pending = false;
  size_t      srs_off = 0;
  uint32_t    srs_n = 0;
};

inline size_t dmrs_index(uint32_t cs, uint32_t sf, uint32_t n) { return ((size_t)cs * SRSRAN_NOF_SF_X_FRAME + sf) * 101 + n; }

// chest_ul_api.cpp: the estimator's part of a PUSCH descriptor, and the result's scalars from the kernel's output
void fill_chest_desc(PuschUe& u, const srsran_chest_ul_t* q, const srsran_pusch_cfg_t* cfg, uint32_t M);
void finish_chest_res(srsran_chest_ul_res_t* res, const ChestUlOut& o);

// what the PUCCH estimator (pucch_api.cpp) needs of the chest objects: the stream, a device
// scratch of `bytes` (the grid buffer, grown), and a note that res->ce was rewritten on the host
hipStream_t chest_ul_stream(srsran_chest_ul_t* q);
void*       chest_ul_scratch(srsran_chest_ul_t* q, size_t bytes);
void        chest_ul_res_host_changed(srsran_chest_ul_res_t* res);

// pusch_api.cpp: check a PUSCH allocation against the estimator / cell (chest_ul.c:409-414, pusch.c:392-410)
int check_alloc(const srsran_cell_t& cell, const srsran_pusch_cfg_t* cfg);

// One transmission of a batch: the PUSCH object of its cell, where its grid goes and, for the UE uplink path, the
// DMRS tables and the normalisation of its samples.
struct TxReq {
  srsran_pusch_t*                          pusch;
  const UlHopping*                         hop;  // DMRS put (null: none)
  const srsran_refsignal_dmrs_pusch_cfg_t* dmrs_cfg;
  srsran_ul_sf_cfg_t*                      sf;
  srsran_pusch_cfg_t*                      cfg;
  const srsran_uci_value_t*                uci;
  const uint8_t*                           d_data;
  float2*                                  d_grid;
  bool                                     zero_rest;
  const float2*                            samples_in;  // null: no normalisation stage
  float2*                                  samples_out;
  uint32_t                                 sf_len, norm_mode;
  float                                    norm_factor, force_peak;
};

// pusch_api.cpp: srsran_pusch_encode for n transmissions up to the grids
int pusch_tx_run(srsran_pusch_t* owner, uint32_t n, const TxReq* r, std::vector<PuschTxUe>& desc,
                 const PuschTxUe** d_desc, hipStream_t st, const std::vector<PuschTxUe>& extra = {});

// pucch_api.cpp: srsran_pucch_encode up to the kernel
int pucch_tx_prepare(const srsran_cell_t& cell, const srsran_ul_sf_cfg_t* sf, srsran_pucch_cfg_t* cfg,
                     const srsran_uci_value_t* uci, PucchTxUe* d);

}  // namespace srsran_amd
