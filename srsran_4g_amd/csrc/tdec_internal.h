// srsran_4g_amd/csrc/tdec_internal.h -- host tables of tdec_api.cpp that the encoders (sch_api.cpp, tx_api.cpp) read.
#pragma once
#include <stdint.h>

namespace srsran_amd {

// QPP coefficients of code block size index idx (36.212 Table 5.1.3-3)
void qpp_coeffs(uint32_t idx, uint32_t* f1, uint32_t* f2);

}  // namespace srsran_amd
