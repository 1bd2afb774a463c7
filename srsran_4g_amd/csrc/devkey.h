// srsran_4g_amd/csrc/devkey.h -- the current HIP device, used to key every process-wide device table
// cache (QPP tables, rate de-matching tables, CRC shift tables, FFT twiddles, Gold jump tables,
// per-device streams).  One process may drive several GPUs, one host thread per GPU:
// a table built on device 0 must never be handed to a kernel launched on device 1.  Also the library's one
// "is there a HIP device at all" test, which every *_init asks.
#pragma once
#include <hip/hip_runtime.h>

namespace srsran_amd {

inline int cur_dev()
{
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) {
    return 0;
  }
  return d;
}

// whether the process sees a HIP device at all: asked once, and the function-local static needs no lock
inline bool have_gpu()
{
  static const bool have = [] {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
  }();
  return have;
}

}  // namespace srsran_amd
