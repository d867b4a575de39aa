// host_util.h -- what every entry point of the sources outside the MFMA family (mfma_prims.h has its own) needs around a
// launch: the export macro, the status of the launch just made, the stream cast and the grid's rounding-up division.
#pragma once
#include <hip/hip_runtime.h>

#include "gldm.h"

#define GLDM_API extern "C" __attribute__((visibility("default")))

namespace {

inline int launch_status() { return hipGetLastError() == hipSuccess ? GLDM_OK : GLDM_ERR_LAUNCH; }
inline hipStream_t as_stream(gldm_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

}  // namespace
