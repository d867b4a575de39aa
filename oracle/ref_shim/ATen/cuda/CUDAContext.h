// oracle/ref_shim/ATen/cuda/CUDAContext.h -- TEST INFRASTRUCTURE.  The stream the
// reference's launchers ask for: whatever ref_set_stream() (entry.hip) stored
// last, the null stream by default.
#pragma once
#include <hip/hip_runtime.h>

namespace at {
namespace cuda {
hipStream_t getCurrentCUDAStream();
}
}
