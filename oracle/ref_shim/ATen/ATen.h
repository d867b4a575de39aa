// oracle/ref_shim/ATen/ATen.h -- TEST INFRASTRUCTURE.  The reference's kernels
// include ATen only for the current stream (ATen/cuda/CUDAContext.h); no tensor
// type reaches a .cu file.
#pragma once
