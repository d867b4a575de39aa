// oracle/ref_shim/cuda_runtime.h -- TEST INFRASTRUCTURE.  Stands in for the CUDA
// runtime header when the reference's point-op kernels are compiled, unmodified
// and in place, as HIP (oracle/ref_build.py).  Only what those six sources use.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

typedef hipError_t cudaError_t;
#define cudaSuccess hipSuccess
#define cudaGetLastError hipGetLastError
#define cudaGetErrorString hipGetErrorString

// Host min/max on ints (cuda_utils.cuh: optimal_num_threads) come from HIP's own
// math header, as do the same-type device overloads.
//
// Mixed float/double device overloads, as CUDA's math API documents them
// (min(float, double) -> double, ...): interpolate/neighbor_interpolate.cu:61-63
// calls min(1e10f, <double>) and max(<double>, 1e-10f).  Without these four HIP
// picks its catch-all template for mixed arithmetic arguments (__HIP_OVERLOAD2
// in clang's __clang_hip_cmath.h), which casts both to double and calls
// min/max(double, double): the same value, by a rule of HIP's own.  Declared
// here so the call resolves by the rule nvcc applies, not by a coincidence of
// the HIP headers: the clamp runs in double and the running bests stay double
// until the products of :64-66 round them to float.
__device__ inline double min(float a, double b) { return fmin((double)a, b); }
__device__ inline double min(double a, float b) { return fmin(a, (double)b); }
__device__ inline double max(float a, double b) { return fmax((double)a, b); }
__device__ inline double max(double a, float b) { return fmax(a, (double)b); }
