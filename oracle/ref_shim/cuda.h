// oracle/ref_shim/cuda.h -- TEST INFRASTRUCTURE.  See cuda_runtime.h.
#pragma once
#include "cuda_runtime.h"
