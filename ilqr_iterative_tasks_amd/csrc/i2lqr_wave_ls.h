// Launcher of the line-search form of the one-problem-per-wavefront kernel (k_iterate_ls), compiled
// in its own translation unit (i2lqr_wave_ls.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/i2lqr.h"
#include "i2lqr_wave.hpp"

namespace i2lqr {

// Enqueue k_iterate_ls for a.B problems (problem-major layout; the three plants, both precisions,
// with or without stage weights): every iteration tries the `steps` step sizes 2^-j, j = 0 ...
// steps - 1, on lane groups of the wavefront and continues with the cheapest candidate.
// steps: 2, 4 or 8.  lds: the handle's LDS bytes per wavefront (Layout<Sys>(N).total words).
// Returns hipSuccess or the HIP error of the attribute call / launch.
template <class T> hipError_t wave_ls_iterate(const i2lqr_config& cfg, const IterArgs<T>& a,
                                              int steps, size_t lds, hipStream_t stream);

}  // namespace i2lqr
