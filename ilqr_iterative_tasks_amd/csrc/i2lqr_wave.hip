// The one-problem-per-wavefront kernels (i2lqr_wave.hpp), fp64 and fp32: a translation unit of
// their own (i2lqr_kernels.h), so that the library's units compile side by side.
#include "i2lqr_kernels.h"

namespace i2lqr {
I2LQR_WAVE_KERNELS(template __global__, double)
I2LQR_WAVE_KERNELS(template __global__, float)
}  // namespace i2lqr
