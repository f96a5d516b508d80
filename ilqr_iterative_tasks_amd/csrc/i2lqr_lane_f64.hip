// The bicycles' one-problem-per-lane kernels (i2lqr_lane.hpp) and the compaction in fp64: a
// translation unit of their own (i2lqr_kernels.h), so that the library's units compile side by side.
#include "i2lqr_kernels.h"

namespace i2lqr {
I2LQR_LANE_KERNELS(template __global__, double)
}  // namespace i2lqr
