// The bicycles' one-problem-per-lane kernel with the opt-in models (i2lqr_lane_model.hpp) in fp32: a
// translation unit of its own, so that the kernels of i2lqr_lane_f32.hip stay as they are.
#include "i2lqr_lane_model.hpp"

namespace i2lqr {
I2LQR_LANE_MODEL_KERNELS(template __global__, float)
}  // namespace i2lqr
