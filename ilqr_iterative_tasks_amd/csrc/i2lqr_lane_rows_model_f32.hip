// k_lane_iterate_rows_model of quad12 in fp32 with Q = R = 0 ("lane_rows_models"): explicit
// instantiations of the template of i2lqr_lane_rows_model.hpp, launched from i2lqr_abi.hip.
#define I2LQR_LANE_ROWS_MODEL_F32_DEFINE
#include "i2lqr_lane_rows_model.hpp"

namespace i2lqr {
I2LQR_LANE_ROWS_MODEL_F32_KERNELS(template __global__)
}  // namespace i2lqr
