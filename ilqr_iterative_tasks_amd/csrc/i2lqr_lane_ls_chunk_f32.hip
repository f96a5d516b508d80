// The bicycles' one-problem-per-lane kernel with the line search (i2lqr_lane_ls.hpp) as a chunk of the chunked,
// compacting solve ("lane_model_chunks"), in fp32: a translation unit of its own, so that the kernels
// of the other lane units stay as they are.
#include "i2lqr_lane_ls.hpp"

namespace i2lqr {
I2LQR_LANE_LS_CHUNK_KERNELS(template __global__, float)
}  // namespace i2lqr
