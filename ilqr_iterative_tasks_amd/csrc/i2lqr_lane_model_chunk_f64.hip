// The bicycles' one-problem-per-lane kernel with the opt-in models (i2lqr_lane_model.hpp) as a chunk of the chunked,
// compacting solve ("lane_model_chunks"), in fp64: a translation unit of its own, so that the kernels
// of the other lane units stay as they are.
#include "i2lqr_lane_model.hpp"

namespace i2lqr {
I2LQR_LANE_OPT_KERNELS(template __global__, k_lane_chunk_model, I2LQR_LANE_TAIL_CHUNK_MODEL, double)
}  // namespace i2lqr
