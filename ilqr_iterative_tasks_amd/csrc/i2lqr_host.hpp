// Host-side error reporting shared by the library's host translation units: no exception crosses
// the C-ABI, every entry point returns an int code and records a thread-local message for
// i2lqr_last_error().
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/i2lqr.h"

namespace i2lqr {

// records the (printf-formatted) message of the calling thread and returns `code`; the one message
// buffer lives in i2lqr_abi.hip
int fail(int code, const char* fmt, ...);

}  // namespace i2lqr

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return ::i2lqr::fail(I2LQR_ERR_LAUNCH, "%s failed: %s", #expr, hipGetErrorString(e_));  \
  } while (0)
