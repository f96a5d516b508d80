// RCCL, bound at run time (i2lqr_rccl.hip).  The one collective of the path is an
// all-gather of the candidates' terminal costs.  libi2lqr_hip.so does not link librccl: a process
// that already carries a copy (PyTorch ships its own librccl.so, the one torch.distributed's "nccl"
// backend uses) must not get a second one, and single-GPU users need none at all.  The first
// communicator call looks for a loaded librccl first and loads the ROCm one otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types and prototypes only

#include "i2lqr_host.hpp"

namespace i2lqr {

struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t,
                            hipStream_t) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t,
                            hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;  // optional: without them the two all-gathers of a
  ncclResult_t (*GroupEnd)() = nullptr;    // round are issued one after the other
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
  char why[256] = "";  // the loader's message, captured once (dlerror() is cleared by reading it)
};

const RcclApi& rccl_api();  // bound on first use

}  // namespace i2lqr

#define RCCL_TRY(api, expr)                                                                        \
  do {                                                                                             \
    ncclResult_t r_ = (expr);                                                                      \
    if (r_ != ncclSuccess)                                                                         \
      return ::i2lqr::fail(I2LQR_ERR_LAUNCH, "%s failed: %s", #expr, (api).GetErrorString(r_));    \
  } while (0)
