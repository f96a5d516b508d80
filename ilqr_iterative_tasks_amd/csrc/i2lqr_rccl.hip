// The run-time binding of librccl (i2lqr_rccl.hpp); host code only.
#include "i2lqr_rccl.hpp"

#include <dlfcn.h>

#include <cstdio>

namespace i2lqr {

const RcclApi& rccl_api() {
  static const RcclApi api = [] {
    RcclApi a;
    for (const char* name : {"librccl.so", "librccl.so.1"})
      if ((a.lib = dlopen(name, RTLD_NOW | RTLD_NOLOAD))) break;
    if (!a.lib)
      for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if ((a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!a.lib) {
      const char* e = dlerror();
      snprintf(a.why, sizeof(a.why), "%s", e ? e : "librccl.so not found by the dynamic loader");
      return a;
    }
    auto sym = [&](const char* n) { return dlsym(a.lib, n); };
    a.GetUniqueId = (decltype(a.GetUniqueId))sym("ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))sym("ncclCommInitRank");
    a.CommDestroy = (decltype(a.CommDestroy))sym("ncclCommDestroy");
    a.CommAbort = (decltype(a.CommAbort))sym("ncclCommAbort");
    a.CommCount = (decltype(a.CommCount))sym("ncclCommCount");
    a.CommUserRank = (decltype(a.CommUserRank))sym("ncclCommUserRank");
    a.AllGather = (decltype(a.AllGather))sym("ncclAllGather");
    a.Broadcast = (decltype(a.Broadcast))sym("ncclBroadcast");
    a.GroupStart = (decltype(a.GroupStart))sym("ncclGroupStart");
    a.GroupEnd = (decltype(a.GroupEnd))sym("ncclGroupEnd");
    a.GetErrorString = (decltype(a.GetErrorString))sym("ncclGetErrorString");
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.CommAbort && a.CommCount &&
           a.CommUserRank && a.AllGather && a.Broadcast && a.GetErrorString;
    if (!a.ok) snprintf(a.why, sizeof(a.why), "the loaded librccl lacks a symbol this library binds");
    return a;
  }();
  return api;
}

}  // namespace i2lqr
