// The recorder behind the dry-run launches (i2lqr_dryrun.hpp): compiled into every build, empty
// without -DI2LQR_DRY_RUN (the sanitizer build); host code only.
#include "i2lqr_dryrun.hpp"

#ifdef I2LQR_DRY_RUN
#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "i2lqr_geometry.hpp"

namespace i2lqr {
namespace dry {
namespace {
struct State {
  std::mutex mu;
  std::vector<std::pair<uintptr_t, uintptr_t>> ranges;
  std::string text;
  int64_t launches = 0, violations = 0;
};
State& st() {
  static State s;
  return s;
}
}  // namespace
bool on() {
  static const bool v = [] {
    const char* e = getenv("I2LQR_DRY_RUN");
    return e && e[0] == '1';
  }();
  return v;
}
void allow(const void* base, size_t bytes) {
  std::lock_guard<std::mutex> lock(st().mu);
  st().ranges.emplace_back((uintptr_t)base, (uintptr_t)base + bytes);
}
void reset() {
  std::lock_guard<std::mutex> lock(st().mu);
  st().ranges.clear();
  st().text.clear();
  st().launches = st().violations = 0;
}
// the record being built by this thread (launch(): record, the arguments, end)
thread_local std::string t_line, t_kernel;
void record(const char* expr, const void* kernel, dim3 grid, dim3 block, size_t lds) {
  t_kernel = expr;
  Dl_info info;
  if (dladdr(kernel, &info) && info.dli_sname && info.dli_saddr == kernel) {
    int status = 0;
    char* name = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
    t_kernel = status == 0 && name ? name : info.dli_sname;
    free(name);
  }
  char line[96];
  snprintf(line, sizeof(line), " grid %u block %u lds %zu", grid.x, block.x, lds);
  t_line = "launch " + t_kernel + line;
  std::lock_guard<std::mutex> lock(st().mu);
  st().launches++;
  const DeviceGeometry& g = device_geometry();
  if (grid.x == 0 || block.x == 0 || block.x > 1024 || lds > g.max_dyn_lds) {
    st().violations++;
    st().text += "VIOLATION " + t_kernel + ": launch shape" + line + "\n";
  }
}
void ptr(const char* field, const void* p) {
  char buf[96];
  if (!p) {
    snprintf(buf, sizeof(buf), " %s=0", field);
    t_line += buf;
    return;
  }
  std::lock_guard<std::mutex> lock(st().mu);
  const uintptr_t a = (uintptr_t)p;
  for (size_t r = 0; r < st().ranges.size(); r++)
    if (a >= st().ranges[r].first && a < st().ranges[r].second) {
      snprintf(buf, sizeof(buf), " %s=r%zu+%zu", field, r, (size_t)(a - st().ranges[r].first));
      t_line += buf;
      return;
    }
  snprintf(buf, sizeof(buf), " %s=?", field);
  t_line += buf;
  st().violations++;
  char line[160];
  snprintf(line, sizeof(line), ": %s = %p lies in no declared range\n", field, p);
  st().text += "VIOLATION " + t_kernel + line;
}
void val(const char* field, int64_t v) {
  char buf[96];
  snprintf(buf, sizeof(buf), " %s=%lld", field, (long long)v);
  t_line += buf;
}
void end() {
  std::lock_guard<std::mutex> lock(st().mu);
  if (st().text.size() < (1u << 21)) st().text += t_line + "\n";
}
int64_t report(char* buf, int64_t n) {
  std::lock_guard<std::mutex> lock(st().mu);
  if (buf && n > 0) {
    // violations first: the buffer may be shorter than the launch log
    std::string out;
    size_t pos = 0;
    while ((pos = st().text.find("VIOLATION", pos)) != std::string::npos) {
      const size_t end = st().text.find('\n', pos);
      out += st().text.substr(pos, end == std::string::npos ? std::string::npos : end - pos + 1);
      if (end == std::string::npos) break;
      pos = end + 1;
    }
    out += st().text;
    snprintf(buf, (size_t)n, "%s", out.c_str());
  }
  st().text.clear();
  const int64_t v = st().violations;
  st().violations = 0;
  return v;
}
}  // namespace dry
}  // namespace i2lqr
#endif
