// C-ABI of libi2lqr_hip.so (include/i2lqr.h): argument validation, typed device configs and
// kernel dispatch.  No exception crosses the boundary; every entry point returns an int code and
// records a thread-local message for i2lqr_last_error().
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_set>

#include "../../include/i2lqr.h"
#include "i2lqr_devcfg.hpp"
#include "i2lqr_geometry.hpp"
#include "i2lqr_group.h"
#include "i2lqr_handle.hpp"
#include "i2lqr_host.hpp"
#include "i2lqr_kernels.h"
#include "i2lqr_lane12.h"
#include "i2lqr_rccl.hpp"
#include "i2lqr_select.hpp"
#include "i2lqr_wave_opt.h"

// LaneLaunch; brings in i2lqr_dryrun.hpp, whose macros record every launch below as well (empty
// unless -DI2LQR_DRY_RUN: the ASan build)
#include "i2lqr_lane_launch.hpp"
// Launch (behind it: its launches are recorded too)
#include "i2lqr_column_launch.hpp"

using namespace i2lqr;

namespace {
thread_local char g_err[512] = "";
}

int i2lqr::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

namespace i2lqr {
// hipDeviceGetAttribute once per device; I2LQR_FAKE_CUS=<n> (a debug override, parity tests of the
// derived thresholds on the full chip) replaces the CU count.
const DeviceGeometry& device_geometry() {
  constexpr int kMaxDev = 64;
  static DeviceGeometry table[kMaxDev];
  static std::once_flag once[kMaxDev];
  static const DeviceGeometry fallback{};  // no device visible: the MI355X figures
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) {
    (void)hipGetLastError();
    return fallback;
  }
  std::call_once(once[dev], [dev] {
    DeviceGeometry g;
    int v = 0;
    bool ok = true;
    auto attr = [&](hipDeviceAttribute_t a) {
      v = 0;
      const bool got = hipDeviceGetAttribute(&v, a, dev) == hipSuccess && v > 0;
      if (!got) (void)hipGetLastError();
      return got;
    };
    if (attr(hipDeviceAttributeMultiprocessorCount)) g.cus = v; else ok = false;
    if (attr(hipDeviceAttributeWarpSize)) g.wave = v; else ok = false;
    if (attr(hipDeviceAttributeMaxSharedMemoryPerMultiprocessor)) g.lds_per_cu = (size_t)v; else ok = false;
    // what one workgroup can be given: the whole CU's LDS on CDNA (opt-in above the default)
    g.max_dyn_lds = g.lds_per_cu;
    if (attr(hipDeviceAttributeMaxSharedMemoryPerBlock)) {
      g.default_dyn_lds = (size_t)v < g.lds_per_cu ? (size_t)v : g.lds_per_cu;
      if (g.default_dyn_lds > 64 * 1024) g.default_dyn_lds = 64 * 1024;  // opt-in needed above 64 KiB
    }
    g.queried = ok ? 1 : 0;
    if (const char* e = getenv("I2LQR_FAKE_CUS")) {
      const long f = strtol(e, nullptr, 10);
      if (f >= 1 && f <= 4096) { g.cus = (int)f; g.faked = 1; }
    }
    table[dev] = g;
  });
  return table[dev];
}

#ifdef I2LQR_DEBUG
unsigned long long* debug_trap_word() {
  constexpr int kMaxDev = 64;
  static unsigned long long* word[kMaxDev] = {};
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  if (!word[dev]) {
    if (hipMalloc((void**)&word[dev], sizeof(unsigned long long)) != hipSuccess) return nullptr;
    (void)hipMemset(word[dev], 0, sizeof(unsigned long long));
  }
  return word[dev];
}
#else
unsigned long long* debug_trap_word() { return nullptr; }
#endif
}  // namespace i2lqr

#ifdef I2LQR_DEBUG
__global__ void k_debug_self_test(double* buf, unsigned long long* trap) {
  const auto s = i2lqr::make_slice(buf, 8, trap, i2lqr::TAG_WAVE_LDS);
  if (threadIdx.x == 0) s[8] = 1.0;  // one past the end: recorded, redirected to s[0]
}
#endif

namespace {
// Debug build: after a call's launches, wait for the stream and turn a recorded index violation
// into I2LQR_ERR_LAUNCH (the record is cleared).  The product build returns rc untouched and does
// not synchronise.
int debug_check(int rc, void* stream) {
#ifdef I2LQR_DEBUG
  if (rc != I2LQR_OK) return rc;
  unsigned long long* w = i2lqr::debug_trap_word();
  if (!w) return rc;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &cap) == hipSuccess &&
      cap != hipStreamCaptureStatusNone)
    return rc;  // a stream being captured into a graph cannot be waited for: the next eager call checks
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return fail(I2LQR_ERR_LAUNCH, "debug build: the stream reported an error");
  unsigned long long rec = 0;
  if (hipMemcpy(&rec, w, sizeof(rec), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(I2LQR_ERR_LAUNCH, "debug build: could not read the violation record");
  if (rec) {
    (void)hipMemset(w, 0, sizeof(rec));
    static const char* const names[] = {"?", "wave-kernel LDS slice", "eight-lane LDS slice",
                                        "sixteen-lane LDS slice", "quad12 HBM workspace slot",
                                        "lane kernel row of X", "lane kernel row of U / k",
                                        "lane kernel row of K", "lane kernel LDS word",
                                        "compaction row / problem index"};
    const int tag = (int)((rec >> 56) & 0x7f);
    return fail(I2LQR_ERR_LAUNCH, "debug build: index check failed: %s, index %lld, limit %lld",
                names[tag < 10 ? tag : 0], (long long)((rec >> 28) & 0xfffffff),
                (long long)(rec & 0xfffffff));
  }
#else
  (void)stream;
#endif
  return rc;
}
}  // namespace

namespace {

// f(L()) with L the launcher of the handle's layout, precision and plant (validated by i2lqr_create)
template <class F> int dispatch(const i2lqr_handle* h, F&& f) {
  return visit_plant(h->cfg, [&](auto t, auto sys) {
    using T = decltype(t);
    using Sys = decltype(sys);
    if (h->cfg.layout == I2LQR_LAYOUT_BATCH_MINOR) return f(LaneLaunch<T, Sys, false>());
    if (h->cfg.layout == I2LQR_LAYOUT_BATCH_TILED) return f(LaneLaunch<T, Sys, true>());
    return f(Launch<T, Sys>());
  });
}
int dispatch_iterate(i2lqr_handle* h, const SolveIO& io, void* stream) {
  return dispatch(h, [&](auto L) { return L.iterate(h, io, (hipStream_t)stream); });
}

// Live handles: i2lqr_destroy of NULL is a no-op, of a pointer that is not (or no longer) a live
// handle an error code instead of a double free.
std::mutex g_live_mu;
std::unordered_set<const i2lqr_handle*>& live_handles() {
  static std::unordered_set<const i2lqr_handle*> set;
  return set;
}

int check_common(const i2lqr_handle* h, int64_t B) {
  if (!h) return fail(I2LQR_ERR_INVALID, "null handle");
  if (B < 0) return fail(I2LQR_ERR_INVALID, "negative batch %lld", (long long)B);
  if (B > (int64_t)0x7fffffff) return fail(I2LQR_ERR_INVALID, "batch %lld too large", (long long)B);
  return I2LQR_OK;
}

// The arrays a solve call cannot do without (extra_null: one of the call's own is missing), and K
// and k as a pair
int check_io(const SolveIO& io, bool extra_null = false) {
  if (!io.X || !io.U || !io.x_term || !io.lamb || !io.cost || extra_null)
    return fail(I2LQR_ERR_INVALID, "null buffer");
  if ((io.K == nullptr) != (io.k == nullptr))
    return fail(I2LQR_ERR_INVALID, "K and k must both be given or both be NULL");
  return I2LQR_OK;
}

// ---- arg-min kernels (flat, first index wins ties) -------------------------------------------
// FINAL: a single workgroup scans the whole vector and writes the result itself (small batches:
// one launch instead of two)
// The 256-thread reduction of the kernels below: every thread brings the best (value, index) of its
// own scan (index -1: none), all of them return the workgroup's (index -1: empty).
template <class T> __device__ MinPair<T> block_argmin(T bv, int64_t bi) {
  __shared__ T sv[256];
  __shared__ int64_t si[256];
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const T ov = sv[threadIdx.x + s];
      const int64_t oi = si[threadIdx.x + s];
      if (oi >= 0 && better(ov, oi, sv[threadIdx.x], si[threadIdx.x])) {
        sv[threadIdx.x] = ov;
        si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  return MinPair<T>{sv[0], si[0]};
}

template <class T, bool FINAL = false>
__global__ __launch_bounds__(256) void k_argmin_partial(int64_t B, const T* cost, MinPair<T>* part,
                                                        int64_t* best_idx = nullptr,
                                                        T* best_cost = nullptr) {
  T bv = T(0);
  int64_t bi = -1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < B; i += (int64_t)gridDim.x * 256) {
    const T v = cost[i];
    if (better(v, i, bv, bi)) { bv = v; bi = i; }
  }
  const MinPair<T> r = block_argmin(bv, bi);
  if (threadIdx.x == 0) {
    if constexpr (FINAL) {
      *best_idx = r.i;
      *best_cost = r.i >= 0 ? r.v : (T)INFINITY;
    } else {
      part[blockIdx.x].v = r.v;
      part[blockIdx.x].i = r.i;
    }
  }
}

template <class T>
__global__ __launch_bounds__(256) void k_argmin_final(int nparts, const MinPair<T>* part,
                                                      int64_t* best_idx, T* best_cost) {
  T bv = T(0);
  int64_t bi = -1;
  for (int p = threadIdx.x; p < nparts; p += 256) {
    const T v = part[p].v;
    const int64_t i = part[p].i;
    if (i >= 0 && better(v, i, bv, bi)) { bv = v; bi = i; }
  }
  const MinPair<T> r = block_argmin(bv, bi);
  if (threadIdx.x == 0) {
    *best_idx = r.i;
    *best_cost = r.i >= 0 ? r.v : (T)INFINITY;
  }
}

// ---- sharded round (i2lqr_sharded_round_flat) --------------------------------------------------
// What a rank contributes to the exchange, ONE launch: workgroup 0 packs the trajectory of the
// shard's pick (k_pack_problem's gather; zeros for a rank without candidates), and — ragged split
// only (padded non-null) — all workgroups copy the B costs into the `width` slots every rank
// gathers and fill the rest with +inf, which never wins the pick.
template <class T>
__global__ __launch_bounds__(256) void k_round_prepare(int64_t B, int n, int m, int N, int layout,
                                                       const T* X, const T* U, const int64_t* idx,
                                                       T* pack, int64_t width, const T* cost_it,
                                                       T* padded) {
  if (padded)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < width; i += (int64_t)gridDim.x * 256)
      padded[i] = i < B ? cost_it[i] : (T)INFINITY;
  if (blockIdx.x != 0) return;
  const int nu = m * N, nx = n * (N + 1);
  if (B <= 0) {
    for (int e = threadIdx.x; e < nu + nx; e += 256) pack[e] = T(0);
    return;
  }
  int64_t b = idx[0];
  if (b < 0) b = 0;
  if (b >= B) b = B - 1;
  auto fetch = [&](const T* A, int comps, int T_, int c, int t) -> T {
    if (layout == 0) return A[(b * comps + c) * T_ + t];
    if (layout == 1) return A[((int64_t)t * comps + c) * B + b];
    return A[(((b >> 6) * T_ + t) * comps + c) * 64 + (b & 63)];
  };
  for (int e = threadIdx.x; e < nu; e += 256) pack[e] = fetch(U, m, N, e / N, e % N);
  for (int e = threadIdx.x; e < nx; e += 256)
    pack[nu + e] = fetch(X, n, N + 1, e / (N + 1), e % (N + 1));
}

// The pick over the gathered costs and the winner's hand-off in ONE workgroup: k_argmin_partial<T,
// true> (same total order: the flat arg-min with first-index tie-break, NaN never wins) followed by
// k_round_winner's translation and copy.
template <class T>
__global__ __launch_bounds__(256) void k_round_pick(int world, int64_t width, int64_t total,
                                                    int64_t pack_count, const T* cost_all,
                                                    const T* pack_all, T* best_cost, T* winner,
                                                    int64_t* best_global) {
  const int64_t G = (int64_t)world * width;
  T bv = T(0);
  int64_t bi = -1;
  for (int64_t i = threadIdx.x; i < G; i += 256) {
    const T v = cost_all[i];
    if (better(v, i, bv, bi)) { bv = v; bi = i; }
  }
  const MinPair<T> r = block_argmin(bv, bi);
  const int64_t p = r.i;
  const int64_t q = p < 0 ? 0 : p;
  const int64_t owner = q / width, loc = q - owner * width;
  const int64_t base = total / world, rem = total - base * world;
  const int64_t lo = owner * base + (owner < rem ? owner : rem);
  if (threadIdx.x == 0) {
    *best_cost = p >= 0 ? r.v : (T)INFINITY;
    best_global[0] = p < 0 ? -1 : lo + loc;
    best_global[1] = owner;
  }
  for (int64_t e = threadIdx.x; e < pack_count; e += 256)
    winner[e] = pack_all[owner * pack_count + e];
}

constexpr int kArgminBlocks = 256;
constexpr int64_t kArgminSingle = 16384;  // up to here a single workgroup scans the vector

}  // namespace

// ---------------------------------------------------------------------------------------------
extern "C" {

int i2lqr_version(void) { return I2LQR_ABI_VERSION; }

const char* i2lqr_last_error(void) { return g_err; }

int i2lqr_config_default(i2lqr_config* cfg, int system_id, int num_horizon) {
  if (!cfg) return fail(I2LQR_ERR_INVALID, "null cfg");
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->struct_size = (int32_t)sizeof(*cfg);
  cfg->N = num_horizon;
  cfg->dtype = I2LQR_F64;
  cfg->layout = I2LQR_LAYOUT_PROBLEM_MAJOR;
  cfg->system_id = system_id;
  cfg->max_iter = 150;
  cfg->dt = 1.0;
  cfg->eps = 1e-2;
  cfg->lamb_factor = 10.0;
  cfg->max_lamb = 1000.0;
  cfg->ctrl_q1 = cfg->ctrl_q2 = 1.0;
  cfg->obs_q1 = cfg->obs_q2 = 2.74;
  cfg->safety_margin = 0.0;
  auto diag = [&](double* M, int i, double v) { M[i * I2LQR_MAX_N + i] = v; };
  switch (system_id) {
    case I2LQR_SYS_BICYCLE4: {
      cfg->n = 4;
      cfg->m = 2;
      cfg->u_max[0] = 2.0;
      cfg->u_max[1] = 1.57; /* round(pi/2, 2) */
      const double qt[4] = {2.0, 2.0, 40.0, 0.04};
      for (int i = 0; i < 4; i++) diag(cfg->Qt, i, qt[i]);
      break;
    }
    case I2LQR_SYS_BICYCLE6: {
      cfg->n = 6;
      cfg->m = 2;
      cfg->u_max[0] = 1.0;
      cfg->u_max[1] = 0.5;
      const double qt[6] = {2.0, 2.0, 40.0, 0.04, 2.0, 2.0};
      for (int i = 0; i < 6; i++) diag(cfg->Qt, i, qt[i]);
      break;
    }
    case I2LQR_SYS_QUAD12: {
      cfg->n = 12;
      cfg->m = 4;
      for (int a = 0; a < 4; a++) cfg->u_max[a] = 2.0;
      const double qt[4] = {20.0, 10.0, 2.0, 1.0};
      for (int i = 0; i < 12; i++) diag(cfg->Qt, i, qt[i / 3]);
      const double sp[8] = {1.0, 9.81, 0.2, 0.01, 0.01, 0.02, 0.05, 0.0};
      for (int q = 0; q < 8; q++) cfg->sys_par[q] = sp[q];
      break;
    }
    default:
      return fail(I2LQR_ERR_INVALID, "unknown system_id %d", system_id);
  }
  return I2LQR_OK;
}

int i2lqr_create(const i2lqr_config* cfg, i2lqr_handle** out) {
  if (!cfg || !out) return fail(I2LQR_ERR_INVALID, "null argument");
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(i2lqr_config))
    return fail(I2LQR_ERR_INVALID, "config struct_size %d, library expects %zu", cfg->struct_size,
                sizeof(i2lqr_config));
  int n = 0, m = 0;
  switch (cfg->system_id) {
    case I2LQR_SYS_BICYCLE4: n = 4; m = 2; break;
    case I2LQR_SYS_BICYCLE6: n = 6; m = 2; break;
    case I2LQR_SYS_QUAD12: n = 12; m = 4; break;
    default: return fail(I2LQR_ERR_INVALID, "unknown system_id %d", cfg->system_id);
  }
  if (cfg->n != n || cfg->m != m)
    return fail(I2LQR_ERR_INVALID, "system %d has n=%d m=%d, config says n=%d m=%d", cfg->system_id,
                n, m, cfg->n, cfg->m);
  if (cfg->N < 1 || cfg->N > I2LQR_MAX_HORIZON)
    return fail(I2LQR_ERR_INVALID, "horizon %d outside [1, %d]", cfg->N, I2LQR_MAX_HORIZON);
  if (cfg->dtype != I2LQR_F64 && cfg->dtype != I2LQR_F32)
    return fail(I2LQR_ERR_INVALID, "unknown dtype %d", cfg->dtype);
  if (cfg->layout != I2LQR_LAYOUT_PROBLEM_MAJOR && cfg->layout != I2LQR_LAYOUT_BATCH_MINOR &&
      cfg->layout != I2LQR_LAYOUT_BATCH_TILED)
    return fail(I2LQR_ERR_INVALID, "unknown layout %d", cfg->layout);
  if (!(cfg->dt > 0) || !(cfg->lamb_factor > 1) || cfg->max_iter < 0)
    return fail(I2LQR_ERR_INVALID, "need dt > 0, lamb_factor > 1, max_iter >= 0");
  for (int a = 0; a < m; a++)
    if (!(cfg->u_max[a] > 0)) return fail(I2LQR_ERR_INVALID, "u_max[%d] must be > 0", a);
  if (cfg->layout != I2LQR_LAYOUT_PROBLEM_MAJOR)
    if (const char* what = lane_asymmetry(*cfg))
      return fail(I2LQR_ERR_UNSUPPORTED, "the batch-minor / batch-tiled layouts need %s (use the "
                  "problem-major layout otherwise)", what);
  int ndev = 0;
#ifdef I2LQR_DRY_RUN
  const bool dry_run = dry::on();  // (sanitizer build + I2LQR_DRY_RUN=1: launches are recorded, not run)
#else
  constexpr bool dry_run = false;
#endif
  if (!dry_run && (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0))
    return fail(I2LQR_ERR_NODEVICE, "no HIP device visible (this library has no CPU path)");
  i2lqr_handle* h = new (std::nothrow) i2lqr_handle;
  if (!h) return fail(I2LQR_ERR_LAUNCH, "out of host memory");
  h->cfg = *cfg;
  h->geo = device_geometry();  // of the current device: CU count, LDS per CU / per workgroup
  h->fit = column_fit_config(h->cfg);  // (Layout<Sys>: Launch::prepare below)
  column_fit_group(h->cfg, h->fit);
  column_fit_quad(h->cfg, h->fit);
  if (h->geo.wave != 64) {
    const int w = h->geo.wave;
    delete h;
    return fail(I2LQR_ERR_UNSUPPORTED, "the kernels are built for 64-lane wavefronts (gfx950), this "
                "device reports %d", w);
  }
  constexpr size_t kTicketBytes = i2lqr_handle::kTickets * sizeof(unsigned);
  if (dry_run) {
#ifdef I2LQR_DRY_RUN
    static unsigned fake_tickets[i2lqr_handle::kTickets];  // an address to declare, never written by a kernel
    h->device = 0;
    h->ticket = fake_tickets;
    dry::allow(fake_tickets, sizeof(fake_tickets));
#endif
  } else if (hipGetDevice(&h->device) != hipSuccess ||
      hipMalloc((void**)&h->ticket, kTicketBytes) != hipSuccess ||
      hipMemset(h->ticket, 0, kTicketBytes) != hipSuccess) {
    if (h->ticket) (void)hipFree(h->ticket);
    delete h;
    return fail(I2LQR_ERR_LAUNCH, "could not set up the handle's device state: %s",
                hipGetErrorString(hipGetLastError()));
  }
  const int rc = dispatch(h, [&](auto L) { return L.prepare(h); });
  if (rc != I2LQR_OK) {
    (void)hipFree(h->ticket);
    delete h;
    return rc;
  }
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    live_handles().insert(h);
  }
  *out = h;
  g_err[0] = 0;
  return I2LQR_OK;
}

int64_t i2lqr_dry_run(int32_t op, void* p, int64_t n) {
#ifdef I2LQR_DRY_RUN
  switch (op) {
    case 0: return dry::on() ? 1 : 0;
    case 1: if (!dry::on()) break; dry::allow(p, (size_t)n); return 0;
    case 2: if (!dry::on()) break; dry::reset(); return 0;
    case 3: if (!dry::on()) break; return dry::report((char*)p, n);
    default: return fail(I2LQR_ERR_INVALID, "i2lqr_dry_run: unknown operation %d", op);
  }
  return fail(I2LQR_ERR_UNSUPPORTED, "dry-run launches need I2LQR_DRY_RUN=1 in the environment");
#else
  (void)op; (void)p; (void)n;
  return fail(I2LQR_ERR_UNSUPPORTED, "dry-run launches exist in the sanitizer build only (make -C "
              "ilqr_iterative_tasks_amd/csrc asan -> libi2lqr_hip_asan.so, I2LQR_DRY_RUN=1)");
#endif
}

int i2lqr_device_geometry(int32_t* out, int32_t count) {
  if (!out || count < 1) return fail(I2LQR_ERR_INVALID, "null / empty output");
  const DeviceGeometry& g = device_geometry();
  const int32_t v[8] = {g.cus, g.simds_per_cu, (int32_t)g.lds_per_cu, (int32_t)g.max_dyn_lds,
                        (int32_t)g.default_dyn_lds, g.wave, g.faked, g.queried};
  for (int i = 0; i < count && i < 8; i++) out[i] = v[i];
  return I2LQR_OK;
}

int i2lqr_destroy(i2lqr_handle* h) {
  if (!h) return I2LQR_OK;
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    if (live_handles().erase(h) == 0)
      return fail(I2LQR_ERR_INVALID, "i2lqr_destroy: %p is not a live handle (destroyed twice?)",
                  (void*)h);
  }
  if (h->ticket) (void)hipFree(h->ticket);
  if (h->ev_ready) (void)hipEventDestroy(h->ev_ready);
  if (h->ev_side_done) (void)hipEventDestroy(h->ev_side_done);
  delete h;
  return I2LQR_OK;
}

int64_t i2lqr_workspace_bytes(const i2lqr_handle* h, int64_t B) {
  if (!h || B < 0) return 0;
  if (h->cfg.layout == I2LQR_LAYOUT_PROBLEM_MAJOR)
    return column_workspace_bytes(h->geo, h->fit, h->col, B);
  const bool tiled = h->cfg.layout == I2LQR_LAYOUT_BATCH_TILED;
  return visit_plant(h->cfg, [&](auto t, auto sys) {
    using T = decltype(t);
    using Sys = decltype(sys);
    using L = LaneLaunch<T, Sys, false>;
    return tiled ? LaneLaunch<T, Sys, true>::ws_bytes(h, B) : L::ws_bytes(h, B);
  });
}

int i2lqr_recommended_layout(const i2lqr_config* cfg, int64_t B, int32_t early_exit) {
  if (!cfg) return fail(I2LQR_ERR_INVALID, "null config");
  if (cfg->struct_size != (int32_t)sizeof(i2lqr_config))
    return fail(I2LQR_ERR_INVALID, "config struct_size %d, library expects %zu", cfg->struct_size,
                sizeof(i2lqr_config));
  if (B < 0) return fail(I2LQR_ERR_INVALID, "negative batch %lld", (long long)B);
  if (cfg->system_id != I2LQR_SYS_BICYCLE4 && cfg->system_id != I2LQR_SYS_BICYCLE6 &&
      cfg->system_id != I2LQR_SYS_QUAD12)
    return fail(I2LQR_ERR_INVALID, "unknown system_id %d", cfg->system_id);
  return recommended_layout(device_geometry(), *cfg, has_stage_weights(*cfg), B, early_exit != 0);
}

int i2lqr_set_compaction(i2lqr_handle* h, int64_t min_batch) {
  if (!h) return fail(I2LQR_ERR_INVALID, "null handle");
  if (h->cfg.layout == I2LQR_LAYOUT_PROBLEM_MAJOR && min_batch > 0)
    return fail(I2LQR_ERR_UNSUPPORTED, "compaction applies to the batch-minor / batch-tiled layouts");
  h->lane.compact_min_batch = min_batch < 0 ? -1 : min_batch;
  return I2LQR_OK;
}

// What the opt-in forms refuse, and in which words, is i2lqr_lane_opt_in.hpp's: the forms of the
// one-problem-per-wavefront kernel on a handle of another layout (refuse_layout), and whatever
// concerns the lane forms (lane_refusal).  Here an answer becomes the call's return value.
static bool problem_major(const i2lqr_handle* h) { return h->cfg.layout == I2LQR_LAYOUT_PROBLEM_MAJOR; }
static int refused(const LaneRefusal& r) { return r.code ? fail(r.code, "%s", r.text) : I2LQR_OK; }
static int lane_ask(const i2lqr_handle* h, LaneAsk what, int v) {
  return refused(lane_refusal(what, v, problem_major(h), h->cfg.system_id == I2LQR_SYS_QUAD12,
                              h->model, h->lane_opt));
}

int i2lqr_set_option(i2lqr_handle* h, const char* name, int64_t value) {
  if (!h || !name) return fail(I2LQR_ERR_INVALID, "null handle or option name");
  if (value < -1 || value > 0x7fffffff) return fail(I2LQR_ERR_INVALID, "option value out of range");
  const int v = (int)value;
  LaneTune& lane = h->lane;
  ColumnTune& col = h->col;
  if (!strcmp(name, "defer_states")) lane.opt_defer = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "reroll_nominal")) lane.opt_reroll = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "lds_gain_steps")) lane.opt_lds_steps = v;
  else if (!strcmp(name, "merge_inputs")) lane.opt_merge = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "checkpoint_states")) lane.opt_ckpt = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "stagger")) lane.opt_stagger = v;
  else if (!strcmp(name, "per_step_jacobians")) col.opt_fstep = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "wave_tail")) lane.wave_tail = v < 0 ? -1 : (v > 65536 ? 65536 : v);
  else if (!strcmp(name, "first_chunk")) lane.opt_first_chunk = v < 1 ? -1 : (v > 1024 ? 1024 : v);
  else if (!strcmp(name, "helper_wavefront")) lane.opt_pair = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "state_buffers")) lane.opt_two_x = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "chunk_step")) lane.opt_chunk_step = v < 1 ? -1 : (v > 1024 ? 1024 : v);
  else if (!strcmp(name, "fused_compaction")) lane.opt_fuse = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "lane_model_chunks")) lane.opt_model_chunks = v == 1 ? 1 : -1;
  else if (!strcmp(name, "final_round")) lane.opt_final_round = v < 0 ? -1 : (v > 20 ? 20 : v);
  else if (!strcmp(name, "speculate")) col.opt_spec = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "group_workspace")) col.opt_group_ws = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "group_overlap")) col.opt_group_overlap = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "group_fixed_horizon")) col.opt_group_fixed = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "group_chains")) col.opt_group_chains = v < 0 ? -1 : (v != 0);
  else if (!strcmp(name, "debug_self_test")) {
    // Debug build only: provoke one index violation on purpose (a Slice of 8 words indexed at 8)
    // and return what the next call would: I2LQR_ERR_LAUNCH with the decoded record.
#ifdef I2LQR_DEBUG
    unsigned long long* w = i2lqr::debug_trap_word();
    double* buf = nullptr;
    HIP_TRY(hipMalloc((void**)&buf, 8 * sizeof(double)));
    hipLaunchKernelGGL(k_debug_self_test, dim3(1), dim3(64), 0, (hipStream_t)0, buf, w);
    const int rc = debug_check(I2LQR_OK, nullptr);
    (void)hipFree(buf);
    return rc;
#else
    return fail(I2LQR_ERR_UNSUPPORTED, "\"debug_self_test\" exists in the index-checked debug build "
                "only (make -C ilqr_iterative_tasks_amd/csrc debug)");
#endif
  }
  else if (!strcmp(name, "line_search")) {
    if (v != -1 && v != 0 && v != 1 && v != 2 && v != 4 && v != 8)
      return fail(I2LQR_ERR_INVALID, "\"line_search\" is 2, 4 or 8 step sizes, or -1 / 0 / 1 (off)");
    if (v > 1 && !problem_major(h)) return refused(refuse_layout(wave_phrase(WAVE_LS)));
    h->model.ls = v > 1 ? v : 0;
  }
  else if (!strcmp(name, "obstacles")) {
    if (v > I2LQR_MAX_OBSTACLES)
      return fail(I2LQR_ERR_INVALID, "\"obstacles\" is 2 ... %d records per problem, or -1 / 0 / 1 "
                  "(off: one record)", I2LQR_MAX_OBSTACLES);
    if (int rc = lane_ask(h, LANE_ASK_OBSTACLES, v)) return rc;
    h->model.obs = v > 1 ? v : 0;
  }
  else if (!strcmp(name, "lane_models")) {
    if (int rc = lane_ask(h, LANE_ASK_MODELS, v)) return rc;
    h->lane_opt.models = v == 1;
  }
  else if (!strcmp(name, "lane_rows_models")) {
    if (int rc = lane_ask(h, LANE_ASK_ROWS_MODELS, v)) return rc;
    h->lane_opt.rows_models = v == 1;
  }
  else if (!strcmp(name, "barrier_cost")) {
    if (v != -1 && v != 0 && v != 1)
      return fail(I2LQR_ERR_INVALID, "\"barrier_cost\" is 1 (on), or -1 / 0 (off)");
    if (int rc = lane_ask(h, WAVE_ASK_BARRIER_COST, v)) return rc;
    h->model.barrier_cost = v == 1;
  }
  else if (!strcmp(name, "lane_barrier_cost")) {
    if (int rc = lane_ask(h, LANE_ASK_BARRIER_COST, v)) return rc;
    h->lane_opt.barrier_cost = v == 1;
  }
  else if (!strcmp(name, "lane_line_search")) {
    if (int rc = lane_ask(h, LANE_ASK_LINE_SEARCH, v)) return rc;
    h->lane_opt.line_search = v > 1 ? v : 0;
  }
  else if (!strcmp(name, "wave_chain")) {
    if (v != -1 && v != 0 && v != 1)
      return fail(I2LQR_ERR_INVALID, "\"wave_chain\" is 1 (on), or -1 / 0 (off)");
    if (v == 1 && !problem_major(h)) return refused(refuse_layout("\"wave_chain\""));
    col.opt_wave_chain = v == 1 ? 1 : 0;
  }
  else if (!strcmp(name, "group_lanes")) {
    if (v != -1 && v != 8 && v != 16 && v != 64)
      return fail(I2LQR_ERR_INVALID, "\"group_lanes\" is 8, 16, 64 or -1");
    col.opt_group = v;
  }
  else return fail(I2LQR_ERR_INVALID, "unknown option '%s'", name);
  return I2LQR_OK;
}

int i2lqr_set_state_box(i2lqr_handle* h, const double* lo, const double* hi, double q1, double q2) {
  if (!h) return fail(I2LQR_ERR_INVALID, "null handle");
  if ((lo == nullptr) != (hi == nullptr))
    return fail(I2LQR_ERR_INVALID, "state box: lo and hi must both be given or both be NULL");
  if (!(q1 > 0.0) || !(q2 > 0.0) || std::isinf(q1) || std::isinf(q2))
    return fail(I2LQR_ERR_INVALID, "state box: q1 and q2 must be positive and finite");
  i2lqr::StateBox b;
  b.q1 = q1;
  b.q2 = q2;
  for (int i = 0; lo && i < h->cfg.n; i++) {
    if (std::isnan(lo[i]) || std::isnan(hi[i]))
      return fail(I2LQR_ERR_INVALID, "state box: bound %d is NaN", i);
    if (lo[i] >= hi[i])
      return fail(I2LQR_ERR_INVALID, "state box: lo[%d] = %g is not below hi[%d] = %g", i, lo[i], i,
                  hi[i]);
    // an unbounded side keeps its 0: the kernel does no arithmetic on infinities (the masks count)
    if (!std::isinf(lo[i])) {
      b.lo[i] = lo[i];
      b.m_lo |= 1u << i;
    }
    if (!std::isinf(hi[i])) {
      b.hi[i] = hi[i];
      b.m_hi |= 1u << i;
    }
  }
  if (int rc = lane_ask(h, LANE_ASK_BOX, b.on() ? 1 : 0)) return rc;
  h->model.box = b;
  return I2LQR_OK;
}

static const char* kernel_name(const i2lqr_handle* h, int64_t B, bool early_exit) {
  if (!h) return "";
  if (h->cfg.layout != I2LQR_LAYOUT_PROBLEM_MAJOR) {
    // ("lane_rows_models": k_lane_iterate_rows_model with records or a box, from the same record)
    if (h->cfg.system_id == I2LQR_SYS_QUAD12)
      return lane_rows_kernel_name(h->lane_opt.rows_models ? lane_model(h->model, h->lane_opt).form()
                                                           : LANE_PLAIN);
    // a form of "lane_models": what LaneLaunch::iterate launches from the same record
    // ... "lane_model_chunks": with ", chunked" where its plan runs the solve as chunks
    if (const LaneForm f = lane_model(h->model, h->lane_opt).form(); f != LANE_PLAIN) {
      const auto chunks = [&](auto L) { return L.names_model_chunks(h, B, early_exit ? 1 : 0); };
      return dispatch(h, chunks) == 1 ? lane_chunked_kernel_name(f) : lane_kernel_name(f);
    }
    // the helper-wavefront form (both precisions, with or without stage weights): decided by the
    // launcher's own rules (LaneLaunch::names_pair)
    const auto pair = [&](auto L) { return L.names_pair(h, B, early_exit ? 1 : 0); };
    return dispatch(h, pair) == 1 ? "k_lane_iterate_pair" : "k_lane_iterate";
  }
  // (a model's form of the wavefront kernel: wave_kernel_name() of it, through column_kernel_name)
  return column_kernel_name(column_kernel(h, B, early_exit).kernel, h->model.form());
}

const char* i2lqr_iterate_kernel(const i2lqr_handle* h, int64_t B) { return kernel_name(h, B, false); }
const char* i2lqr_solve_kernel(const i2lqr_handle* h, int64_t B) { return kernel_name(h, B, true); }

int i2lqr_set_workspace(i2lqr_handle* h, void* workspace, int64_t bytes) {
  if (!h) return fail(I2LQR_ERR_INVALID, "null handle");
  if (bytes < 0 || (bytes > 0 && !workspace) || ((uintptr_t)workspace & 15))
    return fail(I2LQR_ERR_INVALID, "workspace must be a 16-byte aligned device pointer");
  h->ws = workspace;
  h->ws_bytes = bytes;
  return I2LQR_OK;
}

int i2lqr_rollout(i2lqr_handle* h, int64_t B, void* X, void* U, const void* x_term, void* cost,
                  void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if (B == 0) return I2LQR_OK;
  if (!X || !U || !x_term || !cost) return fail(I2LQR_ERR_INVALID, "null buffer");
  const int rc = dispatch(h, [&](auto L) {
    return L.rollout(h, B, X, U, x_term, cost, (hipStream_t)stream);
  });
  return debug_check(rc, stream);
}

int i2lqr_backward(i2lqr_handle* h, int64_t B, const void* X, const void* U, const void* x_term,
                   const void* lamb, const void* obs, void* K, void* k, void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if (B == 0) return I2LQR_OK;
  if (!X || !U || !x_term || !lamb || !K || !k) return fail(I2LQR_ERR_INVALID, "null buffer");
  // (k_backward has no forward pass: the line search does not concern it)
  if (const WaveForm f = h->model.without_line_search().form(); f != WAVE_PLAIN)
    return fail(I2LQR_ERR_UNSUPPORTED, "i2lqr_backward %s, or use i2lqr_iterate", wave_lack_phrase(f));
  const int rc = dispatch(h, [&](auto L) {
    return L.backward(h, B, X, U, x_term, lamb, obs, K, k, (hipStream_t)stream);
  });
  return debug_check(rc, stream);
}

int i2lqr_forward(i2lqr_handle* h, int64_t B, const void* X, const void* U, const void* x_term,
                  const void* K, const void* k, void* X_new, void* U_new, void* cost_new,
                  void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if (B == 0) return I2LQR_OK;
  if (!X || !U || !x_term || !K || !k || !X_new || !U_new || !cost_new)
    return fail(I2LQR_ERR_INVALID, "null buffer");
  const int rc = dispatch(h, [&](auto L) {
    return L.forward(h, B, X, U, x_term, K, k, X_new, U_new, cost_new, (hipStream_t)stream);
  });
  return debug_check(rc, stream);
}

int i2lqr_iterate(i2lqr_handle* h, int64_t B, int32_t n_iters, void* X, void* U,
                  const void* x_term, void* lamb, const void* obs, void* cost, void* K, void* k,
                  int32_t* iters, int32_t* status, void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if (n_iters < 0) return fail(I2LQR_ERR_INVALID, "negative n_iters");
  if (B == 0) return I2LQR_OK;
  const SolveIO io{B, n_iters, 0, X, U, x_term, lamb, obs, cost, K, k, iters, status};
  if (int rc = check_io(io)) return rc;
  return debug_check(dispatch_iterate(h, io, stream), stream);
}

int i2lqr_solve(i2lqr_handle* h, int64_t B, void* X, void* U, const void* x_term, void* lamb,
                const void* obs, void* cost, void* K, void* k, int32_t* iters, int32_t* status,
                void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if (B == 0) return I2LQR_OK;
  const SolveIO io{B, h->cfg.max_iter, 1, X, U, x_term, lamb, obs, cost, K, k, iters, status};
  if (int rc = check_io(io)) return rc;
  return debug_check(dispatch_iterate(h, io, stream), stream);
}

int i2lqr_solve_chained(i2lqr_handle* h, int64_t chains, int32_t chain_len, void* X, void* U,
                        const void* x_term, void* lamb, const void* obs, void* cost, void* K, void* k,
                        int32_t* iters, int32_t* status, void* stream) {
  if (int rc = check_common(h, chains)) return rc;
  if (chain_len < 1) return fail(I2LQR_ERR_INVALID, "chain_len must be >= 1");
  if (chains * (int64_t)chain_len > (int64_t)0x7fffffff)
    return fail(I2LQR_ERR_INVALID, "%lld chains of %d problems", (long long)chains, chain_len);
  if (chains == 0) return I2LQR_OK;
  const SolveIO io{chains, h->cfg.max_iter, 1, X, U, x_term, lamb, obs, cost, K, k, iters, status};
  if (int rc = check_io(io)) return rc;
  // (k_chain_box carries the models but the barrier cost: nothing else to refuse with "wave_chain" 1)
  if (h->model.barrier_cost) return fail(I2LQR_ERR_UNSUPPORTED, "%s", kChainNoBarrierCost);
  if (const WaveForm f = h->model.form(); f != WAVE_PLAIN && h->col.opt_wave_chain != 1)
    return fail(I2LQR_ERR_UNSUPPORTED, "chains run on the sixteen-lane speculative kernel, which %s, "
                "or solve the chain steps one after the other", wave_lack_phrase(f));
  const int rc = dispatch(h, [&](auto L) {
    return L.solve_chained(h, io, chain_len, (hipStream_t)stream);
  });
  return debug_check(rc, stream);
}

int i2lqr_relax_cost(i2lqr_handle* h, int64_t B, const void* X, const void* x_term,
                     const int32_t* qfun, int32_t outer_iter, int32_t max_relax_iter,
                     void* cost_it, void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if (B == 0) return I2LQR_OK;
  if (!X || !x_term || !qfun || !cost_it) return fail(I2LQR_ERR_INVALID, "null buffer");
  if (outer_iter < 0 || max_relax_iter < 1)
    return fail(I2LQR_ERR_INVALID, "need outer_iter >= 0 and max_relax_iter >= 1");
  const unsigned grid = (unsigned)((B + 255) / 256);
  const int bm = h->cfg.layout;  // 0 problem-major, 1 batch-minor, 2 batch-tiled
  hipStream_t s = (hipStream_t)stream;
  visit_precision(h->cfg, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_relax_cost<T>), dim3(grid), dim3(256), 0, s, B, h->cfg.n, h->cfg.N, bm,
                       (const T*)X, (const T*)x_term, qfun, outer_iter, max_relax_iter, (T*)cost_it);
  });
  HIP_TRY(hipGetLastError());
  return I2LQR_OK;
}

int64_t i2lqr_argmin_workspace_bytes(int64_t B) {
  // one (value, index) pair per workgroup: 256 for i2lqr_argmin, one per eight problems for the
  // pick that i2lqr_iterate_pick folds into the eight-lane kernels
  const int64_t rows = B > 0 ? (B + 3) / 4 : 0;  // ... one per four on the sixteen-lane form
  return (rows > kArgminBlocks ? rows : (int64_t)kArgminBlocks) * 16;
}

int i2lqr_argmin(i2lqr_handle* h, int64_t B, const void* cost_it, int64_t* best_idx,
                 void* best_cost, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if ((B > 0 && !cost_it) || !best_idx || !best_cost || !workspace)
    return fail(I2LQR_ERR_INVALID, "null buffer");
  if (workspace_bytes < i2lqr_argmin_workspace_bytes(B))
    return fail(I2LQR_ERR_INVALID, "arg-min workspace of %lld bytes, %lld problems need "
                "i2lqr_argmin_workspace_bytes(B) = %lld", (long long)workspace_bytes, (long long)B,
                (long long)i2lqr_argmin_workspace_bytes(B));
  hipStream_t s = (hipStream_t)stream;
  int64_t want = (B + 255) / 256;
  const int blocks = (int)(want < 1 ? 1 : (want > kArgminBlocks ? kArgminBlocks : want));
  visit_precision(h->cfg, [&](auto t) {
    using T = decltype(t);
    auto* part = (MinPair<T>*)workspace;
    if (B <= kArgminSingle) {  // one workgroup, one launch
      hipLaunchKernelGGL((k_argmin_partial<T, true>), dim3(1), dim3(256), 0, s, B, (const T*)cost_it,
                         (MinPair<T>*)nullptr, best_idx, (T*)best_cost);
    } else {
      hipLaunchKernelGGL((k_argmin_partial<T>), dim3(blocks), dim3(256), 0, s, B, (const T*)cost_it,
                         part);
      hipLaunchKernelGGL((k_argmin_final<T>), dim3(1), dim3(256), 0, s, blocks, part, best_idx,
                         (T*)best_cost);
    }
  });
  HIP_TRY(hipGetLastError());
  return I2LQR_OK;
}

int i2lqr_iterate_pick(i2lqr_handle* h, int64_t B, int32_t n_iters, void* X, void* U,
                       const void* x_term, void* lamb, const void* obs, void* cost, void* K, void* k,
                       int32_t* iters, int32_t* status, const int32_t* qfun, int32_t outer_iter,
                       int32_t max_relax_iter, void* cost_it, int64_t* best_idx, void* best_cost,
                       void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if (n_iters < 0) return fail(I2LQR_ERR_INVALID, "negative n_iters");
  if (outer_iter < 0 || max_relax_iter < 1)
    return fail(I2LQR_ERR_INVALID, "need outer_iter >= 0 and max_relax_iter >= 1");
  if (best_idx && (!best_cost || !workspace))
    return fail(I2LQR_ERR_INVALID, "best_idx needs best_cost and a workspace of "
                "i2lqr_argmin_workspace_bytes(B)");
  // the fused epilogue writes one (value, index) pair per workgroup of the iterate kernel: a
  // workspace sized for a smaller batch would be written out of bounds on the device
  if (best_idx && workspace_bytes < i2lqr_argmin_workspace_bytes(B))
    return fail(I2LQR_ERR_INVALID, "pick workspace of %lld bytes, %lld problems need "
                "i2lqr_argmin_workspace_bytes(B) = %lld", (long long)workspace_bytes, (long long)B,
                (long long)i2lqr_argmin_workspace_bytes(B));
  if (B == 0)  // nothing to solve; an empty pick is (-1, +inf) as in i2lqr_argmin
    return best_idx ? i2lqr_argmin(h, 0, nullptr, best_idx, best_cost, workspace, workspace_bytes,
                                   stream) : I2LQR_OK;
  const SolveIO io{B, n_iters, 0, X, U, x_term, lamb, obs, cost, K, k, iters, status};
  if (int rc = check_io(io, !qfun || !cost_it)) return rc;
  i2lqr_handle::Epilogue epi{qfun, outer_iter, max_relax_iter, cost_it, workspace, best_idx,
                             best_cost, false};
  t_epi = &epi;
  const int rc = dispatch_iterate(h, io, stream);
  t_epi = nullptr;
  if (rc != I2LQR_OK) return rc;
  if (!epi.fused) {  // kernel families without the epilogue: the same three steps as launches
    if (int r2 = i2lqr_relax_cost(h, B, X, x_term, qfun, outer_iter, max_relax_iter, cost_it, stream))
      return r2;
    if (best_idx)
      if (int r3 = i2lqr_argmin(h, B, cost_it, best_idx, best_cost, workspace, workspace_bytes,
                                stream)) return r3;
  }
  return debug_check(I2LQR_OK, stream);
}

int i2lqr_select_candidates(i2lqr_handle* h, int32_t L, int32_t Tmax, const void* ss,
                            const int32_t* T, const int32_t* qfun, const void* x_guess,
                            int32_t guess_stride, int32_t k, int32_t* idx, void* x_term,
                            int32_t* qf, void* stream) {
  if (!h) return fail(I2LQR_ERR_INVALID, "null handle");
  if (h->cfg.layout != I2LQR_LAYOUT_PROBLEM_MAJOR)
    return fail(I2LQR_ERR_UNSUPPORTED, "controller-round kernels need the problem-major layout");
  if (L < 0 || Tmax < 1 || Tmax > 1024 || k < 1 || k > Tmax || guess_stride < 1)
    return fail(I2LQR_ERR_INVALID, "need L >= 0, 1 <= k <= Tmax <= 1024, guess_stride >= 1");
  if (L == 0) return I2LQR_OK;
  if (!ss || !T || !qfun || !x_guess || !idx || !x_term || !qf)
    return fail(I2LQR_ERR_INVALID, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  visit_precision(h->cfg, [&](auto t) {
    using R = decltype(t);  // (T: the laps' column counts)
    hipLaunchKernelGGL((k_select_candidates<R>), dim3(L), dim3(128), 0, s, h->cfg.n, Tmax, k,
                       (const R*)ss, T, qfun, (const R*)x_guess, guess_stride, idx, (R*)x_term, qf);
  });
  HIP_TRY(hipGetLastError());
  return I2LQR_OK;
}

int i2lqr_init_candidates(i2lqr_handle* h, int64_t B, const void* x0, double lamb0, void* X,
                          void* U, void* lamb, void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if (h->cfg.layout != I2LQR_LAYOUT_PROBLEM_MAJOR)
    return fail(I2LQR_ERR_UNSUPPORTED, "controller-round kernels need the problem-major layout");
  if (B == 0) return I2LQR_OK;
  if (!x0 || !X || !U || !lamb) return fail(I2LQR_ERR_INVALID, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  const int n = h->cfg.n, m = h->cfg.m, N = h->cfg.N;
  visit_precision(h->cfg, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_init_candidates<T>), dim3((unsigned)B), dim3(64), 0, s, B, n, m, N,
                       (const T*)x0, (T)lamb0, (T*)X, (T*)U, (T*)lamb);
  });
  HIP_TRY(hipGetLastError());
  return I2LQR_OK;
}

int i2lqr_pick_best(i2lqr_handle* h, int32_t L, int32_t k, const void* cost_it, const void* X,
                    const void* U, int32_t* best, void* x_pred, void* u_pred, void* stream) {
  if (!h) return fail(I2LQR_ERR_INVALID, "null handle");
  if (L < 1 || k < 1) return fail(I2LQR_ERR_INVALID, "need L >= 1 and k >= 1");
  if (!cost_it || !best) return fail(I2LQR_ERR_INVALID, "null buffer");
  // X, U, x_pred, u_pred all NULL: the pick alone (a sharded round picks on the gathered costs;
  // the winner's trajectory is on the rank that solved it) — any layout
  const bool index_only = !X && !U && !x_pred && !u_pred;
  if (!index_only && (!X || !U || !x_pred || !u_pred))
    return fail(I2LQR_ERR_INVALID, "X, U, x_pred, u_pred must all be given or all be NULL");
  if (!index_only && h->cfg.layout != I2LQR_LAYOUT_PROBLEM_MAJOR)
    return fail(I2LQR_ERR_UNSUPPORTED, "controller-round kernels need the problem-major layout");
  hipStream_t s = (hipStream_t)stream;
  const int n = h->cfg.n, m = h->cfg.m, N = h->cfg.N;
  visit_precision(h->cfg, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_pick_best<T>), dim3(1), dim3(64), 0, s, L, k, n, m, N, (const T*)cost_it,
                       (const T*)X, (const T*)U, best, (T*)x_pred, (T*)u_pred);
  });
  HIP_TRY(hipGetLastError());
  return I2LQR_OK;
}

int i2lqr_comm_available(void) {
  const RcclApi& api = rccl_api();
  if (!api.ok) return fail(I2LQR_ERR_UNSUPPORTED, "librccl could not be loaded: %s", api.why);
  return I2LQR_OK;
}

int i2lqr_comm_unique_id(void* id) {
  if (!id) return fail(I2LQR_ERR_INVALID, "null id buffer");
  const RcclApi& api = rccl_api();
  if (!api.ok) return fail(I2LQR_ERR_UNSUPPORTED, "librccl could not be loaded: %s", api.why);
  static_assert(sizeof(ncclUniqueId) == I2LQR_COMM_ID_BYTES, "unique id size");
  ncclUniqueId uid;
  RCCL_TRY(api, api.GetUniqueId(&uid));
  std::memcpy(id, &uid, sizeof(uid));
  return I2LQR_OK;
}

int i2lqr_comm_create(const void* id, int32_t world, int32_t rank, void** comm) {
  if (!id || !comm) return fail(I2LQR_ERR_INVALID, "null argument");
  *comm = nullptr;
  if (world < 1 || rank < 0 || rank >= world)
    return fail(I2LQR_ERR_INVALID, "need 0 <= rank < world (got rank %d, world %d)", rank, world);
  const RcclApi& api = rccl_api();
  if (!api.ok) return fail(I2LQR_ERR_UNSUPPORTED, "librccl could not be loaded: %s", api.why);
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  ncclComm_t c = nullptr;
  RCCL_TRY(api, api.CommInitRank(&c, world, uid, rank));  // binds the calling thread's device
  *comm = (void*)c;
  return I2LQR_OK;
}

int i2lqr_comm_destroy(void* comm) {
  if (!comm) return I2LQR_OK;
  const RcclApi& api = rccl_api();
  if (!api.ok) return fail(I2LQR_ERR_UNSUPPORTED, "librccl could not be loaded");
  RCCL_TRY(api, api.CommDestroy((ncclComm_t)comm));
  return I2LQR_OK;
}

int i2lqr_comm_abort(void* comm) {
  if (!comm) return I2LQR_OK;
  const RcclApi& api = rccl_api();
  if (!api.ok) return fail(I2LQR_ERR_UNSUPPORTED, "librccl could not be loaded");
  RCCL_TRY(api, api.CommAbort((ncclComm_t)comm));
  return I2LQR_OK;
}

int i2lqr_comm_info(void* comm, int32_t* world, int32_t* rank) {
  if (!comm || !world || !rank) return fail(I2LQR_ERR_INVALID, "null argument");
  const RcclApi& api = rccl_api();
  if (!api.ok) return fail(I2LQR_ERR_UNSUPPORTED, "librccl could not be loaded");
  int w = 0, r = 0;
  RCCL_TRY(api, api.CommCount((ncclComm_t)comm, &w));
  RCCL_TRY(api, api.CommUserRank((ncclComm_t)comm, &r));
  *world = w;
  *rank = r;
  return I2LQR_OK;
}

int i2lqr_allgather_costs(i2lqr_handle* h, void* comm, const void* cost_local, void* cost_all,
                          int64_t n_local, void* stream) {
  if (int rc = check_common(h, n_local)) return rc;
  if (!comm) return fail(I2LQR_ERR_INVALID, "null communicator");
  if (n_local == 0) return I2LQR_OK;
  if (!cost_local || !cost_all) return fail(I2LQR_ERR_INVALID, "null buffer");
  const RcclApi& api = rccl_api();
  if (!api.ok) return fail(I2LQR_ERR_UNSUPPORTED, "librccl could not be loaded");
  const ncclDataType_t dt = h->cfg.dtype == I2LQR_F64 ? ncclDouble : ncclFloat;
  RCCL_TRY(api, api.AllGather(cost_local, cost_all, (size_t)n_local, dt, (ncclComm_t)comm,
                              (hipStream_t)stream));
  return I2LQR_OK;
}

int i2lqr_allgather_round(i2lqr_handle* h, void* comm, const void* cost_local, void* cost_all,
                          int64_t n_local, const void* pack_local, void* pack_all,
                          int64_t pack_count, void* stream) {
  if (int rc = check_common(h, n_local)) return rc;
  if (!comm) return fail(I2LQR_ERR_INVALID, "null communicator");
  if (pack_count < 0) return fail(I2LQR_ERR_INVALID, "negative pack_count");
  if ((n_local > 0 && (!cost_local || !cost_all)) || (pack_count > 0 && (!pack_local || !pack_all)))
    return fail(I2LQR_ERR_INVALID, "null buffer");
  if (n_local == 0 && pack_count == 0) return I2LQR_OK;
  const RcclApi& api = rccl_api();
  if (!api.ok) return fail(I2LQR_ERR_UNSUPPORTED, "librccl could not be loaded");
  const ncclDataType_t dt = h->cfg.dtype == I2LQR_F64 ? ncclDouble : ncclFloat;
  // both all-gathers as ONE grouped operation (one launch on the communicator's stream)
  const bool grouped = api.GroupStart && api.GroupEnd;
  if (grouped) RCCL_TRY(api, api.GroupStart());
  ncclResult_t r1 = ncclSuccess, r2 = ncclSuccess;
  if (n_local > 0)
    r1 = api.AllGather(cost_local, cost_all, (size_t)n_local, dt, (ncclComm_t)comm,
                       (hipStream_t)stream);
  if (r1 == ncclSuccess && pack_count > 0)
    r2 = api.AllGather(pack_local, pack_all, (size_t)pack_count, dt, (ncclComm_t)comm,
                       (hipStream_t)stream);
  if (grouped) {  // the group is closed whatever happened inside it
    const ncclResult_t r3 = api.GroupEnd();
    if (r1 == ncclSuccess && r2 == ncclSuccess) RCCL_TRY(api, r3);
  }
  RCCL_TRY(api, r1);
  RCCL_TRY(api, r2);
  return I2LQR_OK;
}

int i2lqr_pack_problem(i2lqr_handle* h, int64_t B, const void* X, const void* U, const int64_t* idx,
                       void* pack, void* stream) {
  if (int rc = check_common(h, B)) return rc;
  if (B < 1) return fail(I2LQR_ERR_INVALID, "need at least one problem");
  if (!X || !U || !idx || !pack) return fail(I2LQR_ERR_INVALID, "null buffer");
  if (h->cfg.layout == I2LQR_LAYOUT_BATCH_TILED && (B & 63))
    return fail(I2LQR_ERR_INVALID, "the batch-tiled layout needs a batch that is a multiple of 64");
  hipStream_t s = (hipStream_t)stream;
  const int n = h->cfg.n, m = h->cfg.m, N = h->cfg.N;
  visit_precision(h->cfg, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_pack_problem<T>), dim3(1), dim3(256), 0, s, B, n, m, N, (int)h->cfg.layout,
                       (const T*)X, (const T*)U, idx, (T*)pack);
  });
  HIP_TRY(hipGetLastError());
  return I2LQR_OK;
}

int i2lqr_round_winner(i2lqr_handle* h, int32_t world, int64_t width, int64_t total,
                       int64_t pack_count, const int64_t* best_padded, const void* pack_all,
                       void* winner, int64_t* best_global, void* stream) {
  if (!h) return fail(I2LQR_ERR_INVALID, "null handle");
  if (world < 1 || width < 1 || total < 0 || total > (int64_t)world * width || pack_count < 0)
    return fail(I2LQR_ERR_INVALID, "need world >= 1, width >= 1, 0 <= total <= world * width, "
                "pack_count >= 0");
  if (!best_padded || !best_global || (pack_count > 0 && (!pack_all || !winner)))
    return fail(I2LQR_ERR_INVALID, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  visit_precision(h->cfg, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_round_winner<T>), dim3(1), dim3(256), 0, s, world, width, total, pack_count,
                       best_padded, (const T*)pack_all, (T*)winner, best_global);
  });
  HIP_TRY(hipGetLastError());
  return I2LQR_OK;
}

int i2lqr_broadcast_winner(i2lqr_handle* h, void* comm, void* buf, int64_t count, int32_t root,
                           void* stream) {
  if (int rc = check_common(h, count)) return rc;
  if (!comm) return fail(I2LQR_ERR_INVALID, "null communicator");
  if (root < 0) return fail(I2LQR_ERR_INVALID, "negative root rank");
  if (count == 0) return I2LQR_OK;
  if (!buf) return fail(I2LQR_ERR_INVALID, "null buffer");
  const RcclApi& api = rccl_api();
  if (!api.ok) return fail(I2LQR_ERR_UNSUPPORTED, "librccl could not be loaded");
  const ncclDataType_t dt = h->cfg.dtype == I2LQR_F64 ? ncclDouble : ncclFloat;
  RCCL_TRY(api, api.Broadcast(buf, buf, (size_t)count, dt, root, (ncclComm_t)comm,
                              (hipStream_t)stream));
  return I2LQR_OK;
}

int i2lqr_round_pick(i2lqr_handle* h, int32_t world, int64_t width, int64_t total,
                     int64_t pack_count, const void* cost_all, const void* pack_all,
                     void* best_cost, void* winner, int64_t* best_global, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  if (!h) return fail(I2LQR_ERR_INVALID, "null handle");
  if (world < 1 || width < 1 || total < 0 || total > (int64_t)world * width || pack_count < 0)
    return fail(I2LQR_ERR_INVALID, "need world >= 1, width >= 1, 0 <= total <= world * width, "
                "pack_count >= 0");
  const int64_t G = (int64_t)world * width;
  if (G > (int64_t)0x7fffffff) return fail(I2LQR_ERR_INVALID, "%lld gathered costs", (long long)G);
  if (!cost_all || !best_cost || !best_global || (pack_count > 0 && (!pack_all || !winner)))
    return fail(I2LQR_ERR_INVALID, "null buffer");
  hipStream_t s = (hipStream_t)stream;
  if (G <= kArgminSingle) {
    visit_precision(h->cfg, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((k_round_pick<T>), dim3(1), dim3(256), 0, s, world, width, total, pack_count,
                         (const T*)cost_all, (const T*)pack_all, (T*)best_cost, (T*)winner,
                         best_global);
    });
    HIP_TRY(hipGetLastError());
    return I2LQR_OK;
  }
  // large gathers: the two-level arg-min, its index parked behind the partial minima
  const int64_t need = i2lqr_argmin_workspace_bytes(G) + 16;
  if (!workspace || workspace_bytes < need)
    return fail(I2LQR_ERR_INVALID, "round-pick workspace of %lld bytes, %lld gathered costs need "
                "i2lqr_argmin_workspace_bytes + 16 = %lld", (long long)workspace_bytes, (long long)G,
                (long long)need);
  int64_t* best_padded = (int64_t*)((char*)workspace + i2lqr_argmin_workspace_bytes(G));
  if (int rc = i2lqr_argmin(h, G, cost_all, best_padded, best_cost, workspace,
                            i2lqr_argmin_workspace_bytes(G), stream)) return rc;
  return i2lqr_round_winner(h, world, width, total, pack_count, best_padded, pack_all, winner,
                            best_global, stream);
}

int i2lqr_sharded_round_flat(i2lqr_handle* h, void* comm, const i2lqr_round* r, void* side_stream,
                             void* stream) {
  if (!h) return fail(I2LQR_ERR_INVALID, "null handle");
  if (!r) return fail(I2LQR_ERR_INVALID, "null round");
  if (r->struct_size != (int32_t)sizeof(i2lqr_round))
    return fail(I2LQR_ERR_INVALID, "round struct_size %d, library expects %zu", r->struct_size,
                sizeof(i2lqr_round));
  if (int rc = check_common(h, r->B)) return rc;
  if (r->world < 1 || r->rank < 0 || r->rank >= r->world)
    return fail(I2LQR_ERR_INVALID, "need 0 <= rank < world (got rank %d, world %d)", r->rank, r->world);
  if (r->total < 1)
    return fail(I2LQR_ERR_INVALID, "a round needs at least one candidate over all ranks (total %lld)",
                (long long)r->total);
  if (!comm && r->world != 1 && !r->loopback)
    return fail(I2LQR_ERR_INVALID, "a world of %d ranks needs a communicator", r->world);
  // the contiguous split every rank derives from (total, world): dist.shard_range
  const int64_t base = r->total / r->world, rem = r->total - base * r->world;
  const int64_t mine = base + (r->rank < rem ? 1 : 0);
  const int64_t width = base + (rem ? 1 : 0);
  if (r->B != mine)
    return fail(I2LQR_ERR_INVALID, "rank %d of %d owns %lld of %lld candidates, the round says %lld",
                r->rank, r->world, (long long)mine, (long long)r->total, (long long)r->B);
  if (width * r->world > (int64_t)0x7fffffff)
    return fail(I2LQR_ERR_INVALID, "%lld gathered costs", (long long)(width * r->world));
  const int n = h->cfg.n, m = h->cfg.m, N = h->cfg.N;
  const int64_t P = (int64_t)m * N + (int64_t)n * (N + 1);
  if (!r->pack_local || !r->cost_all || !r->pack_all || !r->best_cost || !r->winner ||
      !r->best_global || (r->B > 0 && (!r->cost_it || !r->local_best || !r->local_best_cost)))
    return fail(I2LQR_ERR_INVALID, "null buffer");
  if (r->B != width && !r->cost_padded)
    return fail(I2LQR_ERR_INVALID, "a ragged split (%lld of width %lld) needs cost_padded",
                (long long)r->B, (long long)width);
  if (width * r->world > kArgminSingle &&
      (!r->side_ws || r->side_ws_bytes < i2lqr_argmin_workspace_bytes(width * r->world) + 16))
    return fail(I2LQR_ERR_INVALID, "side workspace of %lld bytes, %lld gathered costs need %lld",
                (long long)r->side_ws_bytes, (long long)(width * r->world),
                (long long)(i2lqr_argmin_workspace_bytes(width * r->world) + 16));
  if (h->cfg.layout == I2LQR_LAYOUT_BATCH_TILED && (r->B & 63))
    return fail(I2LQR_ERR_INVALID, "the batch-tiled layout needs a batch that is a multiple of 64");
  hipStream_t s = (hipStream_t)stream;
  hipStream_t ss = side_stream ? (hipStream_t)side_stream : s;
  const bool two = ss != s;
  if (two && !h->ev_ready) {
    HIP_TRY(hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_side_done, hipEventDisableTiming));
  }
  if (r->guard_previous && h->side_pending) HIP_TRY(hipStreamWaitEvent(s, h->ev_side_done, 0));
  // -- the shard (launch stream) -------------------------------------------------------------------
  if (r->B > 0) {
    if (r->n_iters >= 0) {
      if (int rc = i2lqr_iterate_pick(h, r->B, r->n_iters, r->X, r->U, r->x_term, r->lamb, r->obs,
                                      r->cost, r->K, r->k, r->iters, r->status, r->qfun,
                                      r->outer_iter, r->max_relax_iter, r->cost_it, r->local_best,
                                      r->local_best_cost, r->pick_ws, r->pick_ws_bytes, stream))
        return rc;
    } else {
      if (!r->qfun) return fail(I2LQR_ERR_INVALID, "null buffer");
      if (int rc = i2lqr_solve(h, r->B, r->X, r->U, r->x_term, r->lamb, r->obs, r->cost, r->K, r->k,
                               r->iters, r->status, stream)) return rc;
      if (int rc = i2lqr_relax_cost(h, r->B, r->X, r->x_term, r->qfun, r->outer_iter,
                                    r->max_relax_iter, r->cost_it, stream)) return rc;
      if (int rc = i2lqr_argmin(h, r->B, r->cost_it, r->local_best, r->local_best_cost, r->pick_ws,
                                r->pick_ws_bytes, stream)) return rc;
    }
  }
  if (two) {
    HIP_TRY(hipEventRecord(h->ev_ready, s));
    HIP_TRY(hipStreamWaitEvent(ss, h->ev_ready, 0));
  }
  // -- the exchange (side stream) ------------------------------------------------------------------
  const bool ragged = r->B != width;
  {
    int64_t padblocks = ragged ? (width + 255) / 256 : 1;
    if (padblocks > 64) padblocks = 64;
    visit_precision(h->cfg, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((k_round_prepare<T>), dim3((unsigned)padblocks), dim3(256), 0, ss, r->B, n,
                         m, N, (int)h->cfg.layout, (const T*)r->X, (const T*)r->U, r->local_best,
                         (T*)r->pack_local, width, (const T*)r->cost_it,
                         ragged ? (T*)r->cost_padded : (T*)nullptr);
    });
    HIP_TRY(hipGetLastError());
  }
  const void* src = ragged ? r->cost_padded : r->cost_it;
  if (comm && !r->loopback) {
    if (int rc = i2lqr_allgather_round(h, comm, src, r->cost_all, width, r->pack_local, r->pack_all,
                                       P, (void*)ss)) return rc;
  } else {  // a world of one without RCCL, or one process playing rank after rank: own slots only
    const size_t item = h->cfg.dtype == I2LQR_F64 ? 8 : 4;
    char* ca = (char*)r->cost_all + (size_t)r->rank * (size_t)width * item;
    char* pa = (char*)r->pack_all + (size_t)r->rank * (size_t)P * item;
    HIP_TRY(hipMemcpyAsync(ca, src, (size_t)width * item, hipMemcpyDeviceToDevice, ss));
    HIP_TRY(hipMemcpyAsync(pa, r->pack_local, (size_t)P * item, hipMemcpyDeviceToDevice, ss));
  }
  if (int rc = i2lqr_round_pick(h, r->world, width, r->total, P, r->cost_all, r->pack_all,
                                r->best_cost, r->winner, r->best_global, r->side_ws,
                                r->side_ws_bytes, (void*)ss)) return rc;
  if (two) {
    HIP_TRY(hipEventRecord(h->ev_side_done, ss));
    h->side_pending = true;
  }
  return debug_check(I2LQR_OK, (void*)ss);
}

}  // extern "C"
