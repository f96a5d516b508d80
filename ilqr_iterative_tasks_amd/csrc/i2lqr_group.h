// Launchers of the eight- / sixteen-lanes-per-problem kernels (i2lqr_group.hpp, i2lqr_quad.hpp),
// compiled in their own translation units (i2lqr_group.hip, i2lqr_quad.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/i2lqr.h"
#include "i2lqr_column_plan.hpp"
#include "i2lqr_devcfg.hpp"
#include "i2lqr_wave.hpp"

namespace i2lqr {

// Which form of these kernels a call runs on, with how many wavefronts per workgroup, and what fits
// the device's LDS is decided in i2lqr_column_plan.hpp from a ColumnFit: what the configuration says
// itself, then the bytes of the layouts, filled by the unit that owns them (i2lqr_group.hip: the
// bicycles' eight- / sixteen-lane forms; i2lqr_quad.hip: quad12's; Layout<Sys> by Launch::prepare).
inline ColumnFit column_fit_config(const i2lqr_config& cfg) {
  ColumnFit f;
  f.plant = cfg.m == 2 && cfg.n + cfg.m <= 8 ? ColumnFit::BICYCLE
            : cfg.n + cfg.m == 16 ? ColumnFit::SIXTEEN : ColumnFit::OTHER;
  f.weights = has_stage_weights(cfg);
  f.problem_major = cfg.layout == I2LQR_LAYOUT_PROBLEM_MAJOR;
  f.f64 = cfg.dtype == I2LQR_F64;
  f.n = cfg.n;
  f.N = cfg.N;
  f.word = f.f64 ? 8 : 4;
  return f;
}
void column_fit_group(const i2lqr_config& cfg, ColumnFit& fit);
void column_fit_quad(const i2lqr_config& cfg, ColumnFit& fit);

// Enqueue k_group_iterate for B problems (problem-major layout) with 1 or 3 wavefronts per workgroup
// (group8_wavefronts).  Returns hipSuccess or the HIP error of the attribute call / launch.
template <class T> hipError_t group_iterate(const i2lqr_config& cfg, const IterArgs<T>& a,
                                            hipStream_t stream, int wavefronts);

// The same column scheme with SIXTEEN lanes per problem — one problem per 16-lane DPP row, four per
// wavefront — whose backward step exchanges columns by DPP row broadcasts instead of LDS round trips
// (i2lqr_group.hpp: GroupWorker::backward_row).
// wavefronts: 1, 2 or 3 per workgroup (group16_wavefronts); fixed: the fixed-horizon kernel below
// (group16_fixed: the horizon must be one it is built for)
template <class T> hipError_t group16_iterate(const i2lqr_config& cfg, const IterArgs<T>& a,
                                              hipStream_t stream, int wavefronts, bool fixed);
// Fixed-horizon form of the sixteen-lane kernel (k_group_iterate_fixed: the horizon a compile-time
// constant, the fast passes straight-line code), compiled in i2lqr_group_fixed.hip for the horizons
// of this list — THE list: instantiations and dispatch both expand it.  20 is the horizon of the
// BASELINE configs 2-4.  Each entry is twelve kernels (two plants, two precisions, H = 1, 2, 3).
#define I2LQR_GROUP_FIXED_HORIZONS(X) X(20)
bool group16_fixed_horizon(int N);
// wavefronts: 1, 2 or 3 per workgroup, as group16_iterate chose them; N must be in the list
template <class T> hipError_t group16_iterate_fixed(const i2lqr_config& cfg, const IterArgs<T>& a,
                                                    hipStream_t stream, int wavefronts);

// Workspace form of the eight-lane kernel (records and gains in a caller-provided HBM workspace of
// group_ws_bytes() for B problems: 4 KB of LDS per problem, four wavefronts per CU)
template <class T> hipError_t group_iterate_ws(const i2lqr_config& cfg, const IterArgs<T>& a,
                                               void* ws, hipStream_t stream);

// The speculative form (k_group_spec: V wavefronts per workgroup, wavefront v runs the iteration that
// follows v rejects): small batches only.  lanes = 8 (eight problems per workgroup, LDS exchanges)
// or 16 (four problems per workgroup, the DPP passes of the sixteen-lane form: shorter rounds, and
// three workgroups fit a CU's LDS instead of one).  wavefronts: 2 or 3 (spec_wavefronts).
template <class T> hipError_t group_spec_iterate(const i2lqr_config& cfg, const IterArgs<T>& a,
                                                 hipStream_t stream, int lanes, int wavefronts);
// Chains (k_group_spec<.., CHAIN>): a.B chains of a.chain_len problems each, stored chain after chain,
// solved in ONE launch — the final lamb of a chain's problem c is the initial lamb of its problem
// c + 1 (utils/base.py:393, :414-426: the controller's chained regularisation).  Supported for the
// plants of the speculative kernel with Q = R = 0 in the problem-major layout, up to the batch of
// its three-wavefront form (512 chains on 256 CUs): spec_chain_fits.
template <class T> hipError_t group_spec_chain(const i2lqr_config& cfg, const IterArgs<T>& a,
                                               hipStream_t stream);
// The same kernel on the first *a.count (<= a.count_max) columns of a batch-minor work set: the tail
// of the chunked solves of the one-problem-per-lane layouts (IterArgs::count / set_stride /
// max_total).  Supported for the plants of the eight-lane kernel with Q = R = 0, whatever the
// handle's layout is; sixteen lanes per problem where that fits the LDS (spec_tail_lanes).
bool group_spec_tail_supported(const i2lqr_config& cfg);
template <class T> hipError_t group_spec_tail(const i2lqr_config& cfg, const IterArgs<T>& a,
                                              hipStream_t stream);

// Sixteen lanes per problem (i2lqr_quad.hpp; the n + m = 16 plant quad12, Q = R = 0): needs a
// caller-provided HBM workspace of quad_ws_bytes() for B problems.
template <class T> hipError_t quad_iterate(const i2lqr_config& cfg, const IterArgs<T>& a, void* ws,
                                           hipStream_t stream);

}  // namespace i2lqr
