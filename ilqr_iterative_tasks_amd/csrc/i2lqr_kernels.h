// The fused and function-level kernels of the one-problem-per-wavefront family (i2lqr_wave.hpp) and
// of the bicycles' one-problem-per-lane family (i2lqr_lane.hpp) are compiled in translation units
// of their own (i2lqr_wave.hip; i2lqr_lane_f64.hip, i2lqr_lane_f32.hip: the cut by measured compile
// time); i2lqr_abi.hip launches them through these declarations.
// A kernel i2lqr_abi.hip launches that is missing here is compiled into that unit again
// (tests/test_isa_abi_unit.py); one declared here and instantiated nowhere fails the link.
#pragma once
#include "i2lqr_lane.hpp"
#include "i2lqr_wave.hpp"

namespace i2lqr {

// One problem per wavefront: what Launch<T, Sys> launches for a plant, with (QR) and without stage
// weights ...
#define I2LQR_WAVE_KERNELS_(DECL, REAL, SYS, N_, M_, QR)                                           \
  DECL void k_iterate<REAL, SYS<REAL>, 64, QR>(const DevCfg<REAL, N_, M_>, const IterArgs<REAL>);  \
  DECL void k_rollout<REAL, SYS<REAL>, 64, QR>(const DevCfg<REAL, N_, M_>, int64_t, REAL*, REAL*,  \
                                               const REAL*, REAL*);                                \
  DECL void k_backward<REAL, SYS<REAL>, 64, QR>(const DevCfg<REAL, N_, M_>, int64_t, const REAL*,  \
                                                const REAL*, const REAL*, const REAL*,             \
                                                const REAL*, REAL*, REAL*);                        \
  DECL void k_forward<REAL, SYS<REAL>, 64, QR>(const DevCfg<REAL, N_, M_>, int64_t, const REAL*,   \
                                               const REAL*, const REAL*, const REAL*, const REAL*, \
                                               REAL*, REAL*, REAL*);
// ... and, for the bicycles (Launch::kHasFstep), the per-step-Jacobian form and the chunked solve's
// tail
#define I2LQR_WAVE_FSTEP_KERNELS_(DECL, REAL, SYS, N_, M_, QR)                                     \
  DECL void k_iterate<REAL, SYS<REAL>, 64, QR, true>(const DevCfg<REAL, N_, M_>,                   \
                                                     const IterArgs<REAL>);                        \
  DECL void k_iterate<REAL, SYS<REAL>, 64, QR, true, true>(const DevCfg<REAL, N_, M_>,             \
                                                           const IterArgs<REAL>);
#define I2LQR_WAVE_KERNELS(DECL, REAL)                                                             \
  I2LQR_WAVE_KERNELS_(DECL, REAL, Bicycle4, 4, 2, false)                                           \
  I2LQR_WAVE_KERNELS_(DECL, REAL, Bicycle4, 4, 2, true)                                            \
  I2LQR_WAVE_KERNELS_(DECL, REAL, Bicycle6, 6, 2, false)                                           \
  I2LQR_WAVE_KERNELS_(DECL, REAL, Bicycle6, 6, 2, true)                                            \
  I2LQR_WAVE_KERNELS_(DECL, REAL, Quad12, 12, 4, false)                                            \
  I2LQR_WAVE_KERNELS_(DECL, REAL, Quad12, 12, 4, true)                                             \
  I2LQR_WAVE_FSTEP_KERNELS_(DECL, REAL, Bicycle4, 4, 2, false)                                     \
  I2LQR_WAVE_FSTEP_KERNELS_(DECL, REAL, Bicycle4, 4, 2, true)                                      \
  I2LQR_WAVE_FSTEP_KERNELS_(DECL, REAL, Bicycle6, 6, 2, false)                                     \
  I2LQR_WAVE_FSTEP_KERNELS_(DECL, REAL, Bicycle6, 6, 2, true)

// One problem per lane, the bicycles (quad12: i2lqr_lane12.h): what LaneLaunch<T, Sys, TILED>
// launches for a plant, stage weights (QR) and layout (TL: batch-tiled), and the chunked solve's
// compaction
#define I2LQR_LANE_KERNELS_(DECL, REAL, SYS, N_, M_, QR, TL)                                       \
  DECL void k_lane_iterate<REAL, SYS<REAL>, QR, TL>(const DevCfg<REAL, N_, M_>,                    \
                                                    const LaneArgs<REAL>);                         \
  DECL void k_lane_rollout<REAL, SYS<REAL>, QR, TL>(const DevCfg<REAL, N_, M_>, int64_t, REAL*,    \
                                                    REAL*, const REAL*, REAL*);                    \
  DECL void k_lane_backward<REAL, SYS<REAL>, QR, TL>(const DevCfg<REAL, N_, M_>, int64_t,          \
                                                     const REAL*, const REAL*, const REAL*,        \
                                                     const REAL*, const REAL*, REAL*, REAL*);      \
  DECL void k_lane_forward<REAL, SYS<REAL>, QR, TL>(const DevCfg<REAL, N_, M_>, int64_t,           \
                                                    const REAL*, const REAL*, const REAL*,         \
                                                    const REAL*, const REAL*, REAL*, REAL*, REAL*);
#define I2LQR_LANE_BICYCLE_KERNELS_(DECL, REAL, SYS, N_, M_)                                       \
  I2LQR_LANE_KERNELS_(DECL, REAL, SYS, N_, M_, false, false)                                       \
  I2LQR_LANE_KERNELS_(DECL, REAL, SYS, N_, M_, false, true)                                        \
  I2LQR_LANE_KERNELS_(DECL, REAL, SYS, N_, M_, true, false)                                        \
  I2LQR_LANE_KERNELS_(DECL, REAL, SYS, N_, M_, true, true)
#define I2LQR_LANE_COMPACT_(DECL, REAL, TL)                                                        \
  DECL void k_lane_compact<REAL, TL>(int, int, int, LaneSet<REAL>, int, const int32_t*,            \
                                     LaneSet<REAL>, int32_t*, LaneSet<REAL>, unsigned long long*);
#define I2LQR_LANE_KERNELS(DECL, REAL)                                                             \
  I2LQR_LANE_BICYCLE_KERNELS_(DECL, REAL, Bicycle4, 4, 2)                                          \
  I2LQR_LANE_BICYCLE_KERNELS_(DECL, REAL, Bicycle6, 6, 2)                                          \
  I2LQR_LANE_COMPACT_(DECL, REAL, false) I2LQR_LANE_COMPACT_(DECL, REAL, true)

// (an explicit instantiation definition may follow its declaration: the units include this header
// as it is)
I2LQR_WAVE_KERNELS(extern template __global__, double)
I2LQR_WAVE_KERNELS(extern template __global__, float)
I2LQR_LANE_KERNELS(extern template __global__, double)
I2LQR_LANE_KERNELS(extern template __global__, float)

}  // namespace i2lqr
