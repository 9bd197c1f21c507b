// cmx_fixed.hpp -- the 2^-30 fixed-point vote representation (CMX_OPT_DETERMINISTIC), the two forms of a bilinear vote
// that reaches global memory and the vote into an LDS window, shared by the LDS splats (cmx_binning.hip) and the
// whole-trajectory reconstruction (cmx_recon.hip).  Device inline only.
#pragma once
#include "cmx_warp.hpp"

namespace cmx {

typedef unsigned long long fix_t;
constexpr float kFixScale = 1073741824.0f;        // 2^30
constexpr double kFixInv = 1.0 / 1073741824.0;
__device__ __forceinline__ fix_t to_fix(float w) { return (fix_t)(unsigned)(w * kFixScale + 0.5f); }

__device__ __forceinline__ void vote4_global(float *img, int W, int xx, int yy, float dx, float dy) {
  float *q = img + (size_t)yy * W + xx;
  atomic_add_f32(q, (1.f - dx) * (1.f - dy));
  atomic_add_f32(q + 1, dx * (1.f - dy));
  atomic_add_f32(q + W, (1.f - dx) * dy);
  atomic_add_f32(q + W + 1, dx * dy);
}
// 64-bit INTEGER adds: they commute, so the plane is the same bits whatever order the votes arrive in
__device__ __forceinline__ void vote4_global_fix(fix_t *img, int W, int xx, int yy, float dx, float dy) {
  fix_t *q = img + (size_t)yy * W + xx;
  atomicAdd(q, to_fix((1.f - dx) * (1.f - dy)));
  atomicAdd(q + 1, to_fix(dx * (1.f - dy)));
  atomicAdd(q + W, to_fix((1.f - dx) * dy));
  atomicAdd(q + W + 1, to_fix(dx * dy));
}

// The two votes with a temporal weight and a sign (the voxel grids of a reconstruction): every bilinear product of vote4_global,
// formed the same way, times wt, negated when neg -- s * (wt * wb) in fp32.  The fixed-point form converts the magnitude and
// negates the integer: two's complement, so the cell is read back as SIGNED.
__device__ __forceinline__ void vote4_global_w(float *img, int W, int xx, int yy, float dx, float dy, float wt, bool neg) {
  float *q = img + (size_t)yy * W + xx;
  const float m0 = wt * ((1.f - dx) * (1.f - dy)), m1 = wt * (dx * (1.f - dy)), m2 = wt * ((1.f - dx) * dy), m3 = wt * (dx * dy);
  atomic_add_f32(q, neg ? -m0 : m0);
  atomic_add_f32(q + 1, neg ? -m1 : m1);
  atomic_add_f32(q + W, neg ? -m2 : m2);
  atomic_add_f32(q + W + 1, neg ? -m3 : m3);
}
__device__ __forceinline__ void vote4_global_fix_w(fix_t *img, int W, int xx, int yy, float dx, float dy, float wt, bool neg) {
  fix_t *q = img + (size_t)yy * W + xx;
  const fix_t m0 = to_fix(wt * ((1.f - dx) * (1.f - dy))), m1 = to_fix(wt * (dx * (1.f - dy)));
  const fix_t m2 = to_fix(wt * ((1.f - dx) * dy)), m3 = to_fix(wt * (dx * dy));
  atomicAdd(q, neg ? 0ull - m0 : m0);
  atomicAdd(q + 1, neg ? 0ull - m1 : m1);
  atomicAdd(q + W, neg ? 0ull - m2 : m2);
  atomicAdd(q + W + 1, neg ? 0ull - m3 : m3);
}

// The same vote into a workgroup's LDS window (kBinWindow^2 cells, row stride kBinStride).  LDS accumulators are 64-bit fixed point
// (2^-30 units), not fp32: on gfx950 ds_add_f32 retires ONE lane at a time (193 G lane-atomics/s for any address pattern) while
// ds_add_u64 runs at 1.7 T/s (tools/microbench/lds_atomics.hip).  Integer adds also commute, so a window's sum does not depend on
// the order the votes arrive in; the quantisation (<= 2^-31 per vote) is far below fp32's own rounding of the reference's accumulators.
__device__ __forceinline__ void lds_add_fix(fix_t *p, fix_t v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void vote4_lds(fix_t *win, int lx, int ly, float dx, float dy) {
  fix_t *q = win + ly * kBinStride + lx;
  lds_add_fix(q, to_fix((1.f - dx) * (1.f - dy)));
  lds_add_fix(q + 1, to_fix(dx * (1.f - dy)));
  lds_add_fix(q + kBinStride, to_fix((1.f - dx) * dy));
  lds_add_fix(q + kBinStride + 1, to_fix(dx * dy));
}

}  // namespace cmx
