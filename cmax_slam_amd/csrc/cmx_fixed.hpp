// cmx_fixed.hpp -- the 2^-30 fixed-point vote representation (CMX_OPT_DETERMINISTIC) and the two forms of a bilinear vote
// that reaches global memory, shared by the LDS splats (cmx_binning.hip) and the whole-trajectory reconstruction
// (cmx_recon.hip).  Device inline only.
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

}  // namespace cmx
