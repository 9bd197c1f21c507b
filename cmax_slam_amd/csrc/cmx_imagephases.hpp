// cmx_imagephases.hpp -- the tile phases shared by the image kernels of cmx_kernels.hip, ONE device-inline definition of each.
// Two are those kernels' correctness contract: the operation order of the forward blur (blur_row / blur_col) and the clearing
// and un-flagging of the ping-pong partner plane (tile_clear_partner).  tile_* functions are whole phases: every thread of the
// workgroup calls them, and those that hold a barrier say so.  Included by cmx_kernels.hip (st_sc1 is defined there) and, for the
// load and the Gaussian passes alone, by cmx_recon.hip (recon_smooth_kernel: no moments, so no st_sc1).
// A helper is optimised on its own before it is inlined, so moving text here is not neutral; what therefore stays in the kernels
// (tables and timings: profiles/image_phases_refactor.txt):
//   * the register copy of the taps: as a function it grew image_adjoint2_kernel's scratch (36 -> 44, 28 -> 44, 44 -> 76 bytes);
//   * the G^T passes of image_adjoint_sobel_kernel: with their folds in a function its <-1> form went from 81 to 80 or 97 VGPRs,
//     across an occupancy step either way;
//   * all of image_adjoint_kernel: its <-1> forms crossed occupancy steps with the folds or the moment stores in functions
//     (80 -> 96, 87 -> 104 VGPRs), ran 7 % longer with blur_row / blur_col in its G^T passes, and its <4, false> form measured
//     2-3 % longer (11.4-11.6 against 11.1-11.2 us) over any of the shared phases.  It uses the named list bits only and compiles
//     to the parent's instruction stream.
#pragma once
#include "cmx_internal.hpp"

namespace cmx {

__device__ __forceinline__ void st_sc1(double *p, double v);  // defined in cmx_kernels.hip, with the finalize helpers

__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = (p < 0) ? -p : 2 * (len - 1) - p;
  return p;
}

// Tile occupancy (ImgArgs::flags_*): is there anything non-zero within `reach` pixels of tile (tx, ty)?
__device__ __forceinline__ bool tile_active(const ImgArgs &a, int tx, int ty, int reach, int TX, int TY) {
  if (!a.flags_cur) return true;
  const int nx = (reach + TX - 1) / TX, ny = (reach + TY - 1) / TY;
  bool any = false;
  for (int dy = -ny; dy <= ny; dy++)
    for (int dx = -nx; dx <= nx; dx++) {
      const int x = tx + dx, y = ty + dy;
      if (x < 0 || y < 0 || x >= a.tiles_x || y >= a.tiles_y) continue;  // REFLECT_101 mirrors pixels of the same tiles
      const int t = y * a.tiles_x + x;
      any = any || a.flags_cur[t] != 0 || (a.igp && a.flags_igp && a.flags_igp[t] != 0);
    }
  return any;
}

// ---------------------------------------------------------------------------------------------- work-list entries
// An entry of the compacted tile list (written by tile_list_kernel / tile_mark_kernel + tile_list_ordered_kernel): the tile
// index, whether anything lies within reach of it, whether its tile of the ping-pong partner plane has to be cleared.
constexpr unsigned kTileIndexMask = 0x3fffffffu, kTilePartnerDirty = 0x40000000u, kTileActive = 0x80000000u;
constexpr unsigned kTileMarked = 0x20000000u;  // dense scratch array of the ordered list only: "listed" (tile 0 is all-zero otherwise)
__device__ __forceinline__ unsigned tile_entry(int tile, bool active, bool dirty) {
  return (unsigned)tile | (active ? kTileActive : 0u) | (dirty ? kTilePartnerDirty : 0u);
}

struct TileWork {
  unsigned entry;  // LIST: the list entry; otherwise the tile index
  int tile, x0, y0;
  int slot;        // row position of this tile's partial moments
};
// Work-loop header.  LIST: walk the compacted list with a bounded grid (wi = list position); otherwise wi is the tile.
// LIST holds a BARRIER (the LDS of the previous tile is free): every thread of the workgroup reaches it.
template <int TX, int TY, bool LIST>
__device__ __forceinline__ TileWork tile_begin(const ImgArgs &a, int wi) {
  TileWork w;
  w.entry = LIST ? a.tile_list[wi] : (unsigned)wi;
  w.tile = (int)(w.entry & kTileIndexMask);
  w.x0 = (w.tile % a.tiles_x) * TX;
  w.y0 = (w.tile / a.tiles_x) * TY;
  w.slot = LIST ? wi : w.tile;
  if (LIST) __syncthreads();
  return w;
}
template <bool LIST>  // does this tile of the partner plane hold votes?  (only asked when a.zero_ptr is set)
__device__ __forceinline__ bool tile_partner_dirty(const ImgArgs &a, const TileWork &w) {
  return LIST ? (w.entry & kTilePartnerDirty) != 0 : (!a.flags_other || a.flags_other[w.tile] != 0);
}
template <int TX, int TY, bool LIST>  // anything non-zero within `reach` pixels?  Workgroup-uniform.
__device__ __forceinline__ bool tile_in_reach(const ImgArgs &a, const TileWork &w, int reach) {
  return LIST ? (w.entry & kTileActive) != 0 : tile_active(a, w.tile % a.tiles_x, w.tile / a.tiles_x, reach, TX, TY);
}

// Clear this tile of the other accumulation buffer (ping-pong: no memset launch next time; nobody reads it during this
// launch), then un-flag it -- under LIST the list pre-pass has already done that.  !LIST holds a BARRIER (every thread has
// read the flag before thread 0 clears it): a.zero_ptr is launch-uniform, and no per-thread exit sits in front of it.
template <int TX, int TY, int NT, bool LIST>
__device__ __forceinline__ void tile_clear_partner(const ImgArgs &a, const TileWork &w) {
  if (!a.zero_ptr) return;
  const bool dirty = tile_partner_dirty<LIST>(a, w);
  if (dirty)
    for (int idx = threadIdx.x; idx < TX * TY * a.zero_planes; idx += NT) {
      const int pl = idx / (TX * TY), q = idx - pl * (TX * TY);
      const int gx = w.x0 + (q % TX), gy = w.y0 + (q / TX);
      if (gx < a.W && gy < a.H) a.zero_ptr[(size_t)pl * a.W * a.H + (size_t)gy * a.W + gx] = 0.f;
    }
  if (!LIST) {
    __syncthreads();
    if (threadIdx.x == 0 && a.flags_other && dirty) a.flags_other[w.tile] = 0;
  }
}

// ---------------------------------------------------------------------------------------------- moments
// How a tile's two moments leave the workgroup (thread 0 stores them).  Also the exit of a tile with nothing within reach:
// zero moments, in the plain or the write-through mode (the caller keeps its `continue` / `return`).
enum MomentStore {
  kMomentsPlain,         // rows of the partial table, read by a later launch
  kMomentsWriteThrough,  // the same rows, read by the last-arriving workgroup of THIS launch (tail finalize)
  kMomentsAccumulate     // accumulator rows, fp64 atomics in arrival order; exact zeros are skipped
};
template <MomentStore MODE>
__device__ __forceinline__ void tile_store_moments(const ImgArgs &a, int slot, double t0, double t1) {
  if (threadIdx.x != 0) return;
  if (MODE == kMomentsAccumulate) {  // read by every workgroup of the gradient pass queued behind this launch
    double *row = a.macc + (size_t)(slot % kTailShards) * 16;
    if (t0 != 0.0) __hip_atomic_fetch_add(row, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t1 != 0.0) __hip_atomic_fetch_add(row + 1, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if (MODE == kMomentsWriteThrough) {
    st_sc1(a.partials + (size_t)0 * a.nblk + slot, t0);
    st_sc1(a.partials + (size_t)1 * a.nblk + slot, t1);
  } else {
    a.partials[(size_t)0 * a.nblk + slot] = t0;
    a.partials[(size_t)1 * a.nblk + slot] = t1;
  }
}

// ---------------------------------------------------------------------------------------------- load
// The composed raw tile fl32(IGp * alpha + (IL_old + IL_new)) with a REFLECT_101 halo, aw x ah, origin (x0 - halo, y0 - halo).
// The product comes first, then the sum (no contraction: -ffp-contract=off).
template <int NT>
__device__ __forceinline__ void tile_load_composed(const ImgArgs &a, float alpha, int x0, int y0, int halo, int aw, int ah, float *buf) {
  for (int idx = threadIdx.x; idx < aw * ah; idx += NT) {
    const int ly = idx / aw, lx = idx - ly * aw;
    const int gx = reflect101(x0 + lx - halo, a.W), gy = reflect101(y0 + ly - halo, a.H);
    const size_t off = (size_t)gy * a.W + gx;
    float v = a.src_a[off];
    if (a.src_b) v = v + a.src_b[off];      // IL = IL_old + IL_new
    if (a.igp) v = a.igp[off] * alpha + v;  // I = IGp*alpha + IL
    buf[idx] = v;
  }
}

// ---------------------------------------------------------------------------------------------- Gaussian passes
// R >= 0: compile-time radius (loops unroll, taps live in registers, index maths is constant); -1: the runtime radius r.
// The forward blur in the reference's operation order -- what makes B and the moments bit-identical to its non-FMA build:
//   Row pass:  s = k[0]*S[x-r]; s += k[j]*S[x-r+j]           (generic row filter order)
//   Col pass:  s = k[r]*T[y];   s += k[r+j]*(T[y+j]+T[y-j])  (symmetric column filter order)
template <int R, int N>  // S: the leftmost input, x - r
__device__ __forceinline__ float blur_row(const float (&taps)[N], int r, const float *S) {
  const int rr = (R >= 0) ? R : r;
  float s = taps[0] * S[0];
#pragma unroll
  for (int j = 1; j <= 2 * rr; j++) s += taps[j] * S[j];
  return s;
}
template <int R, int N>  // T: the centre input, rows `stride` apart
__device__ __forceinline__ float blur_col(const float (&taps)[N], int r, const float *T, int stride) {
  const int rr = (R >= 0) ? R : r;
  float s = taps[rr] * T[0];
#pragma unroll
  for (int t = 1; t <= rr; t++) s += taps[rr + t] * (T[t * stride] + T[-t * stride]);
  return s;
}
// forward row pass of `rows` rows: src (sw wide) -> dst (dw = sw - 2r wide)
template <int R, int NT, int N>
__device__ __forceinline__ void tile_blur_rows(const float (&taps)[N], int r, const float *src, int sw, float *dst, int dw, int rows) {
  for (int idx = threadIdx.x; idx < dw * rows; idx += NT) {
    const int ly = idx / dw, lx = idx - ly * dw;
    dst[idx] = blur_row<R>(taps, r, src + ly * sw + lx);
  }
}

}  // namespace cmx
