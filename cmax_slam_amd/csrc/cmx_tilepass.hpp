// cmx_tilepass.hpp -- the adjoint image pass of ONE strip (32 x 16 pixels) of a 32 x 32 sort tile, run by a workgroup of the front-end
// LDS splat's launch the moment the strip's inputs are complete (tile-dataflow fusion, FusedArgs in cmx_internal.hpp; round 6).
//
// Same arithmetic as image_adjoint2_kernel<4, ..> (cmx_kernels.hip), pixel for pixel:
//   raw (tile + 2r)  ->  [row pass: G_x raw on tile rows +-r, M_x raw on tile rows +-2r]  ->  [column pass: B and Jt on the tile]
// B = G I in the operation order of image_moments_kernel (plain fp32 multiply / add, no contraction), Jt = My (Mx I) with the
// 17-term sums of the banded operator M = G^T G accumulated in fp64 (reference: cv::GaussianBlur of the IWE,
// local_image_warped_events.cpp:32-38, and the variance / gradient of local_focus_funcs.cpp:26-44 in its adjoint form,
// DESIGN.md section 4.2).  Only the grouping of the two image moments differs (32 x 16 strips instead of 64 x 16 tiles).
//
// Memory model.  The raw pixels were written by OTHER workgroups of the SAME launch, on any XCD, with agent-scope atomic adds
// (performed at the coherent level), and every one of those workgroups drained its atomics (s_waitcnt vmcnt(0)) before its
// arrival on the tile's counter -- so the completing arrival may read them, provided it does not hit a stale line of its own
// XCD's L2 / its CU's L1: the loads are agent-scope (sc1) loads, the same rule as the tail finalize (cmx_kernels.hip,
// tail_arrive: "sc1 loads may replace the acquire only when the producer stored sc1").  Everything the pass writes (Jt, the
// partner's cleared tile, moment rows) is read by LATER launches.
//
// Two forms of the two compute phases.  fused_tile_pass_legacy: one output per thread per sweep, 17 LDS reads per output -- bound by
// that LDS traffic (137 LDS read instructions per thread, 68 of them 8-byte).  fused_tile_pass_blocked (the two-launch default,
// FUSE = 1): four outputs per thread from one register window, 5 + 8 wide LDS reads per thread, the interior operator row in SGPRs
// -- row phase 1.36 -> 1.12 us (now bound by VALU issue: the fp64 FMAs, conversions and the fp32 G_x taps of 48-of-64-lane waves),
// column phase 1.28 -> 0.52 us, the 1M-event launch 17.5 -> 15.8 us (profiles/tilepass_register_blocked.txt).  The one-launch forms
// (FUSE = 2, 3) keep the legacy pass: their register budgets have no room for the windows.
#pragma once
#include "cmx_internal.hpp"

namespace cmx {

__device__ __forceinline__ int tp_reflect101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
  return p;
}
__device__ __forceinline__ float tp_ld_sc1(const float *p) {
  return __uint_as_float(__hip_atomic_load(reinterpret_cast<const unsigned *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

constexpr int kTpR = 4, kTpT = kBinTile, kTpH = kBinTile / kFuseStrips;  // a strip: kTpT columns x kTpH lines
constexpr int kTpAW = kTpT + 4 * kTpR, kTpAH = kTpH + 4 * kTpR, kTpGH = kTpH + 2 * kTpR, kTpTap = 4 * kTpR + 1;
// LDS of one pass: reduction scratch | raw (float) | G_x raw (float) | M_x raw (double) | the strip's rows of M_y (double)
constexpr size_t kTpLdsBytes = sizeof(double) * 32 + sizeof(float) * ((size_t)kTpAW * kTpAH + (size_t)kTpT * kTpGH) +
                               sizeof(double) * ((size_t)kTpT * kTpAH + (size_t)kTpH * kTpTap);
constexpr int kTpRawPerThread = (kTpAW * kTpAH + 511) / 512;  // raw pixels per thread of a 512-thread workgroup

// N agent-scope (sc1) dword loads in flight at once, then ONE wait.  As relaxed atomic loads the compiler waits for each of them
// in turn (dependent ~1-2 us trips to memory per tile); the loads and the wait therefore live in one asm statement.
__device__ __forceinline__ void tp_ld_sc1_n(const float *const (&p)[3], float (&v)[3]) {
  asm volatile(
      "global_load_dword %0, %3, off sc1\n\t"
      "global_load_dword %1, %4, off sc1\n\t"
      "global_load_dword %2, %5, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2])
      : "v"(p[0]), "v"(p[1]), "v"(p[2])
      : "memory");
}
__device__ __forceinline__ void tp_ld_sc1_n(const float *const (&p)[5], float (&v)[5]) {
  asm volatile(
      "global_load_dword %0, %5, off sc1\n\t"
      "global_load_dword %1, %6, off sc1\n\t"
      "global_load_dword %2, %7, off sc1\n\t"
      "global_load_dword %3, %8, off sc1\n\t"
      "global_load_dword %4, %9, off sc1\n\t"
      "s_waitcnt vmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4])
      : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4])
      : "memory");
}


// the strip's two moments: wave sums, one LDS slot per wave, thread 0 adds them in wave order
template <int NT, bool PUB>
__device__ __forceinline__ void tp_store_moments(const FusedArgs &f, int strip, double *red, double sI, double sII) {
  const int tid = threadIdx.x;
  double v0 = sI, v1 = sII;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    v0 += __shfl_xor(v0, o, 64);
    v1 += __shfl_xor(v1, o, 64);
  }
  const int wave = tid >> 6, lane = tid & 63;
  if (lane == 0) { red[2 * wave] = v0; red[2 * wave + 1] = v1; }
  __syncthreads();
  if (tid == 0) {
    double t0 = 0, t1 = 0;
    for (int w = 0; w < NT / 64; w++) { t0 += red[2 * w]; t1 += red[2 * w + 1]; }
    if (f.macc) {  // device-driven solve: accumulator rows read by every workgroup of the gradient pass queued behind this launch
      double *row = f.macc + (size_t)(strip % kTailShards) * 16;
      if (t0 != 0.0) __hip_atomic_fetch_add(row, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (t1 != 0.0) __hip_atomic_fetch_add(row + 1, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      const int nstrips = f.tiles_x * f.tiles_y * kFuseStrips;
      if (PUB) {
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(f.partials + strip), (unsigned long long)__double_as_longlong(t0),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(f.partials + nstrips + strip), (unsigned long long)__double_as_longlong(t1),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        f.partials[strip] = t0;
        f.partials[nstrips + strip] = t1;
      }
    }
  }
}

// NT threads (a multiple of kTpT, at least 64), all of them call; `lds` = kTpLdsBytes bytes, 16-byte aligned, free for this call.
// wait_inputs(): called by every thread once everything that does NOT depend on the tile's votes has been requested (operator
// rows, taps) -- it returns (in every thread, behind a workgroup barrier) whether the votes are complete; false: nothing is computed.
// The caller issues a barrier before it reuses `lds`.
// PUB: the pass's outputs (Jt, the moment row) are read by OTHER workgroups of the same launch (the one-launch evaluation's gather
// role and finalize): stored write-through (agent scope), the caller publishes the strip's done flag behind them.
template <int NT, bool PUB, typename WaitFn>
__device__ __forceinline__ void fused_tile_pass_legacy(const FusedArgs &f, const float *plane, int W, int H, int strip, unsigned char *lds,
                                                WaitFn wait_inputs) {
  constexpr int R = kTpR, T = kTpT, TH = kTpH, AW = kTpAW, AH = kTpAH, GH = kTpGH, NTAP = kTpTap, NRAW = kTpRawPerThread;
  static_assert(NT % T == 0 && NT >= 64 && NT % 64 == 0, "tile pass geometry");
  static_assert(AW * AH <= NRAW * NT, "raw pixels per thread");
  constexpr int ROWS = NT / T;  // strip lines one sweep of the workgroup covers
  double *red = reinterpret_cast<double *>(lds);
  float *bufA = reinterpret_cast<float *>(lds + 32 * sizeof(double));  // raw, AW x AH
  float *bufG = bufA + AW * AH;                                        // G_x raw, T x GH (strip lines -r .. TH+r)
  double *bufM = reinterpret_cast<double *>(bufG + T * GH);            // M_x raw (rounded to fp32, kept as fp64), T x AH (lines -2r .. TH+2r)
  double *bufY = bufM + T * AH;                                        // rows of M_y for the strip's TH lines, TH x NTAP, as fp64
  static_assert((sizeof(double) * 32 + sizeof(float) * (AW * AH + T * GH)) % 8 == 0, "fp64 buffers 8-byte aligned");
  const int tid = threadIdx.x, tx = tid % T, ty0 = tid / T;
  const int tile = strip / kFuseStrips;
  const int x0 = (tile % f.tiles_x) * T, y0 = (tile / f.tiles_x) * T + (strip % kFuseStrips) * TH;
  if (y0 >= H) {  // (the lower strips of a partial bottom tile row lie outside the image: nothing to compute, but the counter is consumed)
    (void)wait_inputs();
    return;
  }
  // ---- what does not depend on the votes: taps, this column's row of M_x (registers), the strip's rows of M_y (LDS) -- the
  // operator rows as fp64: v_cvt_f64_f32 is a quarter-rate instruction, and with both factors of every one of the pass's 2 x 17
  // products per pixel converted where they are used the conversions were most of the pass (2.7 us of LDS / ALU phases per tile)
  float taps[2 * R + 1];
#pragma unroll
  for (int j = 0; j < 2 * R + 1; j++) taps[j] = f.taps[j];
  double mx[NTAP];
  {
    const bool interior = x0 >= 2 * R && x0 + T - 1 <= W - 1 - 2 * R;
    const float *row = f.Mx + (size_t)(interior ? 2 * R : min(x0 + tx, W - 1)) * NTAP;
#pragma unroll
    for (int i = 0; i < NTAP; i++) mx[i] = (double)row[i];
  }
  {
    const bool interior = y0 >= 2 * R && y0 + TH - 1 <= H - 1 - 2 * R;
    for (int idx = tid; idx < TH * NTAP; idx += NT) {
      const int ty = idx / NTAP, i = idx - ty * NTAP;
      bufY[idx] = (double)f.My[(size_t)(interior ? 2 * R : min(y0 + ty, H - 1)) * NTAP + i];
    }
  }
  // raw strip + 2r halo (REFLECT_101 beyond the image for G_x; M's rows carry zeros there): addresses first
  const float *rp[NRAW];
#pragma unroll
  for (int k = 0; k < NRAW; k++) {
    const int idx = min(tid + k * NT, AW * AH - 1);
    const int ly = idx / AW, lx = idx - ly * AW;
    const int gx = tp_reflect101(x0 + lx - 2 * R, W), gy = tp_reflect101(y0 + ly - 2 * R, H);
    rp[k] = plane + (size_t)gy * W + gx;
  }
  if (!wait_inputs()) return;
  {
    float v[NRAW];
    tp_ld_sc1_n(rp, v);
#pragma unroll
    for (int k = 0; k < NRAW; k++)
      if (tid + k * NT < AW * AH) bufA[tid + k * NT] = v[k];
  }
  if (f.trace && tid == 0) f.trace[8 * (size_t)blockIdx.x + 4] = wall_clock64();
  if (f.zero_ptr) {  // ping-pong: the previous evaluation's votes on this strip (nobody reads that buffer in this launch)
    for (int idx = tid; idx < T * TH; idx += NT) {
      const int gx = x0 + (idx % T), gy = y0 + (idx / T);
      if (gx < W && gy < H) f.zero_ptr[(size_t)gy * W + gx] = 0.f;
    }
  }
  __syncthreads();
  for (int ly = ty0; ly < AH; ly += ROWS) {  // row pass: raw row ly, output column tx
    const float *S = bufA + ly * AW + tx;
    float in[NTAP];
#pragma unroll
    for (int i = 0; i < NTAP; i++) in[i] = S[i];
    // four independent fp64 chains (i mod 4) instead of one of 17 dependent FMAs: with two waves per SIMD nothing hides a dependent
    // v_fma_f64's latency.  (The sum's grouping differs from image_adjoint2's: ~1e-16 relative, before the rounding to fp32.)
    double mc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) mc[q] = mx[q] * (double)in[q];
#pragma unroll
    for (int i = 4; i < NTAP; i++) mc[i & 3] = __builtin_fma(mx[i], (double)in[i], mc[i & 3]);
    const double m = (mc[0] + mc[1]) + (mc[2] + mc[3]);
    bufM[ly * T + tx] = (double)(float)m;  // (rounded to fp32 as image_adjoint2 stores it)
    if (ly >= R && ly < R + GH) {  // forward row pass, same op order as image_moments
      float s = taps[0] * in[R];
#pragma unroll
      for (int j = 1; j <= 2 * R; j++) s += taps[j] * in[R + j];
      bufG[(ly - R) * T + tx] = s;
    }
  }
  __syncthreads();
  if (f.trace && tid == 0) f.trace[8 * (size_t)blockIdx.x + 5] = wall_clock64();
  double sI = 0, sII = 0;
  for (int ty = ty0; ty < TH; ty += ROWS) {  // column pass: B (moments) and Jt at (x0 + tx, y0 + ty)
    const int gx = x0 + tx, gy = y0 + ty;
    if (gx < W && gy < H) {
      const float *Tg = bufG + (ty + R) * T + tx;
      float s = taps[R] * Tg[0];
#pragma unroll
      for (int t = 1; t <= R; t++) s += taps[R + t] * (Tg[t * T] + Tg[-t * T]);
      sI += (double)s;
      sII += (double)s * (double)s;
      const double *my = bufY + ty * NTAP;  // (wave-uniform per half wave: LDS broadcast)
      const double *Q = bufM + ty * T + tx;
      double jc[4];
#pragma unroll
      for (int q = 0; q < 4; q++) jc[q] = my[q] * Q[q * T];
#pragma unroll
      for (int i = 4; i < NTAP; i++) jc[i & 3] = __builtin_fma(my[i], Q[i * T], jc[i & 3]);
      const double j = (jc[0] + jc[1]) + (jc[2] + jc[3]);
      if (PUB) __hip_atomic_store(reinterpret_cast<unsigned *>(f.jt + (size_t)gy * W + gx), __float_as_uint((float)j), __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
      else f.jt[(size_t)gy * W + gx] = (float)j;
    }
  }
  if (f.trace && tid == 0) f.trace[8 * (size_t)blockIdx.x + 6] = wall_clock64();
  tp_store_moments<NT, PUB>(f, strip, red, sI, sII);
}

// ---------------------------------------------------------------------------------------------- the register-blocked pass
// Both compute phases produce kTpL = 4 consecutive outputs ALONG THE FILTER DIRECTION from one register window of 16 + 4 inputs
// (5 LDS values and 5 conversions per output instead of 17 and 17), and the interior row of M_x / M_y (workgroup-uniform, the same
// floating-point sum on both axes) is an fp64 kernel argument: a v_fma_f64 takes it as SGPR pairs -- no LDS read, no VGPR.
//   row pass      wave w = the four columns 4w .. 4w+3, lane = raw line (48 of 64 lanes): ten ds_read_b64 of the line's 20 raw values.
//                 bufA's stride is 66 floats = 2 banks per line, so the 32 lines of a half wave hit 32 distinct 8-byte bank pairs.
//                 G_x raw / M_x raw are stored TRANSPOSED (column-major, fp32): lane = line -> consecutive addresses.
//   column pass   a thread = four consecutive lines of one column: its windows are contiguous in the transposed buffers, 5 + 3
//                 ds_read_b128 (strides 52 / 44 floats: 16-byte aligned, the sixteen lanes of a b128 group on sixteen distinct
//                 16-byte slots).  Waves 0-3 compute Jt, waves 4-7 B and the moments: two short independent instruction streams
//                 per SIMD instead of one long one.
// Rows of M within 2r of the image border differ per output, and only those outputs leave the interior path: the row pass decides per
// wave (its four columns; their rows are wave-uniform loads from the table), the column pass per thread (its four lines; fp64 rows in
// LDS, bufY, as the one-output-per-thread pass kept them) -- a border tile runs mostly the interior path.  The row pass's border
// path takes one output at a time and reads its window from LDS again: with the window and a table row in registers the kernel spilled.
// Arithmetic per pixel: B as before, bit for bit; the 17-term fp64 sums as ONE chain in tap order (the four outputs of a thread are the
// independent chains; image_adjoint2's order), rounded to fp32 where they were.
constexpr int kTpL = 4;
constexpr int kTpSA = 66, kTpSM = kTpAH + 4, kTpSG = kTpGH + 4;  // strides (floats) of raw [line][x], M_x raw [x][line], G_x raw [x][line]
constexpr size_t kTpBlockedLdsBytes = sizeof(double) * 32 + sizeof(float) * ((size_t)kTpSA * kTpAH + (size_t)kTpT * kTpSG + (size_t)kTpT * kTpSM) +
                                      sizeof(double) * ((size_t)kTpH * kTpTap);
static_assert(kTpBlockedLdsBytes <= kTpLdsBytes, "the register-blocked pass needs no more LDS than the one-output-per-thread pass");
static_assert(kTpSA % 2 == 0 && kTpSA >= kTpAW + kTpL - 4 && kTpSM % 4 == 0 && kTpSG % 4 == 0 && kTpSM >= kTpAH && kTpSG >= kTpGH, "window alignment");
static_assert(kTpT % kTpL == 0 && kTpH % kTpL == 0 && kTpR == 4, "register blocking geometry");

template <int NT, bool PUB, typename WaitFn>
__device__ __forceinline__ void fused_tile_pass_blocked(const FusedArgs &f, const float *plane, int W, int H, int strip, unsigned char *lds,
                                                        WaitFn wait_inputs) {
  constexpr int R = kTpR, T = kTpT, TH = kTpH, AW = kTpAW, AH = kTpAH, GH = kTpGH, NTAP = kTpTap, NRAW = kTpRawPerThread;
  constexpr int L = kTpL, SA = kTpSA, SM = kTpSM, SG = kTpSG, NWIN = NTAP - 1 + L;
  static_assert(NT % 128 == 0 && AH <= 64, "tile pass geometry");
  static_assert(AW * AH <= NRAW * NT, "raw pixels per thread");
  double *red = reinterpret_cast<double *>(lds);
  float *bufA = reinterpret_cast<float *>(lds + 32 * sizeof(double));  // raw, AH lines of SA
  float *bufG = bufA + SA * AH;                                        // G_x raw, T columns of SG (strip lines -r .. TH+r)
  float *bufM = bufG + T * SG;                                         // M_x raw (rounded to fp32), T columns of SM (lines -2r .. TH+2r)
  double *bufY = reinterpret_cast<double *>(bufM + T * SM);            // y-border tiles: rows of M_y for the strip's TH lines, as fp64
  static_assert((sizeof(double) * 32) % 16 == 0 && (sizeof(float) * SA * AH) % 16 == 0 && (sizeof(float) * T * SG) % 16 == 0 &&
                    (sizeof(float) * T * SM) % 8 == 0, "16-byte windows, 8-byte rows");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = strip / kFuseStrips;
  const int x0 = (tile % f.tiles_x) * T, y0 = (tile / f.tiles_x) * T + (strip % kFuseStrips) * TH;
  if (y0 >= H) {  // (the lower strips of a partial bottom tile row lie outside the image: nothing to compute, but the counter is consumed)
    (void)wait_inputs();
    return;
  }
  const bool interior_y = f.M_in_ok && y0 >= 2 * R && y0 + TH - 1 <= H - 1 - 2 * R;
  // ---- what does not depend on the votes: the taps and the interior row of M_x / M_y out of the argument block (scalar loads --
  // pinned into SGPRs HERE: left to the compiler they are issued where they are used, a trip to memory behind each barrier of the
  // critical path), a y-border tile's rows of M_y (LDS), the raw pixels' addresses
  float taps[2 * R + 1];
  double mi[NTAP];
#pragma unroll
  for (int j = 0; j < 2 * R + 1; j++) {
    taps[j] = f.taps[j];
    asm volatile("" : "+s"(taps[j]));
  }
#pragma unroll
  for (int i = 0; i < NTAP; i++) {
    mi[i] = f.M_in[i];
    asm volatile("" : "+s"(mi[i]));
  }
  if (!interior_y) {
    for (int idx = tid; idx < TH * NTAP; idx += NT) {
      const int ty = idx / NTAP, i = idx - ty * NTAP;
      bufY[idx] = (double)f.My[(size_t)min(y0 + ty, H - 1) * NTAP + i];
    }
  }
  // raw strip + 2r halo (REFLECT_101 beyond the image for G_x; M's rows carry zeros there): addresses first
  const float *rp[NRAW];
  int ra[NRAW];  // (where the pixel goes in bufA)
#pragma unroll
  for (int k = 0; k < NRAW; k++) {
    const int idx = min(tid + k * NT, AW * AH - 1);
    const int ly = idx / AW, lx = idx - ly * AW;
    const int gx = tp_reflect101(x0 + lx - 2 * R, W), gy = tp_reflect101(y0 + ly - 2 * R, H);
    rp[k] = plane + (size_t)gy * W + gx;
    ra[k] = ly * SA + lx;
  }
  if (!wait_inputs()) return;
  {
    float v[NRAW];
    tp_ld_sc1_n(rp, v);
#pragma unroll
    for (int k = 0; k < NRAW; k++)
      if (tid + k * NT < AW * AH) bufA[ra[k]] = v[k];
  }
  if (f.trace && tid == 0) f.trace[8 * (size_t)blockIdx.x + 4] = wall_clock64();
  if (f.zero_ptr) {  // ping-pong: the previous evaluation's votes on this strip (nobody reads that buffer in this launch)
    for (int idx = tid; idx < T * TH; idx += NT) {
      const int gx = x0 + (idx % T), gy = y0 + (idx / T);
      if (gx < W && gy < H) f.zero_ptr[(size_t)gy * W + gx] = 0.f;
    }
  }
  __syncthreads();
  // ---- row pass: raw line `lane`, output columns 4 kg .. 4 kg + 3
  for (int kg = wave; kg < T / L; kg += NT / 64) {
    if (lane < AH) {
      float in[NWIN];
      {
        const float2 *S = reinterpret_cast<const float2 *>(bufA + lane * SA + L * kg);
#pragma unroll
        for (int i = 0; i < NWIN / 2; i++) {
          const float2 v = S[i];
          in[2 * i] = v.x;
          in[2 * i + 1] = v.y;
        }
      }
      double acc[L];
      // one row of M_x for every column at least 2r from the image's border: the fp64 kernel arguments (SGPR pairs)
      if (f.M_in_ok && x0 + L * kg >= 2 * R && x0 + L * kg + L - 1 <= W - 1 - 2 * R) {
#pragma unroll
        for (int w = 0; w < NWIN; w++) {
          const double d = (double)in[w];
#pragma unroll
          for (int j = 0; j < L; j++) {
            const int i = w - j;
            if (i == 0) acc[j] = mi[0] * d;
            else if (i > 0 && i < NTAP) acc[j] = __builtin_fma(mi[i], d, acc[j]);
          }
        }
#pragma unroll
        for (int j = 0; j < L; j++) bufM[(L * kg + j) * SM + lane] = (float)acc[j];  // (rounded to fp32 as image_adjoint2 stores it)
      } else {  // the (at most 2r + L - 1) columns next to the border: each has its own row (wave-uniform), one output at a time
#pragma unroll 1
        for (int j = 0; j < L; j++) {
          const float *row = f.Mx + (size_t)min(x0 + L * kg + j, W - 1) * NTAP;
          const float *S = bufA + lane * SA + L * kg + j;
          double m = (double)row[0] * (double)S[0];
#pragma unroll
          for (int i = 1; i < NTAP; i++) m = __builtin_fma((double)row[i], (double)S[i], m);
          bufM[(L * kg + j) * SM + lane] = (float)m;
        }
      }
      if (lane >= R && lane < R + GH) {  // forward row pass, same op order as image_moments
#pragma unroll
        for (int j = 0; j < L; j++) {
          float s = taps[0] * in[j + R];
#pragma unroll
          for (int t = 1; t <= 2 * R; t++) s += taps[t] * in[j + R + t];
          bufG[(L * kg + j) * SG + (lane - R)] = s;
        }
      }
    }
  }
  __syncthreads();
  if (f.trace && tid == 0) f.trace[8 * (size_t)blockIdx.x + 5] = wall_clock64();
  // ---- column pass: items 0 .. T*TH/L - 1 compute Jt, the next T*TH/L items B and the moments, each on lines 4 m .. 4 m + 3 of column tx
  double sI = 0, sII = 0;
  constexpr int NIT = T * TH / L;
  static_assert(NIT % 64 == 0, "the two roles split at a wave boundary");
  for (int it = tid; it < 2 * NIT; it += NT) {
    const bool moments = it >= NIT;  // (wave-uniform)
    const int q = moments ? it - NIT : it, tx = q % T, m = q / T;
    const int gx = x0 + tx, gy = y0 + L * m;
    if (gx >= W || gy >= H) continue;
    if (moments) {
      float g[2 * R + L];
      {
        const float4 *S = reinterpret_cast<const float4 *>(bufG + tx * SG + L * m);
#pragma unroll
        for (int i = 0; i < (2 * R + L) / 4; i++) {
          const float4 v = S[i];
          g[4 * i] = v.x; g[4 * i + 1] = v.y; g[4 * i + 2] = v.z; g[4 * i + 3] = v.w;
        }
      }
#pragma unroll
      for (int j = 0; j < L; j++) {
        float s = taps[R] * g[j + R];
#pragma unroll
        for (int t = 1; t <= R; t++) s += taps[R + t] * (g[j + R + t] + g[j + R - t]);
        if (gy + j < H) {
          sI += (double)s;
          sII += (double)s * (double)s;
        }
      }
    } else {
      float in[NWIN];
      {
        const float4 *S = reinterpret_cast<const float4 *>(bufM + tx * SM + L * m);
#pragma unroll
        for (int i = 0; i < NWIN / 4; i++) {
          const float4 v = S[i];
          in[4 * i] = v.x; in[4 * i + 1] = v.y; in[4 * i + 2] = v.z; in[4 * i + 3] = v.w;
        }
      }
      double acc[L];
      if (f.M_in_ok && gy >= 2 * R && gy + L - 1 <= H - 1 - 2 * R) {  // lines at least 2r from the border: the same row of M_y
#pragma unroll
        for (int w = 0; w < NWIN; w++) {
          const double d = (double)in[w];
#pragma unroll
          for (int j = 0; j < L; j++) {
            const int i = w - j;
            if (i == 0) acc[j] = mi[0] * d;
            else if (i > 0 && i < NTAP) acc[j] = __builtin_fma(mi[i], d, acc[j]);
          }
        }
      } else {  // lines next to the border: each has its own row, fp64 in LDS (uniform per half wave: broadcast)
#pragma unroll
        for (int j = 0; j < L; j++) {
          const double *my = bufY + (L * m + j) * NTAP;
          double a = my[0] * (double)in[j];
#pragma unroll
          for (int i = 1; i < NTAP; i++) a = __builtin_fma(my[i], (double)in[j + i], a);
          acc[j] = a;
        }
      }
#pragma unroll
      for (int j = 0; j < L; j++) {
        if (gy + j < H) {
          if (PUB) __hip_atomic_store(reinterpret_cast<unsigned *>(f.jt + (size_t)(gy + j) * W + gx), __float_as_uint((float)acc[j]),
                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else f.jt[(size_t)(gy + j) * W + gx] = (float)acc[j];
        }
      }
    }
  }
  if (f.trace && tid == 0) f.trace[8 * (size_t)blockIdx.x + 6] = wall_clock64();
  tp_store_moments<NT, PUB>(f, strip, red, sI, sII);
}

// CMX_TILEPASS_LEGACY: the one-output-per-thread pass (17 LDS reads per output), kept selectable for same-box A/Bs
// (tools/build_variant.sh tp_legacy "-DCMX_TILEPASS_LEGACY", tools/microbench/tilepass.hip runs both side by side)
template <int NT, bool PUB, typename WaitFn>
__device__ __forceinline__ void fused_tile_pass(const FusedArgs &f, const float *plane, int W, int H, int strip, unsigned char *lds,
                                                WaitFn wait_inputs) {
#ifdef CMX_TILEPASS_LEGACY
  fused_tile_pass_legacy<NT, PUB>(f, plane, W, H, strip, lds, wait_inputs);
#else
  fused_tile_pass_blocked<NT, PUB>(f, plane, W, H, strip, lds, wait_inputs);
#endif
}

}  // namespace cmx
