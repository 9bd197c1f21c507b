// cmx_recon.hip -- whole-trajectory panorama reconstruction (cmx_backend_recon_*): all events of a recording warped along the
// final spline, whatever its knot count, into ONE plane.
//
//   recon_delta     once per begin: delta_i = log(knot_i^-1 knot_{i+1}) for the K-1 neighbouring pairs -- the value part of
//                   PairConsts (cmx_so3.hpp) in device memory: a logarithm, a square root and an atan out of every batch pose
//   recon_votes     one launch per slice: a workgroup owns a run of consecutive packed events = a run of consecutive batches;
//                   its first lanes evaluate one batch pose each into LDS (So3Spline<N>::evaluate, value only: the arithmetic
//                   of spline_eval<N, false> with knots / delta read from global memory at segment s .. s+N-1), and after one
//                   barrier all lanes walk the run's events with be_warp_math<0> and vote (event_pano_warper.cpp:262-311
//                   without the old / new split).  No pose table in global memory, no tile sort, no second launch.
//                   POL (cmx_backend_recon_pol_add*): the same walk, the same cell and weights, but the four adds go to the ON or
//                   the OFF plane by the event's polarity, and the voting events are counted per plane.
//   recon_set_votes   the same walk with the targets of a set as the targets of the votes -- the planes of M pinhole views
//                   (recon_view_votes), the bins of G voxel grids (recon_voxel_votes), the cells of S time surfaces
//                   (recon_surface_votes: one 64-bit integer max per vote) -- ONE skeleton, further down with its description, and
//                   a Target per set; recon_surface_fill and recon_surface_decay beside it
//   recon_smooth, recon_score   the way back from the map to the events (cmx_backend_recon_score*): S = G plane, and the export's walk
//                   with S read at every event's vote cell -- further down with their description
//   recon_fixed_to_float   deterministic mode: the 2^-30 fixed-point plane as fp32, leaving it as it is (accumulation goes on)
#include "../../include/cmax_hip.h"
#include "cmx_internal.hpp"
#include "cmx_warp.hpp"
#include "cmx_fixed.hpp"
#include "cmx_imagephases.hpp"

namespace cmx {

// Packed events per workgroup.  A run starts at a multiple of itself, so it touches at most run / per_batch + 2 batches:
// kReconMaxRun whole ones for small batches, at most 2048 / 8 + 2 otherwise -- what the LDS pose table below holds.  A batch
// longer than a run (batch size 5000) is shared by several workgroups, each of which evaluates its pose for itself.
int recon_run(int per_batch) {
  const long long r = (long long)kReconMaxRun * per_batch;
  return r < 2048 ? (int)r : 2048;
}

__global__ __launch_bounds__(256) void recon_delta_kernel(const Quat *knots, int K, double *delta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i + 1 >= K) return;
  double d[3];
  so3_log(q_mul(q_conj(knots[i]), knots[i + 1]), d);
  delta[3 * i] = d[0]; delta[3 * i + 1] = d[1]; delta[3 * i + 2] = d[2];
}
void launch_recon_delta(const Quat *knots, int K, double *delta, hipStream_t s) {
  if (K < 2) return;
  hipLaunchKernelGGL(recon_delta_kernel, dim3((K - 1 + 255) / 256), dim3(256), 0, s, knots, K, delta);
}

template <int N>
__device__ __forceinline__ void recon_pose(const ReconArgs &a, long long t_ns, double *R) {
  const long long st = t_ns - a.start_ns;
  long long s = st / a.dt_ns;
  // (every batch time was validated before the launch: st >= 0 and s + N <= K; the clamp keeps a bad one inside the tables)
  const long long s_max = (long long)a.K - N;
  s = s < 0 ? 0 : (s > s_max ? s_max : s);
  const double u = (double)(st % a.dt_ns) / (double)a.dt_ns;
  double p[N], coeff[N];
  p[0] = 1.0;
  double ti = u;
#pragma unroll
  for (int j = 1; j < N; j++) { p[j] = 1.0 * ti; ti = ti * u; }
#pragma unroll
  for (int i = 0; i < N; i++) {
    double c = 0;
#pragma unroll
    for (int j = 0; j < N; j++) c += a.blend[i * N + j] * p[j];
    coeff[i] = c;
  }
  Quat res = a.knots[s];
#pragma unroll
  for (int i = 0; i < N - 1; i++) {
    const double *d = a.delta + 3 * (s + i);
    const double k = coeff[i + 1];
    res = q_mul(res, so3_exp(d[0] * k, d[1] * k, d[2] * k));
  }
  const Mat3 M = q_to_R(res);
#pragma unroll
  for (int c = 0; c < 9; c++) R[c] = M.m[c];
}

template <int N, bool FIXED, bool POL = false>
__global__ __launch_bounds__(kReconThreads) void recon_votes_kernel(const ReconArgs a) {
  __shared__ double sh_R[(kReconMaxRun + 2) * 9];
  __shared__ unsigned sh_inside;
  __shared__ unsigned sh_inside_off;  // (POL: sh_inside counts the ON votes, this one the OFF votes)
  const int e0 = blockIdx.x * a.run;  // (the grid covers [0, n): e0 < n)
  const int e1 = (a.n - e0 > a.run) ? e0 + a.run : a.n;
  const int b0 = e0 / a.per_batch;
  int nbw = (e1 - 1) / a.per_batch - b0 + 1;
  if (nbw > kReconMaxRun + 2) nbw = kReconMaxRun + 2;  // (cannot happen with run = recon_run(per_batch))
  if (threadIdx.x == 0) sh_inside = 0;
  if (POL && threadIdx.x == 0) sh_inside_off = 0;
  for (int j = threadIdx.x; j < nbw; j += kReconThreads) {
    const int b = b0 + j < a.nb ? b0 + j : a.nb - 1;
    recon_pose<N>(a, a.batch_t[b], sh_R + 9 * j);
  }
  __syncthreads();
  unsigned inside = 0, inside_off = 0;
  const size_t off_plane = (size_t)a.cam.Hp * a.cam.Wp;
  int cur = -1;
  double R[9];
  for (int i = e0 + threadIdx.x; i < e1; i += kReconThreads) {
    const int b = i / a.per_batch;
    int j = b - b0;
    j = j < nbw ? j : nbw - 1;
    if (j != cur) {
#pragma unroll
      for (int c = 0; c < 9; c++) R[c] = sh_R[9 * j + c];
      cur = j;
    }
    // sampling restarts at every batch start (event_pano_warper.cpp:262): packed slot k of batch b is raw event b * B + k * stride
    const size_t src = a.stride ? (size_t)b * a.B + (size_t)(i - b * a.per_batch) * a.stride : (size_t)i;
    const uint32_t word = a.xy[src];
    const uint32_t e = word & 0x7fffffffu;
    // POL: the store's byte (a.pol is a kernel argument: uniform), read beside the word, or the word's own bit 31
    const bool on = POL && (a.pol ? a.pol[src] != 0 : (word >> 31) != 0);
    const int ex = e & 0xffff, ey = e >> 16;
    double v0, v1, v2;
    load_bearing(a.cam, ex, ey, v0, v1, v2);
    const BeWarp w = be_warp_math<0>(a.cam, e, b, v0, v1, v2, R);
    if (w.ok) {  // 1 <= xx < Wp - 2 && 1 <= yy < Hp - 2: the four cells are inside the plane
      const size_t at = POL && !on ? off_plane : 0;  // (POL: the same four adds, into the plane the polarity selects)
      if (FIXED) vote4_global_fix(a.fixed + at, a.cam.Wp, w.xx, w.yy, w.dx, w.dy);
      else vote4_global(a.plane + at, a.cam.Wp, w.xx, w.yy, w.dx, w.dy);
      if (POL && !on) inside_off++;
      else inside++;
    }
  }
  // events that voted: one wave reduction, one atomic per workgroup (POL: per plane)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) inside += __shfl_down(inside, off, 64);
  if ((threadIdx.x & 63) == 0 && inside) atomicAdd(&sh_inside, inside);
  if (POL) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) inside_off += __shfl_down(inside_off, off, 64);
    if ((threadIdx.x & 63) == 0 && inside_off) atomicAdd(&sh_inside_off, inside_off);
  }
  __syncthreads();
  if (threadIdx.x == 0 && sh_inside) atomicAdd(a.n_inside, (unsigned long long)sh_inside);
  if (POL && threadIdx.x == 0 && sh_inside_off) atomicAdd(a.n_inside + 1, (unsigned long long)sh_inside_off);
}

void launch_recon_votes(const ReconArgs &a, hipStream_t s) {
  if (a.n <= 0 || a.nb <= 0) return;
  const dim3 g((unsigned)(((long long)a.n + a.run - 1) / a.run)), b(kReconThreads);  // (a.n <= 2^30: cmx_reconstruct.cpp)
  if (a.order == 2) {
    if (a.fixed) hipLaunchKernelGGL((recon_votes_kernel<2, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((recon_votes_kernel<2, false>), g, b, 0, s, a);
  } else {
    if (a.fixed) hipLaunchKernelGGL((recon_votes_kernel<4, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((recon_votes_kernel<4, false>), g, b, 0, s, a);
  }
}

void launch_recon_votes_pol(const ReconArgs &a, hipStream_t s) {
  if (a.n <= 0 || a.nb <= 0) return;
  const dim3 g((unsigned)(((long long)a.n + a.run - 1) / a.run)), b(kReconThreads);
  if (a.order == 2) {
    if (a.fixed) hipLaunchKernelGGL((recon_votes_kernel<2, true, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((recon_votes_kernel<2, false, true>), g, b, 0, s, a);
  } else {
    if (a.fixed) hipLaunchKernelGGL((recon_votes_kernel<4, true, true>), g, b, 0, s, a);
    else hipLaunchKernelGGL((recon_votes_kernel<4, false, true>), g, b, 0, s, a);
  }
}

// ---------------------------------------------------------------------------------------------- target sets: views, voxel grids, surfaces
// recon_set_votes   cmx_backend_recon_view_add* / _voxel_add* / _surface_add*: the run structure of recon_votes -- the first lanes
//                evaluate the run's batch poses into LDS -- with the n targets of a set, virtual pinhole cameras with a time range
//                each, as the targets of the votes.  Beside the poses the workgroup forms the span [tmin, tmax] of its run's times:
//                of the batch times, kept in LDS, for a set that votes by batch time, or of the EVENT times (the per-event stream
//                ev_t, read at the index of the packed word; every event is looked at, so the span holds for any order of the
//                events -- and a batch of 5000 events spans several targets) by wave reduction and one LDS atomic per wave.  After
//                the barrier the workgroup scans the table of ranges ONCE, 16 bytes per target and lane, and lists the targets whose
//                [t_lo, t_hi) meets that span; the per-event cost therefore depends on the targets a run meets (one or two for
//                disjoint frames), not on n.  The listed targets are taken kReconViewChunk at a time: their entries (R^T,
//                intrinsics, range, index, and what the set adds) are copied into LDS word by word, one barrier, then all lanes walk
//                the run's events: the world ray R_batch * bearing is formed once per event and chunk (be_rotate, the vote kernel's
//                own function on the vote kernel's own pose), and for every target of the chunk that holds the time it is turned
//                into the camera, projected, tested in floating point (recon_view_project) and voted as the set's Target says.  A
//                run that meets more targets than a chunk holds walks its events again for the next chunk (the bearing and the pose
//                are re-read; the votes of a target do not depend on the chunking).  Votes per target are counted in LDS and leave
//                by one global atomic per listed target and workgroup.
//                What a Target supplies: Args (ReconSetArgs and its tail) and Entry (whole 8-byte words, its view first);
//                kEventSpan (span and membership by ev_t, not by batch time); reads_polarity (whether the event's polarity is
//                looked at: the store's byte, or bit 31 of the word); vote (one hit).  What stays per set, once, here: a workgroup's
//                list holds any subset of kReconMaxViews targets (the begin calls refuse more); an entry is 128 or 136 bytes and a
//                chunk of them has at most one word per lane.
constexpr int kReconMaxViews = 4096;
static_assert(sizeof(ReconViewDev) == 128 && sizeof(ReconVoxelDev) == 136 && sizeof(ReconViewRange) == 16, "set entries are copied word by word");

// a world ray in one view: turned into the camera and projected, and the vote test -- in floating point, before any conversion: a
// NaN fails it, and only values inside the plane are ever cast
struct ReconViewHit { double u, w; bool ok; };
__device__ __forceinline__ ReconViewHit recon_view_project(const ReconViewDev &V, double rx, double ry, double rz, double u_hi, double w_hi) {
  double x, y, z;
  be_rotate<false>(V.Rt, rx, ry, rz, x, y, z);
  const double iz = 1.0 / z;
  const double u = V.fx * (x * iz) + V.cx;
  const double w = V.fy * (y * iz) + V.cy;
  return ReconViewHit{u, w, z > 0.0 && u >= 1.0 && u < u_hi && w >= 1.0 && w < w_hi};
}

// pinhole views: the four bilinear adds of vote4_global / vote4_global_fix into the view's plane
template <bool FIXED>
struct ReconViewTarget {
  using Args = ReconViewArgs;
  using Entry = ReconViewDev;
  static constexpr bool kEventSpan = false;
  static __device__ __forceinline__ const ReconViewDev &view(const Entry &V) { return V; }
  static __device__ __forceinline__ bool reads_polarity(const Args &) { return false; }
  static __device__ __forceinline__ void vote(const Args &g, const Entry &V, const ReconViewHit &p, long long, bool, size_t np) {
    const int xx = (int)p.u, yy = (int)p.w;
    const float dx = (float)(p.u - xx), dy = (float)(p.w - yy);
    const size_t at = (size_t)V.index * np;
    if (FIXED) vote4_global_fix(g.fixed + at, g.set.Wv, xx, yy, dx, dy);
    else vote4_global(g.planes + at, g.set.Wv, xx, yy, dx, dy);
  }
};

// voxel grids: the view vote's cell and weights, tau = (t_i - t_lo) * scale in fp64, b0 = min((int)tau, n_bins - 2),
// f = (float)(tau - b0), and the four bilinear adds times 1 - f into bin b0 and times f into bin b0 + 1 (n_bins == 1: one bin, weight
// 1), negated for an OFF event of a signed set.  A bin whose weight is zero is skipped: it would add zeros.  Votes go to global
// memory: the two active bins of a grid are two planes, which no LDS window holds.
template <bool FIXED>
struct ReconVoxelTarget {
  using Args = ReconVoxelArgs;
  using Entry = ReconVoxelDev;
  static constexpr bool kEventSpan = true;
  static __device__ __forceinline__ const ReconViewDev &view(const Entry &G) { return G.v; }
  static __device__ __forceinline__ bool reads_polarity(const Args &g) { return g.is_signed != 0; }
  static __device__ __forceinline__ void vote(const Args &g, const Entry &G, const ReconViewHit &p, long long ti, bool neg, size_t np) {
    const int xx = (int)p.u, yy = (int)p.w;
    const float dx = (float)(p.u - xx), dy = (float)(p.w - yy);
    const int nbins = g.n_bins;
    int bin = 0;
    float w0 = 1.f, w1 = 0.f;
    if (nbins >= 2) {
      const double tau = (double)(ti - G.v.t_lo) * G.scale;  // (0 <= tau < n_bins - 1, up to its rounding: the cast is safe)
      bin = (int)tau;
      bin = bin < nbins - 2 ? bin : nbins - 2;
      w1 = (float)(tau - bin);
      w0 = 1.f - w1;
    }
    const size_t at = ((size_t)G.v.index * nbins + bin) * np;
    if (FIXED) {
      if (w0 != 0.f) vote4_global_fix_w(g.fixed + at, g.set.Wv, xx, yy, dx, dy, w0, neg);
      if (w1 != 0.f) vote4_global_fix_w(g.fixed + at + np, g.set.Wv, xx, yy, dx, dy, w1, neg);
    } else {
      if (w0 != 0.f) vote4_global_w(g.planes + at, g.set.Wv, xx, yy, dx, dy, w0, neg);
      if (w1 != 0.f) vote4_global_w(g.planes + at + np, g.set.Wv, xx, yy, dx, dy, w1, neg);
    }
  }
};

// time surfaces: the NEAREST pixel (int)(u + 0.5), (int)(w + 0.5) -- inside the plane because of the test -- and ONE signed 64-bit
// atomic max of t_i there, in channel 1 for an OFF event of a by-polarity set and in channel 0 otherwise.  The result of the max is
// not read.  No fixed-point form: a max of integers commutes and is idempotent.
struct ReconSurfaceTarget {
  using Args = ReconSurfaceArgs;
  using Entry = ReconViewDev;
  static constexpr bool kEventSpan = true;
  static __device__ __forceinline__ const ReconViewDev &view(const Entry &V) { return V; }
  static __device__ __forceinline__ bool reads_polarity(const Args &g) { return g.by_polarity != 0; }
  static __device__ __forceinline__ void vote(const Args &g, const Entry &V, const ReconViewHit &p, long long ti, bool off, size_t np) {
    const int cx = (int)(p.u + 0.5), cy = (int)(p.w + 0.5);  // (1 <= cx <= Wv - 2 and 1 <= cy <= Hv - 2: the test of the projection)
    const size_t per_surface = g.by_polarity ? 2 * np : np;
    long long *cell = g.cells + (size_t)V.index * per_surface + (off ? np : 0) + (size_t)cy * g.set.Wv + cx;
    atomicMax(cell, ti);
  }
};

template <int N, class Target>
__device__ __forceinline__ void recon_set_votes(const typename Target::Args &g) {
  using Entry = typename Target::Entry;
  constexpr bool kEventSpan = Target::kEventSpan;
  constexpr int kWords = sizeof(Entry) / 8;
  static_assert(kReconViewChunk * kWords <= kReconThreads, "one lane per word of a chunk");
  __shared__ double sh_R[(kReconMaxRun + 2) * 9];
  __shared__ long long sh_bt[kReconMaxRun + 2];  // (batch-time sets alone: the event-time form never names it, and it is not allocated)
  __shared__ Entry sh_entry[kReconViewChunk];
  __shared__ unsigned sh_cnt[kReconViewChunk];
  __shared__ unsigned short sh_match[kReconMaxViews];
  __shared__ unsigned sh_nmatch;
  __shared__ long long sh_tmin, sh_tmax;
  const ReconSetArgs &st = g.set;
  const ReconArgs &a = st.ev;
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * a.run;  // (the grid covers [0, n): e0 < n)
  const int e1 = (a.n - e0 > a.run) ? e0 + a.run : a.n;
  const int b0 = e0 / a.per_batch;
  int nbw = (e1 - 1) / a.per_batch - b0 + 1;
  if (nbw > kReconMaxRun + 2) nbw = kReconMaxRun + 2;  // (cannot happen with run = recon_run(per_batch))
  if (tid == 0) { sh_nmatch = 0; sh_tmin = 0x7fffffffffffffffLL; sh_tmax = -0x7fffffffffffffffLL - 1; }
  __syncthreads();
  for (int j = tid; j < nbw; j += kReconThreads) {
    const int b = b0 + j < a.nb ? b0 + j : a.nb - 1;
    const long long t = a.batch_t[b];
    recon_pose<N>(a, t, sh_R + 9 * j);
    if constexpr (!kEventSpan) {
      sh_bt[j] = t;
      atomicMin(&sh_tmin, t);
      atomicMax(&sh_tmax, t);
    }
  }
  long long tmin = 0x7fffffffffffffffLL, tmax = -0x7fffffffffffffffLL - 1;
  if constexpr (kEventSpan) {
    for (int i = e0 + tid; i < e1; i += kReconThreads) {
      const int b = i / a.per_batch;
      const size_t src = a.stride ? (size_t)b * a.B + (size_t)(i - b * a.per_batch) * a.stride : (size_t)i;
      const long long t = st.ev_t[src];
      tmin = t < tmin ? t : tmin;
      tmax = t > tmax ? t : tmax;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const long long lo = __shfl_down(tmin, off, 64), hi = __shfl_down(tmax, off, 64);
      tmin = lo < tmin ? lo : tmin;
      tmax = hi > tmax ? hi : tmax;
    }
    if ((tid & 63) == 0) { atomicMin(&sh_tmin, tmin); atomicMax(&sh_tmax, tmax); }
  }
  __syncthreads();
  // the targets that meet the run's span [tmin, tmax], in no particular order (integer sums, maxima and counts do not depend on it)
  tmin = sh_tmin; tmax = sh_tmax;
  for (int v = tid; v < st.n; v += kReconThreads) {
    const ReconViewRange r = st.ranges[v];
    if (r.t_lo <= tmax && r.t_hi > tmin) {
      const unsigned pos = atomicAdd(&sh_nmatch, 1u);
      if (pos < (unsigned)kReconMaxViews) sh_match[pos] = (unsigned short)v;
    }
  }
  __syncthreads();
  int nmatch = (int)sh_nmatch;
  nmatch = nmatch < kReconMaxViews ? nmatch : kReconMaxViews;
  const double u_hi = (double)(st.Wv - 2), w_hi = (double)(st.Hv - 2);
  const size_t np = (size_t)st.Hv * st.Wv;
  for (int c0 = 0; c0 < nmatch; c0 += kReconViewChunk) {  // (uniform: nmatch is the workgroup's)
    const int nl = nmatch - c0 < kReconViewChunk ? nmatch - c0 : kReconViewChunk;
    if (tid < nl * kWords) {
      const int k = tid / kWords, wd = tid - k * kWords;
      reinterpret_cast<long long *>(sh_entry)[tid] = reinterpret_cast<const long long *>(static_cast<const Entry *>(st.entries) + sh_match[c0 + k])[wd];
    }
    if (tid < kReconViewChunk) sh_cnt[tid] = 0;
    __syncthreads();
    int cur = -1;
    double R[9];
    long long ti = 0;
    for (int i = e0 + tid; i < e1; i += kReconThreads) {
      const int b = i / a.per_batch;
      int j = b - b0;
      j = j < nbw ? j : nbw - 1;
      if (j != cur) {
#pragma unroll
        for (int c = 0; c < 9; c++) R[c] = sh_R[9 * j + c];
        if constexpr (!kEventSpan) ti = sh_bt[j];
        cur = j;
      }
      // sampling restarts at every batch start: packed slot k of batch b is raw event b * B + k * stride (recon_votes_kernel)
      const size_t src = a.stride ? (size_t)b * a.B + (size_t)(i - b * a.per_batch) * a.stride : (size_t)i;
      const uint32_t word = a.xy[src];
      if constexpr (kEventSpan) ti = st.ev_t[src];
      const uint32_t e = word & 0x7fffffffu;
      // OFF, where the set looks: the store's byte (a.pol is a kernel argument: uniform), read beside the word, or the word's own bit 31
      const bool off = Target::reads_polarity(g) && !(a.pol ? a.pol[src] != 0 : (word >> 31) != 0);
      const int ex = e & 0xffff, ey = e >> 16;
      double v0, v1, v2, rx, ry, rz;
      load_bearing(a.cam, ex, ey, v0, v1, v2);
      be_rotate<false>(R, v0, v1, v2, rx, ry, rz);
      for (int k = 0; k < nl; k++) {
        const Entry &E = sh_entry[k];  // (one address for all lanes: LDS broadcasts)
        const ReconViewDev &V = Target::view(E);
        if (ti < V.t_lo || ti >= V.t_hi) continue;
        const ReconViewHit p = recon_view_project(V, rx, ry, rz, u_hi, w_hi);
        if (!p.ok) continue;
        Target::vote(g, E, p, ti, off, np);
        atomicAdd(&sh_cnt[k], 1u);
      }
    }
    __syncthreads();
    if (tid < nl) {  // (the lane that zeroes the counter of the next chunk)
      const unsigned cnt = sh_cnt[tid];
      if (cnt) atomicAdd(st.n_voted + Target::view(sh_entry[tid]).index, (unsigned long long)cnt);
    }
    __syncthreads();  // (the next chunk's entries overwrite sh_entry)
  }
}

// the kernels: the skeleton with each set's Target (their names are those the three sets have always had)
template <int N, bool FIXED>
__global__ __launch_bounds__(kReconThreads) void recon_view_votes_kernel(const ReconViewArgs g) { recon_set_votes<N, ReconViewTarget<FIXED>>(g); }
template <int N, bool FIXED>
__global__ __launch_bounds__(kReconThreads) void recon_voxel_votes_kernel(const ReconVoxelArgs g) { recon_set_votes<N, ReconVoxelTarget<FIXED>>(g); }
template <int N>
__global__ __launch_bounds__(kReconThreads) void recon_surface_votes_kernel(const ReconSurfaceArgs g) { recon_set_votes<N, ReconSurfaceTarget>(g); }

// the grid of a slice, and the kernel of the spline's order
template <class Args>
static void launch_recon_set_votes(const Args &g, void (*order2)(Args), void (*order4)(Args), hipStream_t s) {
  const ReconArgs &a = g.set.ev;
  if (a.n <= 0 || a.nb <= 0 || g.set.n <= 0) return;
  const dim3 gr((unsigned)(((long long)a.n + a.run - 1) / a.run)), b(kReconThreads);  // (a.n <= 2^30: cmx_reconstruct.cpp)
  hipLaunchKernelGGL(a.order == 2 ? order2 : order4, gr, b, 0, s, g);
}
void launch_recon_view_votes(const ReconViewArgs &g, hipStream_t s) {
  if (g.fixed) launch_recon_set_votes(g, recon_view_votes_kernel<2, true>, recon_view_votes_kernel<4, true>, s);
  else launch_recon_set_votes(g, recon_view_votes_kernel<2, false>, recon_view_votes_kernel<4, false>, s);
}
void launch_recon_voxel_votes(const ReconVoxelArgs &g, hipStream_t s) {
  if (g.fixed) launch_recon_set_votes(g, recon_voxel_votes_kernel<2, true>, recon_voxel_votes_kernel<4, true>, s);
  else launch_recon_set_votes(g, recon_voxel_votes_kernel<2, false>, recon_voxel_votes_kernel<4, false>, s);
}
void launch_recon_surface_votes(const ReconSurfaceArgs &g, hipStream_t s) {
  launch_recon_set_votes(g, recon_surface_votes_kernel<2>, recon_surface_votes_kernel<4>, s);
}

// every cell = "no event yet": INT64_MIN, a pattern no byte memset writes (surface_begin, surface_reset, restart)
__global__ __launch_bounds__(256) void recon_surface_fill_kernel(long long *cells, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) cells[i] = kReconSurfaceEmpty;
}
void launch_recon_surface_fill(long long *cells, size_t n, hipStream_t s) {
  if (n == 0) return;
  size_t blocks = (n + 1023) / 1024;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(recon_surface_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, s, cells, n);
}

// the surfaces read through an exponential decay, one cell per lane (8-byte load, 4-byte store): 0 for an empty cell, 1 at or behind
// the reference time, else exp(-(t_ref - T) / tau) -- the difference as an unsigned number: t_ref > T there, so it is exact whatever
// the two are -- with the quotient and the exponential in fp64, rounded once to fp32
__global__ __launch_bounds__(256) void recon_surface_decay_kernel(const long long *cells, const ReconViewRange *ranges, const long long *t_ref,
                                                                  size_t per_surface, double tau_ns, float *out) {
  const size_t k = blockIdx.y;  // the surface: its reference time is the workgroup's
  const long long tr = t_ref ? t_ref[k] : ranges[k].t_hi;
  cells += k * per_surface;
  out += k * per_surface;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per_surface; i += (size_t)gridDim.x * 256) {
    const long long T = cells[i];
    float v;
    if (T == kReconSurfaceEmpty) v = 0.f;
    else if (T >= tr) v = 1.f;
    else v = (float)exp(-((double)((unsigned long long)tr - (unsigned long long)T) / tau_ns));
    out[i] = v;
  }
}
void launch_recon_surface_decay(const long long *cells, const ReconViewRange *ranges, const long long *t_ref, size_t per_surface, int count,
                                double tau_ns, float *out, hipStream_t s) {
  if (per_surface == 0 || count <= 0) return;
  size_t blocks = (per_surface + 255) / 256;  // one cell per lane, up to 1024 workgroups to a surface (count <= 4096: grid.y)
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(recon_surface_decay_kernel, dim3((unsigned)blocks, (unsigned)count), dim3(256), 0, s, cells, ranges, t_ref, per_surface,
                     tau_ns, out);
}

// ---------------------------------------------------------------------------------------------- per-event export
// recon_warp     cmx_backend_recon_warp*: where every event of a slice lands.  The run structure of recon_votes over the slice's RAW
//                events (run = recon_run(B)): the first lanes evaluate the run's batch poses into LDS -- and, in the workgroup that
//                holds it, the pose of the call's lone trailing event at its own time into a slot of its own -- one barrier, then all
//                lanes walk the run, one event per lane and step.  load_bearing + be_warp_math<0> is the vote kernel's own
//                arithmetic, which hands out (px, py) beside the vote cell and the weights it takes from them: the same bits.
//                No atomics: per event one 16-byte (fp64) or 8-byte (fp32) pair store and one flag byte.  Flag bytes packed four
//                to a store were tried both ways -- a lane owning four consecutive events, and one event per lane with the
//                neighbours' bytes fetched by shuffles -- and neither beat the byte store (profiles/recon_warp_timing.txt).
typedef double warp_pair_f64 __attribute__((ext_vector_type(2)));  // (vector types: the struct double2 is stored member by member)
typedef float warp_pair_f32 __attribute__((ext_vector_type(2)));
template <bool F32>
__device__ __forceinline__ void warp_store_pair(void *out, size_t i, double px, double py, bool vec) {
  if (F32) {
    float *o = static_cast<float *>(out) + 2 * i;
    if (vec) *reinterpret_cast<warp_pair_f32 *>(o) = warp_pair_f32{(float)px, (float)py};
    else { o[0] = (float)px; o[1] = (float)py; }
  } else {
    double *o = static_cast<double *>(out) + 2 * i;
    if (vec) *reinterpret_cast<warp_pair_f64 *>(o) = warp_pair_f64{px, py};
    else { o[0] = px; o[1] = py; }
  }
}

template <int N, bool F32>
__global__ __launch_bounds__(kReconThreads) void recon_warp_kernel(const ReconWarpArgs g) {
  __shared__ double sh_R[(kReconMaxRun + 3) * 9];
  const ReconArgs &a = g.ev;
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * a.run;  // (the grid covers [0, n): e0 < n)
  const int e1 = (a.n - e0 > a.run) ? e0 + a.run : a.n;
  const int nbe = a.n - g.lone;       // events of the slice that batches hold
  const int eb1 = e1 < nbe ? e1 : nbe;
  const int b0 = e0 / a.B;
  int nbw = eb1 > e0 ? (eb1 - 1) / a.B - b0 + 1 : 0;
  if (nbw > kReconMaxRun + 2) nbw = kReconMaxRun + 2;  // (cannot happen with run = recon_run(B))
  const bool has_lone = g.lone && e1 == a.n;           // this workgroup holds the lone trailing event: pose slot nbw
  for (int j = tid; j < nbw + (has_lone ? 1 : 0); j += kReconThreads) {
    long long t = g.lone_t;
    if (j < nbw) t = a.batch_t[b0 + j < a.nb ? b0 + j : a.nb - 1];
    recon_pose<N>(a, t, sh_R + 9 * j);
  }
  __syncthreads();
  const bool vec = g.vec != 0;
  int cur = -1;
  double R[9];
  for (int i = e0 + tid; i < e1; i += kReconThreads) {
    const bool is_lone = i >= nbe;
    const int b = i / a.B;
    int j = b - b0;
    j = is_lone ? nbw : (j < nbw ? j : nbw - 1);
    if (j != cur) {
#pragma unroll
      for (int c = 0; c < 9; c++) R[c] = sh_R[9 * j + c];
      cur = j;
    }
    const uint32_t e = a.xy[i] & 0x7fffffffu;
    const int ex = e & 0xffff, ey = e >> 16;
    double v0, v1, v2, pxy[2];
    load_bearing(a.cam, ex, ey, v0, v1, v2);
    const BeWarp w = be_warp_math<0, true>(a.cam, e, b, v0, v1, v2, R, pxy);
    warp_store_pair<F32>(g.xy_out, (size_t)i, pxy[0], pxy[1], vec);
    if (g.flags_out)
      g.flags_out[i] = (unsigned char)(((!is_lone && (i - b * a.B) % g.rate == 0) ? CMX_WARP_SAMPLED : 0) | (w.ok ? CMX_WARP_INSIDE : 0));
  }
}

void launch_recon_warp(const ReconWarpArgs &g, hipStream_t s) {
  const ReconArgs &a = g.ev;
  if (a.n <= 0) return;
  const dim3 gr((unsigned)(((long long)a.n + a.run - 1) / a.run)), b(kReconThreads);  // (a.n <= 2^30 + 1: cmx_reconstruct.cpp)
  if (a.order == 2) {
    if (g.f32) hipLaunchKernelGGL((recon_warp_kernel<2, true>), gr, b, 0, s, g);
    else hipLaunchKernelGGL((recon_warp_kernel<2, false>), gr, b, 0, s, g);
  } else {
    if (g.f32) hipLaunchKernelGGL((recon_warp_kernel<4, true>), gr, b, 0, s, g);
    else hipLaunchKernelGGL((recon_warp_kernel<4, false>), gr, b, 0, s, g);
  }
}

// ---------------------------------------------------------------------------------------------- per-event support scores
// recon_smooth   cmx_backend_recon_score_open at sigma > 0: S = G plane, one workgroup per 64 x 16 tile.  The phases of
//                image_moments_kernel (cmx_kernels.hip) without its moments -- raw tile with a REFLECT_101 halo into LDS
//                (tile_load_composed), row pass (tile_blur_rows), column pass in registers (blur_col): the operation order of the
//                forward blur that cmx_imagephases.hpp states, so S holds the value the image pass forms.  A tile with no vote within
//                r pixels (launch_tile_flags; tile_in_reach) is left alone: the host has zeroed S in front of the launch.
// recon_score    cmx_backend_recon_score*: recon_warp_kernel's walk -- the run's batch poses into LDS, the lone trailing event's in a
//                slot of its own, one barrier, one event per lane and step with load_bearing + be_warp_math<0, true> -- and then,
//                for an event inside the plane, four loads from S around its vote cell and
//                    score = ((w00 S[yy][xx] + w01 S[yy][xx+1]) + w10 S[yy+1][xx]) + w11 S[yy+1][xx+1]
//                with the four weights of vote4_global, every product and every sum rounded on its own (no FMA): a host forms the
//                same bits from S and the exported (px, py).  One 4-byte store per event, the flag byte of the export when asked
//                for; no atomics, no LDS beyond the poses.  The loads are bound by memory latency, not by issue.
//                Leave-one-out: an event that voted (SAMPLED and INSIDE) put w_c into its four cells, which S hands back as
//                    self = sum_c sum_c' w_c w_c' Gx[x_c, x_c'] Gy[y_c, y_c'] = (wx^T Gx wx) (wy^T Gy wy),  wx = (1 - dx, dx), wy = (1 - dy, dy)
//                with Gx[a, b] the entry of the REFLECT_101 filter matrix (output a, input b): the tap g(a - b) plus the tap that
//                folds onto b at a border (score_fold: a panorama wider than 2r + 1 folds once).  The 2 x 2 blocks of an event
//                away from the borders are (g(0), g(1); g(1), g(0)): it never calls score_fold.  sigma 0: self is
//                ((w00^2 + w01^2) + w10^2) + w11^2.  One fp32 subtraction, no clamp: the plane is a sum of fp32 atomics, which
//                the event's own four adds need not have reached exactly, so a score of -1e-7 is what was measured.
template <int R>
__global__ __launch_bounds__(kImgThreads) void recon_smooth_kernel(const ImgArgs a, float *out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smooth_smem[];
  const int r = (R >= 0) ? R : a.r;
  float taps[2 * kMaxRadius + 1];  // (register copy, local: cmx_imagephases.hpp)
#pragma unroll
  for (int j = 0; j < 2 * kMaxRadius + 1; j++) taps[j] = (R < 0 || j <= 2 * R) ? a.taps[j] : 0.f;
  const int rawW = kTileX + 2 * r, rawH = kTileY + 2 * r;
  float *raw = reinterpret_cast<float *>(smooth_smem);
  float *rowb = raw + rawW * rawH;
  const int tx = threadIdx.x & 63, tq = threadIdx.x >> 6;  // output column, row quad
  const TileWork w = tile_begin<kTileX, kTileY, false>(a, (int)blockIdx.x);
  if (!tile_in_reach<kTileX, kTileY, false>(a, w, r)) return;  // (workgroup-uniform) nothing within reach: S stays zero
  tile_load_composed<kImgThreads>(a, 0.f, w.x0, w.y0, r, rawW, rawH, raw);
  __syncthreads();
  tile_blur_rows<R, kImgThreads>(taps, r, raw, rawW, rowb, kTileX, rawH);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const float s = blur_col<R>(taps, r, rowb + (tq * 4 + j + r) * kTileX + tx, kTileX);
    const int x = w.x0 + tx, y = w.y0 + tq * 4 + j;
    if (x < a.W && y < a.H) out[(size_t)y * a.W + x] = s;
  }
}
void launch_recon_smooth(const ImgArgs &a, float *out, hipStream_t s) {
  const int rawW = kTileX + 2 * a.r, rawH = kTileY + 2 * a.r;
  const size_t lds = sizeof(float) * ((size_t)rawW * rawH + (size_t)kTileX * rawH);
  if (a.r == 4) hipLaunchKernelGGL(recon_smooth_kernel<4>, dim3(a.nblk), dim3(kImgThreads), lds, s, a, out);
  else hipLaunchKernelGGL(recon_smooth_kernel<-1>, dim3(a.nblk), dim3(kImgThreads), lds, s, a, out);
}

// Gx[a, b] of the REFLECT_101 filter with these taps on a side of L > 2r + 1 cells, |a - b| <= 1 <= r: the tap of the offset, plus
// the tap whose input position folds onto b at the left border (-b) or at the right one (2 (L - 1) - b)
__device__ __forceinline__ float score_fold(const float *taps, int r, int L, int a, int b) {
  float g = taps[r + b - a];
  const int kl = r - a - b;                // a - r + kl == -b
  if (kl >= 0 && b > 0) g = __fadd_rn(g, taps[kl]);
  const int kr = 2 * (L - 1) - a - b + r;  // a - r + kr == 2 (L - 1) - b
  if (kr <= 2 * r && b < L - 1) g = __fadd_rn(g, taps[kr]);
  return g;
}
// w^T G w over the cells p, p + 1 of one axis, w = (1 - d, d)
__device__ __forceinline__ float score_self_axis(const float *taps, int r, int L, int p, float d) {
  const float w0 = 1.f - d, w1 = d;
  float g00 = taps[r], g01 = taps[r + 1], g10 = g01, g11 = g00;
  if (2 * p <= r || 2 * p + 2 >= 2 * (L - 1) - r) {  // a tap folds onto one of the two cells: a few events next to a border
    g00 = score_fold(taps, r, L, p, p);
    g01 = score_fold(taps, r, L, p, p + 1);
    g10 = score_fold(taps, r, L, p + 1, p);
    g11 = score_fold(taps, r, L, p + 1, p + 1);
  }
  const float a = __fmul_rn(__fmul_rn(w0, w0), g00), b = __fmul_rn(__fmul_rn(w0, w1), g01);
  const float c = __fmul_rn(__fmul_rn(w1, w0), g10), e = __fmul_rn(__fmul_rn(w1, w1), g11);
  return __fadd_rn(__fadd_rn(__fadd_rn(a, b), c), e);
}

template <int N>
__global__ __launch_bounds__(kReconThreads) void recon_score_kernel(const ReconScoreArgs g) {
  __shared__ double sh_R[(kReconMaxRun + 3) * 9];
  const ReconArgs &a = g.w.ev;
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * a.run;  // (the grid covers [0, n): e0 < n)
  const int e1 = (a.n - e0 > a.run) ? e0 + a.run : a.n;
  const int nbe = a.n - g.w.lone;     // events of the slice that batches hold
  const int eb1 = e1 < nbe ? e1 : nbe;
  const int b0 = e0 / a.B;
  int nbw = eb1 > e0 ? (eb1 - 1) / a.B - b0 + 1 : 0;
  if (nbw > kReconMaxRun + 2) nbw = kReconMaxRun + 2;  // (cannot happen with run = recon_run(B))
  const bool has_lone = g.w.lone && e1 == a.n;         // this workgroup holds the lone trailing event: pose slot nbw
  for (int j = tid; j < nbw + (has_lone ? 1 : 0); j += kReconThreads) {
    long long t = g.w.lone_t;
    if (j < nbw) t = a.batch_t[b0 + j < a.nb ? b0 + j : a.nb - 1];
    recon_pose<N>(a, t, sh_R + 9 * j);
  }
  __syncthreads();
  const int Wp = a.cam.Wp;
  int cur = -1;
  double R[9];
  for (int i = e0 + tid; i < e1; i += kReconThreads) {
    const bool is_lone = i >= nbe;
    const int b = i / a.B;
    int j = b - b0;
    j = is_lone ? nbw : (j < nbw ? j : nbw - 1);
    if (j != cur) {
#pragma unroll
      for (int c = 0; c < 9; c++) R[c] = sh_R[9 * j + c];
      cur = j;
    }
    const uint32_t e = a.xy[i] & 0x7fffffffu;
    const int ex = e & 0xffff, ey = e >> 16;
    double v0, v1, v2, pxy[2];
    load_bearing(a.cam, ex, ey, v0, v1, v2);
    const BeWarp w = be_warp_math<0, true>(a.cam, e, b, v0, v1, v2, R, pxy);
    const bool sampled = !is_lone && (i - b * a.B) % g.w.rate == 0;
    float score = 0.f;
    if (w.ok) {  // 1 <= xx < Wp - 2 && 1 <= yy < Hp - 2: the four cells are inside the plane
      const float *q = g.S + (size_t)w.yy * Wp + w.xx;
      const float s00 = q[0], s01 = q[1], s10 = q[Wp], s11 = q[Wp + 1];
      const float ux = 1.f - w.dx, uy = 1.f - w.dy;
      const float w00 = __fmul_rn(ux, uy), w01 = __fmul_rn(w.dx, uy), w10 = __fmul_rn(ux, w.dy), w11 = __fmul_rn(w.dx, w.dy);
      score = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w00, s00), __fmul_rn(w01, s01)), __fmul_rn(w10, s10)), __fmul_rn(w11, s11));
      if (g.loo && sampled) {  // the event voted: its own four adds, as S hands them back
        float self;
        if (g.r == 0)
          self = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w00, w00), __fmul_rn(w01, w01)), __fmul_rn(w10, w10)), __fmul_rn(w11, w11));
        else
          self = __fmul_rn(score_self_axis(g.taps, g.r, Wp, w.xx, w.dx), score_self_axis(g.taps, g.r, a.cam.Hp, w.yy, w.dy));
        score = __fsub_rn(score, self);
      }
    }
    g.score_out[i] = score;
    if (g.w.flags_out) g.w.flags_out[i] = (unsigned char)((sampled ? CMX_WARP_SAMPLED : 0) | (w.ok ? CMX_WARP_INSIDE : 0));
  }
}

void launch_recon_score(const ReconScoreArgs &g, hipStream_t s) {
  const ReconArgs &a = g.w.ev;
  if (a.n <= 0) return;
  const dim3 gr((unsigned)(((long long)a.n + a.run - 1) / a.run)), b(kReconThreads);  // (a.n <= 2^30 + 1: cmx_reconstruct.cpp)
  if (a.order == 2) hipLaunchKernelGGL(recon_score_kernel<2>, gr, b, 0, s, g);
  else hipLaunchKernelGGL(recon_score_kernel<4>, gr, b, 0, s, g);
}

// ---------------------------------------------------------------------------------------------- bound events
// recon_pose_table     the batch poses of an evaluation as a table in global memory: recon_pose<N> once per batch, the value the
//                        votes kernel above forms in LDS, bit for bit (72 B per batch)
// recon_votes_lds        the vote pass over events sorted by the destination tile of their vote (launch_count_sort /
//                        launch_build_chunks with poseR = the table): be_splat_lds_kernel's structure with ONE plane and the
//                        count of voting events.  load_bearing + be_warp_math<0> on the table's R is the arithmetic of
//                        recon_votes_kernel, so vote cell and weights are the same bits, and to_fix of them the same integers.
//                        Windows that hang over the plane's edge are safe for two reasons: a vote is only made when w.ok (all
//                        four cells inside the plane), and the flush only writes cells that are non-zero.
template <int N>
__global__ __launch_bounds__(256) void recon_pose_table_kernel(const ReconArgs a, PoseR *out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.nb) return;
  double R[9];
  recon_pose<N>(a, a.batch_t[b], R);
#pragma unroll
  for (int c = 0; c < 9; c++) out[b].R[c] = R[c];
}
void launch_recon_pose_table(const ReconArgs &a, PoseR *out, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {
  if (a.nb <= 0) return;
  const dim3 g((unsigned)((a.nb + 255) / 256)), b(256);
  auto k = a.order == 2 ? recon_pose_table_kernel<2> : recon_pose_table_kernel<4>;
  if (t0 || t1) hipExtLaunchKernelGGL(k, g, b, 0, s, t0, t1, 0, a, out);
  else hipLaunchKernelGGL(k, g, b, 0, s, a, out);
}

static_assert(kBinWindow * kBinWindow % kReconThreads == 0, "window cells per thread");
template <bool FIXED>
__global__ __launch_bounds__(kReconThreads) void recon_votes_lds_kernel(const ReconLdsArgs g) {
  __shared__ fix_t win[kBinWindow * kBinStride];
  __shared__ unsigned sh_inside, sh_fall;
  const BeSplatArgs &a = g.cam;
  const BinnedEvents &b = g.ev;
  // (the launch is sized by an upper bound of the table's length, and so is the table's allocation: be_splat_lds_kernel)
  const Chunk c = b.chunks[blockIdx.x];
  if ((int)blockIdx.x >= *b.nchunks_dev) return;
  const bool has_win = c.wx0 > -100000000;
  const int tid = threadIdx.x;
  if (tid == 0) { sh_inside = 0; sh_fall = 0; }
  if (has_win)
    for (int p = tid; p < kBinWindow * kBinStride; p += kReconThreads) win[p] = 0ull;
  __syncthreads();
  unsigned inside = 0, nfall = 0;
  constexpr int U = 2;  // events in flight per thread, as in be_splat_lds_kernel
  for (int j0 = c.beg + tid; j0 < c.end; j0 += kReconThreads * U) {
    uint32_t e[U], bi[U];
    bool act[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int j = j0 + u * kReconThreads;
      act[u] = j < c.end;
      e[u] = act[u] ? b.sxy[j] & 0x7fffffffu : 0u;
      bi[u] = act[u] ? b.sbatch[j] : 0u;
    }
    double v0[U], v1[U], v2[U], R[U][9];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const double *Rp = a.poseR[bi[u]].R;
#pragma unroll
      for (int k = 0; k < 9; k++) R[u][k] = Rp[k];
      load_bearing(a, (int)(e[u] & 0xffff), (int)(e[u] >> 16), v0[u], v1[u], v2[u]);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const BeWarp w = be_warp_math<0>(a, e[u], (int)bi[u], v0[u], v1[u], v2[u], R[u]);
      if (act[u] && w.ok) {  // 1 <= xx < Wp - 2 && 1 <= yy < Hp - 2: the four cells are inside the plane
        inside++;
        const int lx = w.xx - c.wx0, ly = w.yy - c.wy0;
        if (has_win && lx >= 0 && lx < kBinWindow - 1 && ly >= 0 && ly < kBinWindow - 1) {
          vote4_lds(win, lx, ly, w.dx, w.dy);
        } else {
          if (FIXED) vote4_global_fix(b.fixed, a.Wp, w.xx, w.yy, w.dx, w.dy);
          else vote4_global(g.plane, a.Wp, w.xx, w.yy, w.dx, w.dy);
          nfall++;
        }
      }
    }
  }
  // events that voted, and those of them on the global path: one wave reduction, one LDS add per wave, one atomic per workgroup
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    inside += __shfl_down(inside, off, 64);
    nfall += __shfl_down(nfall, off, 64);
  }
  if ((tid & 63) == 0) {
    if (inside) atomicAdd(&sh_inside, inside);
    if (nfall) atomicAdd(&sh_fall, nfall);
  }
  __syncthreads();
  if (tid == 0) {
    if (sh_inside) atomicAdd(g.n_inside, (unsigned long long)sh_inside);
    if (sh_fall) atomicAdd(b.fallback, sh_fall);
  }
  if (has_win) {
    constexpr int kCells = kBinWindow * kBinWindow / kReconThreads;  // (reads first, then the flush: be_splat_lds_kernel)
    fix_t cell[kCells];
#pragma unroll
    for (int k = 0; k < kCells; k++) {
      const int p = tid + kReconThreads * k, ly = p / kBinWindow, lx = p - ly * kBinWindow;
      cell[k] = win[ly * kBinStride + lx];
    }
#pragma unroll
    for (int k = 0; k < kCells; k++) {
      const fix_t v = cell[k];
      if (v != 0ull) {  // (a cell outside the plane never received a vote)
        const int p = tid + kReconThreads * k, ly = p / kBinWindow, lx = p - ly * kBinWindow;
        const size_t at = (size_t)(c.wy0 + ly) * a.Wp + (c.wx0 + lx);
        if (FIXED) atomicAdd(b.fixed + at, v);
        else atomic_add_f32(g.plane + at, (float)((double)v * kFixInv));
      }
    }
  }
}
void launch_recon_votes_lds(const ReconLdsArgs &g, hipStream_t s, hipEvent_t t0, hipEvent_t t1) {
  if (g.ev.nchunks <= 0) return;
  const dim3 gr((unsigned)g.ev.nchunks), b(kReconThreads);
  auto k = g.ev.fixed ? recon_votes_lds_kernel<true> : recon_votes_lds_kernel<false>;
  if (t0 || t1) hipExtLaunchKernelGGL(k, gr, b, 0, s, t0, t1, 0, g);
  else hipLaunchKernelGGL(k, gr, b, 0, s, g);
}

__global__ __launch_bounds__(256) void recon_fixed_to_float_kernel(const fix_t *fixed, float *plane, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    plane[i] = (float)((double)fixed[i] * kFixInv);
}
void launch_recon_fixed_to_float(const unsigned long long *fixed, float *plane, size_t n, hipStream_t s) {
  if (n == 0) return;
  size_t blocks = (n + 1023) / 1024;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(recon_fixed_to_float_kernel, dim3((unsigned)blocks), dim3(256), 0, s, fixed, plane, n);
}
// ... of cells that hold signed sums in two's complement (the voxel grids)
__global__ __launch_bounds__(256) void recon_fixed_to_float_signed_kernel(const fix_t *fixed, float *plane, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    plane[i] = (float)((double)(long long)fixed[i] * kFixInv);
}
void launch_recon_fixed_to_float_signed(const unsigned long long *fixed, float *plane, size_t n, hipStream_t s) {
  if (n == 0) return;
  size_t blocks = (n + 1023) / 1024;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(recon_fixed_to_float_signed_kernel, dim3((unsigned)blocks), dim3(256), 0, s, fixed, plane, n);
}

// ---------------------------------------------------------------------------------------------- contrast and gradient
// recon_gather   the SECOND pass over a slice's events (cmx_backend_recon_grad_add*), one launch per slice with the run structure of
//                recon_votes: batch poses into LDS, then all lanes walk the run's events with be_warp_math<2>, take the two
//                directional differences of Jt = G^T (G I) (and of G^T 1 next to the border) at the vote cell and reduce
//                V = (A, B) dpm_ddrot and U per batch -- the segmented shuffle of be_gather_kernel inside the wave, LDS across waves.
//                After the walk one lane per batch evaluates the batch's 3 x 3N spline Jacobian (So3Spline<N>::evaluate, the
//                arithmetic of spline_eval<N, true>, rounded to fp32 as Trajectory::evaluate hands it on), multiplies V and U
//                through it block by block and stores the 2 x 3N columns in LDS; then one lane per knot PARAMETER of the
//                workgroup's knot window sums the columns that fall on it in batch order -- no atomics inside the workgroup --
//                and adds its two sums to gsum: one global fp64 atomic per (workgroup, parameter touched), or, in
//                deterministic mode, one row per workgroup that recon_gather_rows adds workgroup by workgroup.
//                A batch whose segment lies outside the window (a run spanning more than kReconWindow knot intervals: a gap
//                in the recording) adds its columns to gsum itself, with atomics in both modes.
// recon_moments_finalize   contrast and mean from the image pass's moment rows, summed in index order by one workgroup

__device__ __forceinline__ int recon_segment(const ReconArgs &a, long long t_ns) {
  long long s = (t_ns - a.start_ns) / a.dt_ns;
  const long long s_max = (long long)a.K - a.order;
  return (int)(s < 0 ? 0 : (s > s_max ? s_max : s));  // (validated before the launch; the clamp keeps a bad one inside the tables)
}

// emit(k, J_k): the N blocks d_val_d_knot[s + k] of So3Spline<N>::evaluate at t_ns, in the order spline_eval<N, true> forms them
template <int N, typename Emit>
__device__ __forceinline__ void recon_pose_jac(const ReconArgs &a, long long t_ns, int s, Emit emit) {
  const long long st = t_ns - a.start_ns;
  const double u = (double)(st % a.dt_ns) / (double)a.dt_ns;
  double p[N], coeff[N];
  p[0] = 1.0;
  double ti = u;
#pragma unroll
  for (int j = 1; j < N; j++) { p[j] = 1.0 * ti; ti = ti * u; }
#pragma unroll
  for (int i = 0; i < N; i++) {
    double c = 0;
#pragma unroll
    for (int j = 0; j < N; j++) c += a.blend[i * N + j] * p[j];
    coeff[i] = c;
  }
  Quat res = a.knots[s];
  Mat3 Jh;
#pragma unroll
  for (int i = 0; i < 9; i++) Jh.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
  for (int i = 0; i < N - 1; i++) {
    const Quat p0 = a.knots[s + i];
    const double *d = a.delta + 3 * (size_t)(s + i);
    const double k = coeff[i + 1];
    const double delta[3] = {d[0], d[1], d[2]}, kdelta[3] = {d[0] * k, d[1] * k, d[2] * k};
    const Mat3 Jinv = left_jacobian_inv(delta);
    const Mat3 Jk = left_jacobian(kdelta);
    Mat3 Jb = Jh;
    Mat3 T = q_to_R(res);
#pragma unroll
    for (int c = 0; c < 9; c++) T.m[c] = k * T.m[c];
    T = m3_mul(T, Jk);
    T = m3_mul(T, Jinv);
    Jh = m3_mul(T, q_to_R(q_conj(p0)));
#pragma unroll
    for (int c = 0; c < 9; c++) Jb.m[c] -= Jh.m[c];
    emit(i, Jb);
    res = q_mul(res, so3_exp(kdelta[0], kdelta[1], kdelta[2]));
  }
  emit(N - 1, Jh);
}

__device__ __forceinline__ void recon_gsum_add(double *p, double v) {
  if (v != 0.0) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int kReconWinParams = 3 * kReconWindow;
static_assert(kReconWinParams <= 4 * kReconThreads, "four knot parameters per lane cover a workgroup's window");

template <int N, bool DET>
__global__ __launch_bounds__(kReconThreads) void recon_gather_kernel(const ReconGatherArgs g) {
  constexpr int kCols = 3 * N;
  constexpr int kChunk = 512 / N;  // batches per Jacobian round: their 2 x 3N columns are 24 KB of LDS
  constexpr int kPoseD = (kReconMaxRun + 2) * 9, kColD = kChunk * 2 * kCols;
  __shared__ double sh_u[kPoseD > kColD ? kPoseD : kColD];  // batch rotations during the walk, the rounds' columns after it
  __shared__ double sh_vu[(kReconMaxRun + 2) * 6];          // per batch: V (3), U (3)
  __shared__ int sh_off[kChunk];                             // per batch of a round: first parameter in the window, or none
  __shared__ int sh_s0;
  __shared__ unsigned sh_inside;
  const ReconArgs &a = g.ev;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e0 = blockIdx.x * a.run;  // (the grid covers [0, n): e0 < n)
  const int e1 = (a.n - e0 > a.run) ? e0 + a.run : a.n;
  const int b0 = e0 / a.per_batch;
  int nbw = (e1 - 1) / a.per_batch - b0 + 1;
  if (nbw > kReconMaxRun + 2) nbw = kReconMaxRun + 2;  // (cannot happen with run = recon_run(per_batch))
  if (tid == 0) { sh_inside = 0; sh_s0 = 0x7fffffff; }
  __syncthreads();
  for (int j = tid; j < nbw; j += kReconThreads) {
    const int b = b0 + j < a.nb ? b0 + j : a.nb - 1;
    const long long t = a.batch_t[b];
    recon_pose<N>(a, t, sh_u + 9 * j);
    atomicMin(&sh_s0, recon_segment(a, t));
  }
  for (int j = tid; j < nbw * 6; j += kReconThreads) sh_vu[j] = 0.0;
  __syncthreads();

  unsigned inside = 0;
  int cur = -1;
  double R[9];
  for (int base = e0; base < e1; base += kReconThreads) {  // (uniform trip count: the deterministic form has barriers)
    const int i = base + tid;
    double V0 = 0, V1 = 0, V2 = 0, U0 = 0, U1 = 0, U2 = 0;
    int j = -1;
    if (i < e1) {
      const int b = i / a.per_batch;
      j = b - b0;
      j = j < nbw ? j : nbw - 1;
      if (j != cur) {
#pragma unroll
        for (int c = 0; c < 9; c++) R[c] = sh_u[9 * j + c];
        cur = j;
      }
      const size_t src = a.stride ? (size_t)b * a.B + (size_t)(i - b * a.per_batch) * a.stride : (size_t)i;
      const uint32_t e = a.xy[src] & 0x7fffffffu;
      const int ex = e & 0xffff, ey = e >> 16;
      double v0, v1, v2;
      load_bearing(a.cam, ex, ey, v0, v1, v2);
      const BeWarp w = be_warp_math<2>(a.cam, e, b, v0, v1, v2, R);
      if (w.ok) {
        inside++;
        be_grad_vote(w, g.itilde, g.cx, g.cy, a.cam.Wp, a.cam.Hp, g.r, V0, V1, V2, U0, U1, U2);
      }
    }
    const bool any_u = run_sum(j, lane, V0, V1, V2, U0, U1, U2);
    const int jprev = __shfl_up(j, 1, 64);
    const bool head = j >= 0 && (lane == 0 || jprev != j);  // (one head per batch and wave: distinct LDS cells within a wave)
    double *dst = sh_vu + 6 * (j < 0 ? 0 : j);
    if (!DET) {
      if (head) {
        atomicAdd(dst + 0, V0); atomicAdd(dst + 1, V1); atomicAdd(dst + 2, V2);
        if (any_u) { atomicAdd(dst + 3, U0); atomicAdd(dst + 4, U1); atomicAdd(dst + 5, U2); }
      }
    } else {
      // deterministic mode: the waves add one after the other, walk step by walk step
      for (int w = 0; w < kReconThreads / 64; w++) {
        if (head && wave == w) {
          dst[0] += V0; dst[1] += V1; dst[2] += V2;
          dst[3] += U0; dst[4] += U1; dst[5] += U2;
        }
        __syncthreads();
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) inside += __shfl_down(inside, off, 64);
  if (lane == 0 && inside) atomicAdd(&sh_inside, inside);

  // ---- per batch: V, U through the batch's spline Jacobian; per knot parameter of the window: the sum over the batches on it
  const size_t P = 3 * (size_t)a.K;
  double acc1[4] = {0, 0, 0, 0}, acc2[4] = {0, 0, 0, 0};
  for (int c0 = 0; c0 < nbw; c0 += kChunk) {
    __syncthreads();  // the walk (or the previous round) is done with sh_u; sh_vu and sh_s0 are complete
    const int s0 = sh_s0;
    const int j = c0 + tid;
    if (tid < kChunk) {
      int off = -(1 << 28);
      if (j < nbw) {
        const double *vu = sh_vu + 6 * j;
        const double V0 = vu[0], V1 = vu[1], V2 = vu[2], U0 = vu[3], U1 = vu[4], U2 = vu[5];
        const bool has_u = U0 != 0.0 || U1 != 0.0 || U2 != 0.0;
        if (V0 != 0.0 || V1 != 0.0 || V2 != 0.0 || has_u) {
          const int b = b0 + j < a.nb ? b0 + j : a.nb - 1;
          const long long t = a.batch_t[b];
          const int s = recon_segment(a, t);
          const bool in_win = s - s0 + N <= kReconWindow;
          if (in_win) off = 3 * (s - s0);
          double *col = sh_u + (size_t)tid * 2 * kCols;
          recon_pose_jac<N>(a, t, s, [&](int k, const Mat3 &Jb) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
              const double j0 = (double)(float)Jb.m[c], j1 = (double)(float)Jb.m[3 + c], j2 = (double)(float)Jb.m[6 + c];
              const double c1 = V0 * j0 + V1 * j1 + V2 * j2;
              const double c2 = has_u ? U0 * j0 + U1 * j1 + U2 * j2 : 0.0;
              if (in_win) {
                col[3 * k + c] = c1;
                col[kCols + 3 * k + c] = c2;
              } else {
                const size_t q = 3 * (size_t)(s + k) + c;
                recon_gsum_add(g.gsum + q, c1);
                recon_gsum_add(g.gsum + P + q, c2);
              }
            }
          });
        }
      }
      sh_off[tid] = off;
    }
    __syncthreads();
    const int nj = nbw - c0 < kChunk ? nbw - c0 : kChunk;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int p = tid + q * kReconThreads;
      if (p < kReconWinParams) {
        for (int jj = 0; jj < nj; jj++) {
          const int d = p - sh_off[jj];
          if (d >= 0 && d < kCols) {
            acc1[q] += sh_u[(size_t)jj * 2 * kCols + d];
            acc2[q] += sh_u[(size_t)jj * 2 * kCols + kCols + d];
          }
        }
      }
    }
  }
  const int s0 = sh_s0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int p = tid + q * kReconThreads;
    if (p < kReconWinParams) {
      if (DET) {
        g.rows[((size_t)blockIdx.x * 2 + 0) * kReconWinParams + p] = acc1[q];
        g.rows[((size_t)blockIdx.x * 2 + 1) * kReconWinParams + p] = acc2[q];
      } else {
        const size_t kp = 3 * (size_t)s0 + p;
        if (kp < P) {
          recon_gsum_add(g.gsum + kp, acc1[q]);
          recon_gsum_add(g.gsum + P + kp, acc2[q]);
        }
      }
    }
  }
  if (tid == 0) {
    if (DET) g.row_win[blockIdx.x] = s0;
    if (sh_inside) atomicAdd(g.n_voted, (unsigned long long)sh_inside);  // (every wave's add precedes the rounds' first barrier)
  }
}

int recon_gather_blocks(const ReconArgs &a) {
  if (a.n <= 0 || a.nb <= 0) return 0;
  return (int)(((long long)a.n + a.run - 1) / a.run);  // (a.n <= 2^30: cmx_reconstruct.cpp)
}
void launch_recon_gather(const ReconGatherArgs &g, hipStream_t s) {
  const int blocks = recon_gather_blocks(g.ev);
  if (blocks <= 0) return;
  const dim3 gr((unsigned)blocks), b(kReconThreads);
  if (g.ev.order == 2) {
    if (g.rows) hipLaunchKernelGGL((recon_gather_kernel<2, true>), gr, b, 0, s, g);
    else hipLaunchKernelGGL((recon_gather_kernel<2, false>), gr, b, 0, s, g);
  } else {
    if (g.rows) hipLaunchKernelGGL((recon_gather_kernel<4, true>), gr, b, 0, s, g);
    else hipLaunchKernelGGL((recon_gather_kernel<4, false>), gr, b, 0, s, g);
  }
}

// deterministic mode: gsum[p] += sum over the launch's workgroups, in workgroup order, of the row entries that fall on parameter p.
// One lane per parameter of the knot range the rows cover (a slice of time-ordered events covers few knots); every lane walks
// all the rows' windows.
__global__ __launch_bounds__(256) void recon_gather_rows_kernel(const double *rows, const int *row_win, int blocks, double *gsum, int K) {
  __shared__ int sh_lo, sh_hi;
  if (threadIdx.x == 0) { sh_lo = 0x7fffffff; sh_hi = -1; }
  __syncthreads();
  int lo = 0x7fffffff, hi = -1;
  for (int w = threadIdx.x; w < blocks; w += 256) {
    const int s = row_win[w];
    lo = s < lo ? s : lo;
    hi = s > hi ? s : hi;
  }
  atomicMin(&sh_lo, lo);
  atomicMax(&sh_hi, hi);
  __syncthreads();
  const long long P = 3LL * K;
  const long long p_lo = 3LL * sh_lo;
  long long p_hi = 3LL * sh_hi + kReconWinParams;
  p_hi = p_hi < P ? p_hi : P;
  for (long long p = p_lo + (long long)blockIdx.x * 256 + threadIdx.x; p < p_hi; p += (long long)gridDim.x * 256) {
    double a1 = 0, a2 = 0;
    for (int w = 0; w < blocks; w++) {
      const long long d = p - 3LL * row_win[w];
      if (d >= 0 && d < kReconWinParams) {
        a1 += rows[((size_t)w * 2 + 0) * kReconWinParams + d];
        a2 += rows[((size_t)w * 2 + 1) * kReconWinParams + d];
      }
    }
    gsum[p] += a1;
    gsum[P + p] += a2;
  }
}
void launch_recon_gather_rows(const ReconGatherArgs &g, int blocks, hipStream_t s) {
  if (blocks <= 0 || !g.rows) return;
  hipLaunchKernelGGL(recon_gather_rows_kernel, dim3(64), dim3(256), 0, s, g.rows, g.row_win, blocks, g.gsum, g.ev.K);
}

__global__ __launch_bounds__(256) void recon_moments_finalize_kernel(const double *partials, int nblk, const unsigned *nvalid, double npix,
                                                                     int measure, double *out) {
  __shared__ double sh[2][256];
  const int n = nvalid ? (int)(*nvalid < (unsigned)nblk ? *nvalid : (unsigned)nblk) : nblk;
  double s0 = 0, s1 = 0;
  for (int i = threadIdx.x; i < n; i += 256) { s0 += partials[i]; s1 += partials[(size_t)nblk + i]; }
  sh[0][threadIdx.x] = s0;
  sh[1][threadIdx.x] = s1;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0, t1 = 0;
    for (int i = 0; i < 256; i++) { t0 += sh[0][i]; t1 += sh[1][i]; }
    double mu;
    out[0] = contrast_from_sums(t0, t1, npix, measure, &mu);
    out[1] = mu;
  }
}
void launch_recon_moments_finalize(const double *partials, int nblk, const unsigned *nvalid, double npix, int measure, double *out,
                                   hipStream_t s) {
  hipLaunchKernelGGL(recon_moments_finalize_kernel, dim3(1), dim3(256), 0, s, partials, nblk, nvalid, npix, measure, out);
}

// recon_grad_finalize   the gradient of the FREE parameters from the two sums, where the sums are: out[k - first] =
//                       (2/N)(S1[k] - mu S2[k]) for k in [first, P), the expression of cmx_backend_recon_grad_get term by term --
//                       the product, the difference, the doubling and the division are four roundings (the build does not contract,
//                       and the pragma says so for this function alone), so the same sums give the same bits as the host loop.  mu
//                       is the image pass's own (cm[1], what the host reads back as r->mu), zero for the mean-square measure.
//                       One lane per parameter; out is host memory mapped into the device, read by the solve after its one wait.
__global__ __launch_bounds__(256) void recon_grad_finalize_kernel(const double *gsum, const double *cm, long long P, long long first,
                                                                  double npix, int mean_square, double *out) {
#pragma clang fp contract(off)
  const long long k = first + (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= P) return;
  const double mu = mean_square ? 0.0 : cm[1];
  out[k - first] = 2.0 * (gsum[k] - (mu != 0.0 ? mu * gsum[P + k] : 0.0)) / npix;
}
void launch_recon_grad_finalize(const double *gsum, const double *cm, long long P, long long first, double npix, bool mean_square,
                                double *out, hipStream_t s) {
  if (first >= P) return;
  const long long blocks = (P - first + 255) / 256;  // (P <= 3 x 2^28)
  hipLaunchKernelGGL(recon_grad_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, s, gsum, cm, P, first, npix, mean_square ? 1 : 0, out);
}

}  // namespace cmx
