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
//   recon_fixed_to_float   deterministic mode: the 2^-30 fixed-point plane as fp32, leaving it as it is (accumulation goes on)
#include "../../include/cmax_hip.h"
#include "cmx_internal.hpp"
#include "cmx_warp.hpp"
#include "cmx_fixed.hpp"

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

template <int N, bool FIXED>
__global__ __launch_bounds__(kReconThreads) void recon_votes_kernel(const ReconArgs a) {
  __shared__ double sh_R[(kReconMaxRun + 2) * 9];
  __shared__ unsigned sh_inside;
  const int e0 = blockIdx.x * a.run;  // (the grid covers [0, n): e0 < n)
  const int e1 = (a.n - e0 > a.run) ? e0 + a.run : a.n;
  const int b0 = e0 / a.per_batch;
  int nbw = (e1 - 1) / a.per_batch - b0 + 1;
  if (nbw > kReconMaxRun + 2) nbw = kReconMaxRun + 2;  // (cannot happen with run = recon_run(per_batch))
  if (threadIdx.x == 0) sh_inside = 0;
  for (int j = threadIdx.x; j < nbw; j += kReconThreads) {
    const int b = b0 + j < a.nb ? b0 + j : a.nb - 1;
    recon_pose<N>(a, a.batch_t[b], sh_R + 9 * j);
  }
  __syncthreads();
  unsigned inside = 0;
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
    const uint32_t e = a.xy[src] & 0x7fffffffu;
    const int ex = e & 0xffff, ey = e >> 16;
    double v0, v1, v2;
    load_bearing(a.cam, ex, ey, v0, v1, v2);
    const BeWarp w = be_warp_math<0>(a.cam, e, b, v0, v1, v2, R);
    if (w.ok) {  // 1 <= xx < Wp - 2 && 1 <= yy < Hp - 2: the four cells are inside the plane
      if (FIXED) vote4_global_fix(a.fixed, a.cam.Wp, w.xx, w.yy, w.dx, w.dy);
      else vote4_global(a.plane, a.cam.Wp, w.xx, w.yy, w.dx, w.dy);
      inside++;
    }
  }
  // events that voted: one wave reduction, one atomic per workgroup
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) inside += __shfl_down(inside, off, 64);
  if ((threadIdx.x & 63) == 0 && inside) atomicAdd(&sh_inside, inside);
  __syncthreads();
  if (threadIdx.x == 0 && sh_inside) atomicAdd(a.n_inside, (unsigned long long)sh_inside);
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

}  // namespace cmx
