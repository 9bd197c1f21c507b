// tilepass.hip -- the fused tile pass (cmax_slam_amd/csrc/cmx_tilepass.hpp) on its own: one 512-thread workgroup per 32 x 32 tile of a
// synthetic 640 x 480 plane, no chunk workgroups, no polling (wait_inputs is a barrier).  The one-output-per-thread pass and the
// register-blocked pass side by side: outputs compared (Jt up to the regrouped fp64 sums, moments to 1e-13), then the pass's phases from
// the wall-clock stamps it writes itself (FusedArgs::trace, 100 MHz), over all workgroups of 20 launches.  One pass per launch: a
// repeat loop around the pass changes its register allocation.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -munsafe-fp-atomics -I../../cmax_slam_amd/csrc -o tilepass tilepass.hip && ./tilepass
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cmx_tilepass.hpp"

using namespace cmx;

template <bool BLOCKED>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(6, 8))) void pass_kernel(FusedArgs f, const float *plane, int W, int H) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kTpLdsBytes];
  auto ready = [&]() -> bool {
    __syncthreads();
    if (threadIdx.x == 0) f.trace[8 * (size_t)blockIdx.x + 1] = wall_clock64();
    return true;
  };
  if (BLOCKED) fused_tile_pass_blocked<512, false>(f, plane, W, H, (int)blockIdx.x, lds, ready);
  else fused_tile_pass_legacy<512, false>(f, plane, W, H, (int)blockIdx.x, lds, ready);
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    f.trace[8 * (size_t)blockIdx.x + 2] = wall_clock64();
  }
}

#define CHECK(x)                                                                 \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) {                                                      \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                    \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

// banded M = G^T G of one axis, REFLECT_101 blur G of radius r (cmx_context.cpp upload_gt1)
static std::vector<float> banded(int L, int r, const float *taps) {
  const int bw = 4 * r + 1;
  std::vector<double> G((size_t)L * (2 * r + 1), 0.0);
  auto refl = [L](int p) { while (p < 0 || p >= L) p = p < 0 ? -p : 2 * (L - 1) - p; return p; };
  for (int p = 0; p < L; p++)
    for (int j = -r; j <= r; j++) {
      const int s = refl(p + j);
      if (s >= p - r && s <= p + r) G[(size_t)p * (2 * r + 1) + (s - (p - r))] += (double)taps[r + j];
    }
  std::vector<float> M((size_t)L * bw, 0.f);
  for (int q = 0; q < L; q++)
    for (int i = 0; i < bw; i++) {
      const int s = q - 2 * r + i;
      if (s < 0 || s >= L) continue;
      double acc = 0;
      for (int p = std::max(0, std::max(q, s) - r); p <= std::min(L - 1, std::min(q, s) + r); p++)
        acc += G[(size_t)p * (2 * r + 1) + (q - (p - r))] * G[(size_t)p * (2 * r + 1) + (s - (p - r))];
      M[(size_t)q * bw + i] = (float)acc;
    }
  return M;
}

static void pct(std::vector<double> v, const char *name) {
  std::sort(v.begin(), v.end());
  printf("    %-32s p10 %5.2f  p50 %5.2f  p90 %5.2f  max %5.2f us\n", name, v[v.size() / 10], v[v.size() / 2], v[9 * v.size() / 10], v.back());
}

template <bool BLOCKED>
static int run(const char *name, FusedArgs f, const float *plane, int W, int H, int ntiles, std::vector<float> &jt, std::vector<double> &part) {
  CHECK(hipMemset(f.jt, 0, (size_t)W * H * sizeof(float)));
  std::vector<unsigned long long> tr(8 * (size_t)ntiles);
  std::vector<double> ph[5];
  for (int trial = 0; trial < 21; trial++) {
    hipLaunchKernelGGL(pass_kernel<BLOCKED>, dim3(ntiles), dim3(512), 0, 0, f, plane, W, H);
    CHECK(hipDeviceSynchronize());
    if (trial == 0) continue;  // (cold code)
    CHECK(hipMemcpy(tr.data(), f.trace, tr.size() * 8, hipMemcpyDeviceToHost));
    for (int t = 0; t < ntiles; t++) {
      const unsigned long long *s = &tr[8 * (size_t)t];
      const int idx[6] = {1, 4, 5, 6, 2};
      for (int k = 0; k < 4; k++) ph[k].push_back((double)(s[idx[k + 1]] - s[idx[k]]) / 100.0);
      ph[4].push_back((double)(s[2] - s[1]) / 100.0);
    }
  }
  jt.resize((size_t)W * H);
  part.resize(2 * (size_t)ntiles);
  CHECK(hipMemcpy(jt.data(), f.jt, jt.size() * sizeof(float), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(part.data(), f.partials, part.size() * sizeof(double), hipMemcpyDeviceToHost));
  printf("%s, %d tiles x 20 launches:\n", name, ntiles);
  pct(ph[4], "tile pass");
  pct(ph[0], "  raw pixels loaded (sc1)");
  pct(ph[1], "  LDS write + row pass");
  pct(ph[2], "  column pass (Jt stores issued)");
  pct(ph[3], "  moments + stores drained");
  return 0;
}

int main() {
  const int W = 640, H = 480, R = 4, tiles_x = W / 32, tiles_y = H / 32, ntiles = tiles_x * tiles_y;
  float taps[9];
  {
    double k[9], s = 0;
    for (int j = -R; j <= R; j++) s += k[j + R] = std::exp(-0.5 * j * j);
    for (int j = 0; j < 9; j++) taps[j] = (float)(k[j] / s);
  }
  const std::vector<float> Mx = banded(W, R, taps), My = banded(H, R, taps);
  std::vector<float> plane((size_t)W * H);
  srand(7);
  for (auto &v : plane) v = (float)(rand() % 7 == 0 ? rand() % 9 : 0);
  FusedArgs f{};
  f.tiles_x = tiles_x;
  f.tiles_y = tiles_y;
  memcpy(f.taps, taps, sizeof(taps));
  for (int i = 0; i < 17; i++) f.M_in[i] = (double)Mx[(size_t)2 * R * 17 + i];
  f.M_in_ok = memcmp(&Mx[(size_t)2 * R * 17], &My[(size_t)2 * R * 17], 17 * sizeof(float)) == 0;
  float *dMx, *dMy, *dplane;
  CHECK(hipMalloc(&dMx, Mx.size() * sizeof(float)));
  CHECK(hipMalloc(&dMy, My.size() * sizeof(float)));
  CHECK(hipMalloc(&dplane, plane.size() * sizeof(float)));
  CHECK(hipMalloc(&f.jt, plane.size() * sizeof(float)));
  CHECK(hipMalloc(&f.partials, 2 * (size_t)ntiles * sizeof(double)));
  CHECK(hipMalloc(&f.trace, 8 * (size_t)ntiles * sizeof(unsigned long long)));
  CHECK(hipMemcpy(dMx, Mx.data(), Mx.size() * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dMy, My.data(), My.size() * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dplane, plane.data(), plane.size() * sizeof(float), hipMemcpyHostToDevice));
  f.Mx = dMx;
  f.My = dMy;
  printf("interior row shared by both axes: %d\n", f.M_in_ok);
  std::vector<float> jt0, jt1;
  std::vector<double> p0, p1;
  if (run<false>("one output per thread", f, dplane, W, H, ntiles, jt0, p0)) return 1;
  if (run<true>("register-blocked (L = 4)", f, dplane, W, H, ntiles, jt1, p1)) return 1;
  double dj = 0, sj = 0, dp = 0;
  size_t nbits = 0;
  for (size_t i = 0; i < jt0.size(); i++) {
    dj = std::max(dj, (double)std::fabs(jt0[i] - jt1[i]));
    sj = std::max(sj, (double)std::fabs(jt0[i]));
    nbits += memcmp(&jt0[i], &jt1[i], 4) != 0;
  }
  for (size_t i = 0; i < p0.size(); i++) dp = std::max(dp, std::fabs(p0[i] - p1[i]) / std::max(std::fabs(p0[i]), 1e-300));
  printf("Jt: max |difference| %.3e of max |Jt| %.3e, %zu of %zu values differ in their bits; moments: max relative difference %.3e\n", dj, sj,
         nbits, jt0.size(), dp);
  return dj <= 1e-6 * sj && dp < 1e-13 ? 0 : 2;
}
