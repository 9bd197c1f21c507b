// cmx_display.hip -- the display path on the device: 8-bit tone maps of the local-IWE pair and of the panorama.
//
//   AngVelEstimator::publishEventImage     (src/frontend/ang_vel_estimator.cpp:203-233): hconcat of two blur-free IWEs,
//       normalize(0, 255, NORM_MINMAX, CV_32FC1), 255.f - x, convertTo(CV_8UC1)
//   PoseGraphOptimizer::publishEventImage  (src/backend/pose_graph_optimizer.cpp:378-413): normalize(0, 1, NORM_MINMAX),
//       pow(gamma), normalize(0, 255, NORM_MINMAX, CV_8UC1), 255 - x, GRAY2BGR, drawSensorFOV (event_pano_warper.cpp:56-79)
//
// Three kernels, queued back to back on the context's stream with no host round trip in between:
//   range_kernel      min / max of one or two planes: 16-byte loads, wave reduction, one pair of vector atomics per workgroup
//                     on order-preserving integer keys (exact: min / max do not depend on order)
//   tone_*_kernel     reads the two keys, forms the fp64 scale / fp32 (a, b) pair of cv::normalize itself, 4 pixels per lane
//                     in, one packed 32-bit store (mono) or three (BGR) out
//   fov_kernel        2 (W + H) threads, fp64 projection of the sensor border, byte stores into the BGR image
// and, for the signed polarity map of a reconstruction (no counterpart in the reference), range_signed_kernel / tone_signed_kernel:
// the same two steps over the difference of an ON and an OFF plane.
// cv::normalize(NORM_MINMAX) is  scale = (hi - lo > DBL_EPSILON) ? (dmax - dmin) / (hi - lo) : 0,  shift = dmin - lo * scale
// in fp64, then convertTo: fp32 multiply, fp32 add (the build has -ffp-contract=off), and for an 8-bit destination
// saturate_cast<uchar>(cvRound(.)) = round half to even.
#include <cfloat>

#include "cmx_internal.hpp"

namespace cmx {

constexpr int kDispThreads = 256;

// order-preserving key of an fp32 value: a < b  <=>  key(a) < key(b); -0 and +0 share the key of +0
__device__ __forceinline__ unsigned disp_key(float f) {
  unsigned u = __float_as_uint(f);
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float disp_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// range[0] = key(min), range[1] = ~key(max): both start at 0xffffffff (one memset) and both shrink under atomicMin
__device__ __forceinline__ void disp_range(const unsigned *range, float &lo, float &hi) {
  lo = disp_unkey(range[0]);
  hi = disp_unkey(~range[1]);
}

__device__ __forceinline__ void minmax4(const float4 v, float &lo, float &hi) {
  lo = fminf(lo, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
  hi = fmaxf(hi, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
}

// p1 may be null (one plane).  Both planes hold n floats and start on a 16-byte boundary.
__global__ __launch_bounds__(kDispThreads) void range_kernel(const float *__restrict__ p0, const float *__restrict__ p1, size_t n,
                                                             unsigned *range) {
  float lo = INFINITY, hi = -INFINITY;
  const size_t n4 = n / 4, stride = (size_t)gridDim.x * kDispThreads, t0 = (size_t)blockIdx.x * kDispThreads + threadIdx.x;
  const float4 *q0 = reinterpret_cast<const float4 *>(p0), *q1 = reinterpret_cast<const float4 *>(p1);
  for (size_t i = t0; i < n4; i += stride) {
    minmax4(q0[i], lo, hi);
    if (p1) minmax4(q1[i], lo, hi);
  }
  for (size_t i = 4 * n4 + t0; i < n; i += stride) {  // the last n % 4 pixels
    lo = fminf(lo, p0[i]); hi = fmaxf(hi, p0[i]);
    if (p1) { lo = fminf(lo, p1[i]); hi = fmaxf(hi, p1[i]); }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {  // wave = 64 lanes
    lo = fminf(lo, __shfl_xor(lo, off));
    hi = fmaxf(hi, __shfl_xor(hi, off));
  }
  __shared__ float s_lo[kDispThreads / 64], s_hi[kDispThreads / 64];
  if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kDispThreads / 64; w++) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
    if (lo <= hi) {  // (a workgroup that saw no pixel keeps the infinities to itself)
      atomicMin(&range[0], disp_key(lo));
      atomicMin(&range[1], ~disp_key(hi));
    }
  }
}

// cv::normalize's (scale, shift) for the destination range [0, dmax], as the fp32 pair convertTo multiplies and adds
__device__ __forceinline__ void norm_ab(float lo, float hi, double dmax, float &a, float &b) {
  const double d = (double)hi - (double)lo;
  const double scale = d > DBL_EPSILON ? dmax / d : 0.0;
  a = (float)scale;
  b = (float)(-(double)lo * scale);
}
// saturate_cast<uchar>(cvRound(x)): round half to even, then clamp
__device__ __forceinline__ unsigned sat_u8(float x) {
  const float r = fminf(fmaxf(rintf(x), 0.f), 255.f);
  return (unsigned)(int)r;
}

// ---- front end: S = [A | B], n = S * a + b, out = sat_u8(255.f - n); out is H x 2W
struct FeTone { float a, b; };
__device__ __forceinline__ unsigned fe_level(float s, FeTone t) { return sat_u8(255.f - (s * t.a + t.b)); }

__global__ __launch_bounds__(kDispThreads) void tone_pair_kernel(const float *__restrict__ A, const float *__restrict__ B, int W, int H,
                                                                 const unsigned *__restrict__ range, unsigned char *__restrict__ out) {
  float lo, hi;
  disp_range(range, lo, hi);
  FeTone t;
  norm_ab(lo, hi, 255.0, t.a, t.b);
  const size_t np = (size_t)W * H, stride = (size_t)gridDim.x * kDispThreads, t0 = (size_t)blockIdx.x * kDispThreads + threadIdx.x;
  if ((W & 3) == 0) {  // four pixels of one row of one half: 16 bytes in, one packed word out
    const size_t g_per_plane = np / 4, w4 = (size_t)W / 4;
    for (size_t g = t0; g < 2 * g_per_plane; g += stride) {
      const bool right = g >= g_per_plane;
      const size_t gi = right ? g - g_per_plane : g;
      const float4 v = reinterpret_cast<const float4 *>(right ? B : A)[gi];
      const size_t row = gi / w4, col4 = gi - row * w4;
      const unsigned word = fe_level(v.x, t) | (fe_level(v.y, t) << 8) | (fe_level(v.z, t) << 16) | (fe_level(v.w, t) << 24);
      reinterpret_cast<unsigned *>(out)[row * (2 * w4) + (right ? w4 : 0) + col4] = word;
    }
  } else {  // ragged width: a byte per pixel
    for (size_t i = t0; i < 2 * np; i += stride) {
      const bool right = i >= np;
      const size_t pi = right ? i - np : i;
      const size_t row = pi / (size_t)W, col = pi - row * (size_t)W;
      out[row * (2 * (size_t)W) + (right ? (size_t)W : 0) + col] = (unsigned char)fe_level((right ? B : A)[pi], t);
    }
  }
}

// ---- back end: v = IG * a + b in [0, 1], p = |v|^gamma, q = sat_u8(p * a2 + b2), out = 255 - q
struct BeTone { float a, b, a2, b2, gamma; int linear; };
// cv::pow takes |v| for a non-integer exponent; gamma == 1 is its copy path.  powf is the device library's (no fast-math form).
__device__ __forceinline__ float be_pow(float v, const BeTone &t) { return t.linear ? v : powf(fabsf(v), t.gamma); }
__device__ __forceinline__ unsigned be_level(float ig, const BeTone &t) {
  const float v = ig * t.a + t.b;
  return 255u - sat_u8(be_pow(v, t) * t.a2 + t.b2);
}
__device__ __forceinline__ BeTone be_tone(const unsigned *range, float gamma) {
  float lo, hi;
  disp_range(range, lo, hi);
  BeTone t;
  t.gamma = gamma;
  t.linear = gamma == 1.f;
  norm_ab(lo, hi, 1.0, t.a, t.b);
  // the extremes of p: pow is monotone on |v|, so they are the images of v's extremes, computed as the pixels themselves are
  const float p0 = be_pow(lo * t.a + t.b, t), p1 = be_pow(hi * t.a + t.b, t);
  norm_ab(fminf(p0, p1), fmaxf(p0, p1), 255.0, t.a2, t.b2);
  return t;
}

template <bool BGR>
__global__ __launch_bounds__(kDispThreads) void tone_map_kernel(const float *__restrict__ IG, size_t n, float gamma,
                                                                const unsigned *__restrict__ range, unsigned char *__restrict__ out) {
  const BeTone t = be_tone(range, gamma);
  const size_t n4 = n / 4, stride = (size_t)gridDim.x * kDispThreads, t0 = (size_t)blockIdx.x * kDispThreads + threadIdx.x;
  unsigned *out32 = reinterpret_cast<unsigned *>(out);
  for (size_t g = t0; g < n4; g += stride) {
    const float4 v = reinterpret_cast<const float4 *>(IG)[g];
    const unsigned l0 = be_level(v.x, t), l1 = be_level(v.y, t), l2 = be_level(v.z, t), l3 = be_level(v.w, t);
    if (BGR) {  // 12 bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
      out32[3 * g] = l0 * 0x010101u | (l1 << 24);
      out32[3 * g + 1] = l1 * 0x0101u | (l2 * 0x0101u << 16);
      out32[3 * g + 2] = l2 | (l3 * 0x010101u << 8);
    } else {
      out32[g] = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
    }
  }
  for (size_t i = 4 * n4 + t0; i < n; i += stride) {  // the last n % 4 pixels
    const unsigned char l = (unsigned char)be_level(IG[i], t);
    if (BGR) { out[3 * i] = l; out[3 * i + 1] = l; out[3 * i + 2] = l; }
    else out[i] = l;
  }
}

// ---- signed polarity map (cmx_backend_recon_pol_render): s = ON - OFF, m = max |s|, v = sign(s) (|s| / m)^gamma in fp32;
//   mono8: rint(127.5f + 127.5f v), so OFF is dark, ON is bright and no votes is 128;
//   bgr8 on white: a = rint(255 |v|), ON (B, G, R) = (255 - a, 255 - a, 255) red, OFF (255, 255 - a, 255 - a) blue.
// range_kernel's reduction over the difference of the two planes: its extremes give m = max(|lo|, |hi|) -- min / max are exact,
// so m does not depend on the order.  The planes are n floats each; 16-byte loads when both start on a 16-byte boundary.
__global__ __launch_bounds__(kDispThreads) void range_signed_kernel(const float *__restrict__ on, const float *__restrict__ off, size_t n,
                                                                    unsigned *range) {
  float lo = INFINITY, hi = -INFINITY;
  const bool vec = (((uintptr_t)on | (uintptr_t)off) & 15) == 0;
  const size_t n4 = vec ? n / 4 : 0, stride = (size_t)gridDim.x * kDispThreads, t0 = (size_t)blockIdx.x * kDispThreads + threadIdx.x;
  for (size_t i = t0; i < n4; i += stride) {
    const float4 a = reinterpret_cast<const float4 *>(on)[i], b = reinterpret_cast<const float4 *>(off)[i];
    minmax4(make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w), lo, hi);
  }
  for (size_t i = 4 * n4 + t0; i < n; i += stride) {
    const float s = on[i] - off[i];
    lo = fminf(lo, s); hi = fmaxf(hi, s);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // wave = 64 lanes
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  __shared__ float s_lo[kDispThreads / 64], s_hi[kDispThreads / 64];
  if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kDispThreads / 64; w++) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
    if (lo <= hi) {
      atomicMin(&range[0], disp_key(lo));
      atomicMin(&range[1], ~disp_key(hi));
    }
  }
}

struct PolTone { float m, gamma; int linear; };
__device__ __forceinline__ float pol_v(float s, const PolTone &t) {  // sign(s) (|s| / m)^gamma; m == 0: the neutral image
  const float q = t.m > 0.f ? fabsf(s) / t.m : 0.f;
  return copysignf(t.linear ? q : powf(q, t.gamma), s);
}
// the pixel as B | G << 8 | R << 16 (BGR), or its grey level
template <bool BGR>
__device__ __forceinline__ unsigned pol_level(float s, const PolTone &t) {
  const float v = pol_v(s, t);
  if (!BGR) return sat_u8(127.5f + 127.5f * v);
  const unsigned c = 255u - sat_u8(255.f * fabsf(v));
  return s > 0.f ? (c | (c << 8) | (255u << 16)) : (255u | (c << 8) | (c << 16));
}

template <bool BGR>
__global__ __launch_bounds__(kDispThreads) void tone_signed_kernel(const float *__restrict__ on, const float *__restrict__ off, size_t n,
                                                                   float gamma, const unsigned *__restrict__ range,
                                                                   unsigned char *__restrict__ out) {
  float lo, hi;
  disp_range(range, lo, hi);
  PolTone t;
  t.m = fmaxf(fabsf(lo), fabsf(hi));
  t.gamma = gamma;
  t.linear = gamma == 1.f;
  const bool vec = (((uintptr_t)on | (uintptr_t)off) & 15) == 0;
  const size_t n4 = vec ? n / 4 : 0, stride = (size_t)gridDim.x * kDispThreads, t0 = (size_t)blockIdx.x * kDispThreads + threadIdx.x;
  unsigned *out32 = reinterpret_cast<unsigned *>(out);
  for (size_t g = t0; g < n4; g += stride) {
    const float4 a = reinterpret_cast<const float4 *>(on)[g], b = reinterpret_cast<const float4 *>(off)[g];
    const unsigned l0 = pol_level<BGR>(a.x - b.x, t), l1 = pol_level<BGR>(a.y - b.y, t), l2 = pol_level<BGR>(a.z - b.z, t),
                   l3 = pol_level<BGR>(a.w - b.w, t);
    if (BGR) {  // 12 bytes: B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3
      out32[3 * g] = l0 | (l1 << 24);
      out32[3 * g + 1] = (l1 >> 8) | (l2 << 16);
      out32[3 * g + 2] = (l2 >> 16) | (l3 << 8);
    } else {
      out32[g] = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
    }
  }
  for (size_t i = 4 * n4 + t0; i < n; i += stride) {  // the last n % 4 pixels (all of them when a plane is off the 16-byte grid)
    const unsigned l = pol_level<BGR>(on[i] - off[i], t);
    if (BGR) { out[3 * i] = (unsigned char)l; out[3 * i + 1] = (unsigned char)(l >> 8); out[3 * i + 2] = (unsigned char)(l >> 16); }
    else out[i] = (unsigned char)l;
  }
}

// ---- EventWarper::drawSensorFOV: every sensor border pixel -> bearing (LUT) -> rotate -> equirectangular projection (as
// mark_mask_kernel, cmx_kernels.hip) -> cv::Point2d -> cv::Point rounds half to even -> (B, G, R) = (255, 0, 0).
// Points that fall outside the panorama are skipped (the reference writes them out of bounds).
struct FovArgs {
  double R[9];
  double fx, fy, cxp, cyp;
  int W, H, Wp, Hp;
  const double *lut;
};
__global__ __launch_bounds__(kDispThreads) void fov_kernel(FovArgs a, unsigned char *__restrict__ bgr) {
  const int t = blockIdx.x * kDispThreads + threadIdx.x;
  if (t >= 2 * (a.W + a.H)) return;
  int x, y;
  if (t < a.W) { x = t; y = 0; }
  else if (t < 2 * a.W) { x = t - a.W; y = a.H - 1; }
  else if (t < 2 * a.W + a.H) { x = 0; y = t - 2 * a.W; }
  else { x = a.W - 1; y = t - 2 * a.W - a.H; }
  const double *b = a.lut + 3 * ((size_t)y * a.W + x);
  const double rx = a.R[0] * b[0] + a.R[1] * b[1] + a.R[2] * b[2];
  const double ry = a.R[3] * b[0] + a.R[4] * b[1] + a.R[5] * b[2];
  const double rz = a.R[6] * b[0] + a.R[7] * b[1] + a.R[8] * b[2];
  const double phi = atan2(rx, rz);
  const double theta = asin(ry / sqrt(rx * rx + ry * ry + rz * rz));
  const double px = rint(a.cxp + phi * a.fx), py = rint(a.cyp + theta * a.fy);
  if (!(px >= 0.0 && px < (double)a.Wp && py >= 0.0 && py < (double)a.Hp)) return;  // (NaN fails every comparison)
  unsigned char *o = bgr + 3 * ((size_t)(int)py * a.Wp + (size_t)(int)px);
  o[0] = 255; o[1] = 0; o[2] = 0;
}

static int disp_blocks(size_t items) {
  const size_t b = (items + kDispThreads - 1) / kDispThreads;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

void launch_display_range(const float *p0, const float *p1, size_t n, unsigned *range, hipStream_t s) {
  hipLaunchKernelGGL(range_kernel, dim3(disp_blocks(n / 4 + 3)), dim3(kDispThreads), 0, s, p0, p1, n, range);
}
void launch_display_pair(const float *A, const float *B, int W, int H, const unsigned *range, unsigned char *out, hipStream_t s) {
  const size_t np = (size_t)W * H;
  hipLaunchKernelGGL(tone_pair_kernel, dim3(disp_blocks((W & 3) ? 2 * np : np / 2)), dim3(kDispThreads), 0, s, A, B, W, H, range, out);
}
void launch_display_map(const float *IG, size_t n, float gamma, bool bgr, const unsigned *range, unsigned char *out, hipStream_t s) {
  if (bgr) hipLaunchKernelGGL(tone_map_kernel<true>, dim3(disp_blocks(n / 4 + 3)), dim3(kDispThreads), 0, s, IG, n, gamma, range, out);
  else hipLaunchKernelGGL(tone_map_kernel<false>, dim3(disp_blocks(n / 4 + 3)), dim3(kDispThreads), 0, s, IG, n, gamma, range, out);
}
void launch_display_range_signed(const float *on, const float *off, size_t n, unsigned *range, hipStream_t s) {
  hipLaunchKernelGGL(range_signed_kernel, dim3(disp_blocks(n / 4 + 3)), dim3(kDispThreads), 0, s, on, off, n, range);
}
void launch_display_signed(const float *on, const float *off, size_t n, float gamma, bool bgr, const unsigned *range, unsigned char *out,
                           hipStream_t s) {
  if (bgr) hipLaunchKernelGGL(tone_signed_kernel<true>, dim3(disp_blocks(n / 4 + 3)), dim3(kDispThreads), 0, s, on, off, n, gamma, range, out);
  else hipLaunchKernelGGL(tone_signed_kernel<false>, dim3(disp_blocks(n / 4 + 3)), dim3(kDispThreads), 0, s, on, off, n, gamma, range, out);
}
void launch_display_fov(const BeSplatArgs &cam, const double R[9], int sensor_h, unsigned char *bgr, hipStream_t s) {
  FovArgs a;
  for (int i = 0; i < 9; i++) a.R[i] = R[i];
  a.fx = cam.fx; a.fy = cam.fy; a.cxp = cam.cxp; a.cyp = cam.cyp;
  a.W = cam.W; a.H = sensor_h; a.Wp = cam.Wp; a.Hp = cam.Hp;
  a.lut = cam.lut;
  hipLaunchKernelGGL(fov_kernel, dim3((2 * (a.W + a.H) + kDispThreads - 1) / kDispThreads), dim3(kDispThreads), 0, s, a, bgr);
}

}  // namespace cmx
