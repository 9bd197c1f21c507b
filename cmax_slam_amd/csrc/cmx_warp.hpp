// cmx_warp.hpp -- the per-event warps (device inline), shared by the splat, gather and binning kernels.
//   front end: first-order rotation + pinhole      (reference local_image_warped_events.cpp:94-145)
//   back end : R*b + equirectangular projection    (reference event_pano_warper.cpp:262-296,
//                                                   equirectangular_camera.h:18-45)
// fp64 geometry exactly as the reference (compile with -ffp-contract=off), fp32 bilinear offsets.
#pragma once
#include "cmx_internal.hpp"
#include "cmx_trig.hpp"

namespace cmx {

// fire-and-forget fp32 atomic add (global_atomic_add_f32, no return value); needs -munsafe-fp-atomics
__device__ __forceinline__ void atomic_add_f32(float *p, float v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// per-event front-end warp: fp64 first-order rotation + pinhole; fp32 bilinear offsets; optional 2x3 Jacobian rows
// bearing vector of sensor pixel (ex, ey): one 16-byte load when the table's z column is all ones
template <typename Args>
__device__ __forceinline__ void load_bearing(const Args &a, int ex, int ey, double &b0, double &b1, double &b2) {
  const size_t i = (size_t)ey * a.W + ex;
  if (a.lut2) {
    const double2 v = *reinterpret_cast<const double2 *>(a.lut2 + 2 * i);
    b0 = v.x; b1 = v.y; b2 = 1.0;
  } else {
    const double *l = a.lut + 3 * i;
    b0 = l[0]; b1 = l[1]; b2 = l[2];
  }
}

// device-driven solve: omega lives in device memory (uniform address: scalar loads)
__device__ __forceinline__ void fe_resolve_omega(FeSplatArgs &a) {
  if (a.w_dev) { a.wx = a.w_dev[0]; a.wy = a.w_dev[1]; a.wz = a.w_dev[2]; }
}

// device-driven solve: "finished" (FeSplatArgs::skip / ImgArgs::skip).  The word is set by the finalize step of an earlier launch --
// or by the HOST, on the null stream, in the middle of whatever launch is running when it takes a solve over (cmx_chain.cpp).  The
// decision must therefore be ONE read per workgroup: with one read per wave, some waves of a workgroup leave and the others stay, and
// the ones that stay find LDS the leavers were to clear (a splat window full of a previous workgroup's data, flushed as votes -- also
// to rows below the image's last one, i.e. into whatever allocation follows the plane).
__device__ __forceinline__ bool wg_stop_requested(const int *skip) {
  if (!skip) return false;  // (kernel argument: uniform)
  __shared__ int stop_sh;
  if (threadIdx.x == 0) stop_sh = __hip_atomic_load(skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __syncthreads();
  return stop_sh != 0;
}

struct FeWarp {
  int xx, yy;
  float dx, dy;
  bool ok;
  float r0[3], r1[3];
};

// the arithmetic of the front-end warp on an already-loaded bearing vector (lets callers batch the loads)
template <bool DERIV>
__device__ __forceinline__ FeWarp fe_warp_math(const FeSplatArgs &a, double px, double py, double pz, double dt) {
  FeWarp w;
  // p' = p + (omega*dt) x p   (first-order rotation)
  const double drx = a.wx * dt, dry = a.wy * dt, drz = a.wz * dt;
  const double rx = px + (dry * pz - drz * py);
  const double ry = py + (drz * px - drx * pz);
  const double rz = pz + (drx * py - dry * px);
  const double iz = 1.0 / rz;
  const double cxn = rx * iz, cyn = ry * iz;
  const double u = a.fx * cxn + a.cx;
  const double v = a.fy * cyn + a.cy;
  w.xx = (int)u;
  w.yy = (int)v;
  w.ok = (1 <= w.xx && w.xx < a.W - 2 && 1 <= w.yy && w.yy < a.H - 2);
  w.dx = (float)(u - w.xx);
  w.dy = (float)(v - w.yy);
  if (DERIV) {
    // J = diag(fx,fy) * J_proj(2x3) * [(-dt) p]_x   evaluated in the reference's operation order
    const double vx = (-dt) * px, vy = (-dt) * py, vz = (-dt) * pz;
    const double a02 = -cxn * iz, a12 = -cyn * iz;
    w.r0[0] = (float)(a.fx * (a02 * (-vy)));
    w.r0[1] = (float)(a.fx * (iz * (-vz) + a02 * vx));
    w.r0[2] = (float)(a.fx * (iz * vy));
    w.r1[0] = (float)(a.fy * (iz * vz + a12 * (-vy)));
    w.r1[1] = (float)(a.fy * (a12 * vx));
    w.r1[2] = (float)(a.fy * (iz * (-vx)));
  }
  return w;
}

template <bool DERIV>
__device__ __forceinline__ FeWarp fe_warp_core(const FeSplatArgs &a, uint32_t e, double dt) {
  const int ex = e & 0xffff, ey = (e >> 16) & 0x7fff;
  double b0, b1, b2;
  load_bearing(a, ex, ey, b0, b1, b2);
  return fe_warp_math<DERIV>(a, b0, b1, b2, dt);
}

template <bool DERIV>
__device__ __forceinline__ FeWarp fe_warp_event(const FeSplatArgs &a, int i) {
  return fe_warp_core<DERIV>(a, a.xy[i], a.batch_dt[i / a.per_batch]);
}

// per-event back-end warp: R*b, equirectangular projection (fp64), optional fp32 d(pixel)/d(rotation) 2x3
struct BeWarp {
  int xx, yy;
  float dx, dy;
  bool ok, is_old;
  int batch;
  float m[6];
};

// Back-end arithmetic and FMA contraction (round 5).  The library is built with -ffp-contract=off so that the FRONT end's fp64 warp is
// the reference's x86-64 (no FMA) arithmetic bit for bit.  The back end never was bit-identical -- its atan2 / asin are polynomial forms
// 1-3 ulp from glibc's (cmx_trig.hpp, themselves FMA chains) -- so the rotation R b, |R b|^2, the Newton steps and the pixel
// coordinate are contracted too: a difference of ~1e-16 relative in the ray, far below the trig forms' own, for 15 fp64 instructions
// less per event in kernels whose VALU issue is what binds them (profiles/r05_be_valu.txt).  Every back-end kernel (tile keys, splat,
// gather, reference-shaped splat) goes through these two functions, so they agree with one another on every vote cell bit for bit.
// Z1: the bearing's z is the constant 1 (tile- / time-ordered bearing streams hold (x, y) only): R[2], R[5], R[8] are added, not multiplied.
template <bool Z1>
__device__ __forceinline__ void be_rotate(const double *R, double b0, double b1, double b2, double &x, double &y, double &z) {
  // explicit FMAs in ONE association for both forms: with b2 == 1.0 the general form rounds R2 * b2 exactly, so
  // fma(R1, b1, R2 * b2) is the Z1 form's fma(R1, b1, R2) bit for bit -- whatever the compiler's contraction pass would have chosen
  if (Z1) {
    x = __builtin_fma(R[0], b0, __builtin_fma(R[1], b1, R[2]));
    y = __builtin_fma(R[3], b0, __builtin_fma(R[4], b1, R[5]));
    z = __builtin_fma(R[6], b0, __builtin_fma(R[7], b1, R[8]));
  } else {
    x = __builtin_fma(R[0], b0, __builtin_fma(R[1], b1, R[2] * b2));
    y = __builtin_fma(R[3], b0, __builtin_fma(R[4], b1, R[5] * b2));
    z = __builtin_fma(R[6], b0, __builtin_fma(R[7], b1, R[8] * b2));
  }
}

// the arithmetic of the back-end warp behind the rotation: e_ray_w = (x, y, z) = R * bearing.
// DERIV = 1: d(pixel)/d(rotation) with the projection Jacobian evaluated in fp64 and cast to fp32 entry by entry,
//            exactly the reference's Matx23f (equirectangular_camera.h:33-44) -- the derivative-plane (faithful) mode.
// DERIV = 2: the same five entries evaluated in fp32 from the fp64 ray (the reference multiplies them in fp32 anyway,
//            event_pano_warper.cpp:281-285); relative difference ~1e-7 per entry, saves five fp64 divisions and a
//            square root per event in the ALU-bound gather pass of the adjoint mode.
// EXPORT: the fp64 panorama coordinate (pxm, pym) the vote cell and the weights are taken from goes to pxy[0], pxy[1] as well -- the
//         per-event export (recon_warp_kernel, cmx_recon.hip) hands out the vote kernels' own values
template <int DERIV, bool EXPORT = false>
__device__ __forceinline__ BeWarp be_project(const BeSplatArgs &a, uint32_t e, int batch, double x, double y, double z,
                                             double *pxy = nullptr) {
  BeWarp w;
  w.is_old = (e >> 31) != 0;
  w.batch = batch;
  double pxm, pym, rho;
  {
#pragma clang fp contract(fast)  // (this block only: the Jacobian entries below keep the reference's operation-by-operation rounding)
    // equirectangular projection
    const double phi = lean_atan2(x, z);  // (cmx_trig.hpp: the two transcendental calls were three quarters of this function)
    // rho = |R b|: the reference's sqrt and division (y / rho) as ONE reciprocal square root -- v_rsq_f64 and two Newton steps
    // (~14 instructions against ~45; y * (1/rho) is within 2 ulp of y / rho, i.e. 1e-16 of the pixel coordinate)
    const double rho2 = x * x + (y * y + z * z);
    double inv_rho = __builtin_amdgcn_rsq(rho2);
    const double h = 0.5 * rho2;
    inv_rho = inv_rho * (1.5 - (h * inv_rho) * inv_rho);
    inv_rho = inv_rho * (1.5 - (h * inv_rho) * inv_rho);
    rho = rho2 * inv_rho;
    const double theta = lean_asin(y * inv_rho);
    pxm = a.cxp + phi * a.fx;
    pym = a.cyp + theta * a.fy;
  }
  w.xx = (int)pxm;
  w.yy = (int)pym;
  w.ok = (1 <= w.xx && w.xx < a.Wp - 2 && 1 <= w.yy && w.yy < a.Hp - 2);
  w.dx = (float)(pxm - w.xx);
  w.dy = (float)(pym - w.yy);
  if (EXPORT) { pxy[0] = pxm; pxy[1] = pym; }
  if (DERIV == 2) {
    const float xf = (float)x, yf = (float)y, zf = (float)z, rhof = (float)rho;
    const float fxf = (float)a.fx, fyf = (float)a.fy;
    // hardware reciprocal / reciprocal square root (1 ulp) instead of IEEE fp32 divisions and a square root: these five
    // entries are fp32 approximations of fp64 quantities to begin with, and four correctly rounded divisions were ~40 of
    // the gather's ~380 VALU instructions per event
    const float inv_rho = __builtin_amdgcn_rcpf(rhof), inv_z = __builtin_amdgcn_rcpf(zf);
    const float Ydivrho = yf * inv_rho, XdivZ = xf * inv_z;
    const float tmp1 = fxf * inv_z * __builtin_amdgcn_rcpf(1.f + XdivZ * XdivZ);
    const float tmp2 = -fyf * __builtin_amdgcn_rsqf(1.f - Ydivrho * Ydivrho);
    const float tmp3 = Ydivrho * inv_rho * inv_rho;
    const float d00 = tmp1, d02 = -tmp1 * XdivZ;
    const float d10 = tmp2 * tmp3 * xf, d11 = tmp2 * (tmp3 * yf - inv_rho), d12 = tmp2 * tmp3 * zf;
    w.m[0] = d02 * yf;
    w.m[1] = d00 * zf + d02 * (-xf);
    w.m[2] = d00 * (-yf);
    w.m[3] = d11 * (-zf) + d12 * yf;
    w.m[4] = d10 * zf + d12 * (-xf);
    w.m[5] = d10 * (-yf) + d11 * xf;
  } else if (DERIV == 1) {
    const double Ydivrho = y / rho;
    const double XdivZ = x / z;
    const double tmp1 = a.fx / ((1 + XdivZ * XdivZ) * z);
    const double tmp2 = -a.fy / sqrt(1 - Ydivrho * Ydivrho);
    const double tmp3 = Ydivrho / (rho * rho);
    const float d00 = (float)tmp1, d02 = (float)(-tmp1 * XdivZ);
    const float d10 = (float)(tmp2 * tmp3 * x), d11 = (float)(tmp2 * (tmp3 * y - 1 / rho)),
                d12 = (float)(tmp2 * tmp3 * z);
    const float rbx = (float)x, rby = (float)y, rbz = (float)z;
    // dpm_ddrot = dpm_drb(2x3) * (-[rb]x)(3x3), fp32 accumulation in k order (d01 == 0)
    w.m[0] = 0.f * (-rbz) + d02 * rby;
    w.m[1] = d00 * rbz + d02 * (-rbx);
    w.m[2] = d00 * (-rby) + 0.f * rbx;
    w.m[3] = d11 * (-rbz) + d12 * rby;
    w.m[4] = d10 * rbz + d12 * (-rbx);
    w.m[5] = d10 * (-rby) + d11 * rbx;
  }
  return w;
}

// rotation + projection on already-loaded operands: bearing (b0, b1, b2) and the batch rotation R[9]
template <int DERIV, bool EXPORT = false>
__device__ __forceinline__ BeWarp be_warp_math(const BeSplatArgs &a, uint32_t e, int batch, double b0, double b1,
                                              double b2, const double *R, double *pxy = nullptr) {
  double x, y, z;
  be_rotate<false>(R, b0, b1, b2, x, y, z);
  return be_project<DERIV, EXPORT>(a, e, batch, x, y, z, pxy);
}

template <int DERIV>
__device__ __forceinline__ BeWarp be_warp_core(const BeSplatArgs &a, uint32_t e, int batch) {
  const int ex = e & 0xffff, ey = (e >> 16) & 0x7fff;
  double b0, b1, b2;
  load_bearing(a, ex, ey, b0, b1, b2);
  double R[9];
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = a.poseR[batch].R[k];
  return be_warp_math<DERIV>(a, e, batch, b0, b1, b2, R);
}

template <int DERIV>
__device__ __forceinline__ BeWarp be_warp_event(const BeSplatArgs &a, int i) {
  return be_warp_core<DERIV>(a, a.xy[i], i / a.per_batch);
}

// ---- gather passes (adjoint gradient)
// d(contrast)/d(theta_k) = (2/N) sum_events [ r0_k * dJt/dx(at the event) + r1_k * dJt/dy ] where the
// bilinear-interpolation derivatives are exactly the signed-weight sums the reference scatters into its derivative
// images (local_image_warped_events.cpp:163-166, event_pano_warper.cpp:327-330).
__device__ __forceinline__ void bilinear_grad(const float *it, int W, int xx, int yy, float dx, float dy, float &A, float &B) {
  const float *q = it + (size_t)yy * W + xx;
  const float i00 = q[0], i01 = q[1], i10 = q[W], i11 = q[W + 1];
  A = (1.f - dy) * (i01 - i00) + dy * (i11 - i10);
  B = (1.f - dx) * (i10 - i00) + dx * (i11 - i01);
}

// the same two directional derivatives of the separable plane c(x,y) = cx[x]*cy[y] (= G^T 1); zero away from the border
__device__ __forceinline__ void border_grad(const float *cx, const float *cy, int W, int H, int r, int xx, int yy, float dx,
                                            float dy, float &A, float &B) {
  A = 0.f;
  B = 0.f;
  if (xx <= r || xx + 1 >= W - 1 - r || yy <= r || yy + 1 >= H - 1 - r) {
    const float c00 = cx[xx] * cy[yy], c01 = cx[xx + 1] * cy[yy], c10 = cx[xx] * cy[yy + 1], c11 = cx[xx + 1] * cy[yy + 1];
    A = (1.f - dy) * (c01 - c00) + dy * (c11 - c10);
    B = (1.f - dx) * (c10 - c00) + dx * (c11 - c01);
  }
}

// back end and reconstruction: per event V = (dItilde/dx, dItilde/dy) * dpm_ddrot (3-vector, BeWarp::m), and its border twin U
// against c = G^T 1 (zero but for votes within r of the panorama border).  fp64 sums of fp32 x fp32 products (exact in fp64).
// V and U are ASSIGNED the products' sums (one event per lane: be_gather_kernel, recon_gather_kernel).  be_gather4_kernel, four events
// per lane, accumulates with explicit FMAs under a contract pragma and keeps its own text (it measured 2 % longer through a helper).
__device__ __forceinline__ void be_grad_vote(const BeWarp &w, const float *itilde, const float *cx, const float *cy, int Wp, int Hp, int r,
                                             double &V0, double &V1, double &V2, double &U0, double &U1, double &U2) {
  float A, B;
  bilinear_grad(itilde, Wp, w.xx, w.yy, w.dx, w.dy, A, B);
  V0 = (double)A * (double)w.m[0] + (double)B * (double)w.m[3];
  V1 = (double)A * (double)w.m[1] + (double)B * (double)w.m[4];
  V2 = (double)A * (double)w.m[2] + (double)B * (double)w.m[5];
  float Ac, Bc;
  border_grad(cx, cy, Wp, Hp, r, w.xx, w.yy, w.dx, w.dy, Ac, Bc);
  if (Ac != 0.f || Bc != 0.f) {  // rare: votes within r of the panorama border
    U0 = (double)Ac * (double)w.m[0] + (double)Bc * (double)w.m[3];
    U1 = (double)Ac * (double)w.m[1] + (double)Bc * (double)w.m[4];
    U2 = (double)Ac * (double)w.m[2] + (double)Bc * (double)w.m[5];
  }
}

// segmented wave reduction of V and U over the runs of equal `run` (a batch index, -1 = no event; events of a run are adjacent
// lanes): afterwards the first lane of every run holds the run's sums.  Returns whether any lane of the wave had a non-zero U
// (wave-uniform; U's shuffles are skipped otherwise).
__device__ __forceinline__ bool run_sum(int run, int lane, double &V0, double &V1, double &V2, double &U0, double &U1, double &U2) {
  const bool any_u = __any(U0 != 0.0 || U1 != 0.0 || U2 != 0.0);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t0 = __shfl_down(V0, o, 64), t1 = __shfl_down(V1, o, 64), t2 = __shfl_down(V2, o, 64);
    const int ro = __shfl_down(run, o, 64);
    const bool same = lane + o < 64 && ro == run;
    if (same) { V0 += t0; V1 += t1; V2 += t2; }
    if (any_u) {  // wave-uniform
      const double u0 = __shfl_down(U0, o, 64), u1 = __shfl_down(U1, o, 64), u2 = __shfl_down(U2, o, 64);
      if (same) { U0 += u0; U1 += u1; U2 += u2; }
    }
  }
  return any_u;
}

}  // namespace cmx
