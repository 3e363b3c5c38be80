// fsg_transform_convert.hip -- pose conversions on the device: (n,6) axis-angle rows [rotation vector | translation] to and
// from (n,3,4) matrices [R | t], each with its backward (reference svort/transform/transform_convert_cuda_kernel.cu:14-440,
// the extension behind transform_convert.py:164-201).  DESIGN.md section 21.
//
// Shape of the work: none to speak of.  One thread owns one row, 256 threads per workgroup, ceil(n/256) workgroups, n a few
// hundred.  No LDS, no tuning, no variants: what these kernels buy is launches and host time (one launch where the torch
// formulation issues about forty), and a gradient of mat2axisangle that did not exist.
//
// Arithmetic: fp32 in the reference's operation order, contraction off (fsg_common.h).  What the reference's literals do,
// and what is made of it here:
//   - `theta2 > 1e-6`, `r22 < 1e-6`, `tmp > 1e-6` compare a float with a DOUBLE literal.  Written the same way here
//     (TC_EPS is a double).  float(1e-6) < 1e-6 and the next float up is > 1e-6, so no float lies between the two
//     thresholds: `v > 1e-6` agrees with the float32 compare `v > float(1e-6)` for every float32 v, and `v < 1e-6` with
//     `v < float(1e-6)` for every v but float(1e-6) itself (below the double, not below itself).  rigid.py, which compares
//     float32 tensors in float32, relies on that for `theta2 > 1e-6` and `r22 < 1e-6`.  It parts from these kernels in two
//     places: a matrix whose r22 is exactly float(1e-6) takes another (equally valid) quaternion formula there; and its
//     mat2axisangle tests the NORM, sqrt(tmp) > 1e-6, not tmp, as the reference's CPU path does, so for 1e-12 < tmp <= 1e-6
//     the host takes theta / si where these kernels and the reference's take 2 / w (the two agree to rounding there).
//   - `0.25 * s` is a double product of a float with a power of two: exact, so 0.25f * s here.
//   - `2.0 / w` is a double division rounded once to float.  A double holds 53 >= 2 * 24 + 2 bits, so rounding its quotient
//     to float gives the correctly rounded float32 quotient (double rounding is innocuous at that width): 2.0f / w here.  The
//     same holds for `... + 0.25 * dw` in the backward (an exact product, then one sum).
//   - in the small-norm branch of the mat2axisangle backward, `si + 1e-6`, the quotients by it and the products with them
//     are DOUBLE arithmetic, several operations deep, rounded to float only where the reference assigns to a float.  Kept in
//     double, operation for operation.  The branch is taken by a row in thousands and is not optimised.
// Branches:
//   axisangle2mat           theta2 > 1e-6: Rodrigues' formula on the unit axis; else the first-order matrix I + [a]x.
//   axisangle2mat backward  theta2 > 1e-6: the chain rule through c, s, the unit axis and theta; else the three antisymmetric
//                           differences of grad_mat.  A derivative in both branches.
//   mat2axisangle           quaternion (w,x,y,z) from one of four formulas: (1) r22 >= 1e-6 and r00 >= -r11, (2) r22 < 1e-6
//                           and r00 > r11, (3) r22 < 1e-6 and r00 <= r11, (4) r22 >= 1e-6 and r00 < -r11; the sign of all four
//                           flipped where w < 0; rotation vector = (x,y,z) * fac, fac = theta / si for tmp = x^2+y^2+z^2 > 1e-6
//                           with si = sqrt(tmp), theta = 2 atan2(si, w); else fac = 2 / w.
//   mat2axisangle backward  the chain rule through fac, the sign flip and the branch's formula, all 12 matrix entries treated
//                           as free variables.  QUIRK, kept: for tmp <= 1e-6 it is NOT the derivative of the forward.  The
//                           forward uses fac = 2 / w there; the backward differentiates as if fac depended on si, with si
//                           floored by 1e-6 in the quotients.  It is the reference's rule.  Everywhere else it is the derivative.
// No address depends on a value: every index is 12 * i + constant or 6 * i + constant with i < n.  A NaN or Inf in a row
// gives NaN or Inf in that row's output and touches nothing else.  NaN compares false, so a NaN takes the `else` branches;
// one of them does not read what was NaN: the small branch of the axisangle2mat backward takes its result from grad_mat
// alone, so a NaN POSE there leaves a finite row (a NaN in grad_mat does not).  The reference does the same.
// Every output element is written by every call: the translation column / elements are copied, and each of the four branches
// of the mat2axisangle backward stores all nine rotation entries of grad_mat.  Outputs need no zeroing.
// The reference's DEGREE macro is never defined there; there is no degree mode here.
// The overlap test in front of the launches is fsg_common.h's fsg_overlap.
#include "fsg_common.h"

namespace {

#define TC_EPS 1e-6  // double, as the reference's TRANSFORM_EPS
constexpr int TC_THREADS = 256;

__global__ __launch_bounds__(TC_THREADS) void tc_axisangle2mat_kernel(const float* __restrict__ ax, float* __restrict__ mat,
                                                                      int n) {
  const int i = blockIdx.x * TC_THREADS + threadIdx.x;
  if (i >= n) return;
  const float* a = ax + 6 * i;
  float* m = mat + 12 * i;
  float ux = a[0], uy = a[1], uz = a[2];
  const float theta2 = ux * ux + uy * uy + uz * uz;
  if (theta2 > TC_EPS) {
    const float theta = sqrtf(theta2);
    ux /= theta; uy /= theta; uz /= theta;
    const float s = sinf(theta), c = cosf(theta);
    const float o = 1.f - c;
    m[0] = c + ux * ux * o;
    m[1] = ux * uy * o - uz * s;
    m[2] = uy * s + ux * uz * o;
    m[4] = uz * s + ux * uy * o;
    m[5] = c + uy * uy * o;
    m[6] = -ux * s + uy * uz * o;
    m[8] = -uy * s + ux * uz * o;
    m[9] = ux * s + uy * uz * o;
    m[10] = c + uz * uz * o;
  } else {
    m[0] = 1.f; m[1] = -uz; m[2] = uy;
    m[4] = uz; m[5] = 1.f; m[6] = -ux;
    m[8] = -uy; m[9] = ux; m[10] = 1.f;
  }
  m[3] = a[3]; m[7] = a[4]; m[11] = a[5];
}

__global__ __launch_bounds__(TC_THREADS) void tc_axisangle2mat_backward_kernel(const float* __restrict__ gmat,
                                                                               const float* __restrict__ ax,
                                                                               float* __restrict__ gax, int n) {
  const int i = blockIdx.x * TC_THREADS + threadIdx.x;
  if (i >= n) return;
  const float* a = ax + 6 * i;
  const float* gm = gmat + 12 * i;
  float* ga = gax + 6 * i;
  float ux = a[0], uy = a[1], uz = a[2];
  const float theta2 = ux * ux + uy * uy + uz * uz;
  if (theta2 > TC_EPS) {
    const float theta = sqrtf(theta2);
    ux /= theta; uy /= theta; uz /= theta;
    const float s = sinf(theta), c = cosf(theta);
    const float o = 1.f - c;
    // sums of the gradient on the unit axis (dx, dy, dz), on sin (ds) and on cos (dc), entry by entry in row-major order
    float dx = 0.f, dy = 0.f, dz = 0.f, ds = 0.f, dc = 0.f, g;
    g = gm[0];  // c + ux ux o
    dc += (1.f - ux * ux) * g;
    dx += 2.f * o * ux * g;
    g = gm[1];  // ux uy o - uz s
    dc -= ux * uy * g; ds -= uz * g;
    dx += uy * o * g; dy += ux * o * g; dz -= s * g;
    g = gm[2];  // uy s + ux uz o
    dc -= ux * uz * g; ds += uy * g;
    dx += uz * o * g; dy += s * g; dz += ux * o * g;
    g = gm[4];  // uz s + ux uy o
    dc -= ux * uy * g; ds += uz * g;
    dx += uy * o * g; dy += ux * o * g; dz += s * g;
    g = gm[5];  // c + uy uy o
    dc += (1.f - uy * uy) * g;
    dy += 2.f * o * uy * g;
    g = gm[6];  // -ux s + uy uz o
    dc -= uy * uz * g; ds -= ux * g;
    dx -= s * g; dy += uz * o * g; dz += uy * o * g;
    g = gm[8];  // -uy s + ux uz o
    dc -= ux * uz * g; ds -= uy * g;
    dx += uz * o * g; dy -= s * g; dz += ux * o * g;
    g = gm[9];  // ux s + uy uz o
    dc -= uy * uz * g; ds += ux * g;
    dx += s * g; dy += uz * o * g; dz += uy * o * g;
    g = gm[10];  // c + uz uz o
    dc += (1.f - uz * uz) * g;
    dz += 2.f * o * uz * g;
    // theta moves along the axis; the unit axis moves across it, by (I - u u^T) / theta
    g = (c * ds - s * dc) * ux;
    g += (dx * (1.f - ux * ux) - (dy * uy + dz * uz) * ux) / theta;
    ga[0] = g;
    g = (c * ds - s * dc) * uy;
    g += (dy * (1.f - uy * uy) - (dx * ux + dz * uz) * uy) / theta;
    ga[1] = g;
    g = (c * ds - s * dc) * uz;
    g += (dz * (1.f - uz * uz) - (dx * ux + dy * uy) * uz) / theta;
    ga[2] = g;
  } else {
    ga[0] = gm[9] - gm[6];
    ga[1] = gm[2] - gm[8];
    ga[2] = gm[4] - gm[1];
  }
  ga[3] = gm[3]; ga[4] = gm[7]; ga[5] = gm[11];
}

// The quaternion of a rotation matrix by the reference's four formulas, before the sign flip; `s` is the branch's divisor.
// branch: 0..3 for (1)..(4) of the header comment.
struct TcQuat {
  float w, x, y, z, s;
  int branch;
};

__device__ __forceinline__ TcQuat tc_quat(const float* __restrict__ m) {
  const float r00 = m[0], r01 = m[1], r02 = m[2];
  const float r10 = m[4], r11 = m[5], r12 = m[6];
  const float r20 = m[8], r21 = m[9], r22 = m[10];
  const bool low22 = r22 < TC_EPS, d0_gt_d1 = r00 > r11, d0_lt_nd1 = r00 < -r11;
  TcQuat q;
  if (!low22 && !d0_lt_nd1) {
    q.branch = 0;
    q.s = 2.f * sqrtf(r00 + r11 + r22 + 1.f);
    q.w = 0.25f * q.s;
    q.x = (r21 - r12) / q.s;
    q.y = (r02 - r20) / q.s;
    q.z = (r10 - r01) / q.s;
  } else if (low22 && d0_gt_d1) {
    q.branch = 1;
    q.s = 2.f * sqrtf(r00 - r11 - r22 + 1.f);
    q.w = (r21 - r12) / q.s;
    q.x = 0.25f * q.s;
    q.y = (r01 + r10) / q.s;
    q.z = (r02 + r20) / q.s;
  } else if (low22 && !d0_gt_d1) {
    q.branch = 2;
    q.s = 2.f * sqrtf(r11 - r00 - r22 + 1.f);
    q.w = (r02 - r20) / q.s;
    q.x = (r01 + r10) / q.s;
    q.y = 0.25f * q.s;
    q.z = (r12 + r21) / q.s;
  } else {
    q.branch = 3;
    q.s = 2.f * sqrtf(r22 - r00 - r11 + 1.f);
    q.w = (r10 - r01) / q.s;
    q.x = (r02 + r20) / q.s;
    q.y = (r12 + r21) / q.s;
    q.z = 0.25f * q.s;
  }
  return q;
}

__global__ __launch_bounds__(TC_THREADS) void tc_mat2axisangle_kernel(const float* __restrict__ mat, float* __restrict__ ax,
                                                                      int n) {
  const int i = blockIdx.x * TC_THREADS + threadIdx.x;
  if (i >= n) return;
  const float* m = mat + 12 * i;
  float* a = ax + 6 * i;
  const TcQuat q = tc_quat(m);
  float w = q.w, x = q.x, y = q.y, z = q.z;
  if (w < 0.f) { w = -w; x = -x; y = -y; z = -z; }
  const float tmp = x * x + y * y + z * z;
  const float si = sqrtf(tmp);
  const float theta = 2.f * atan2f(si, w);
  const float fac = tmp > TC_EPS ? theta / si : 2.f / w;
  a[0] = x * fac; a[1] = y * fac; a[2] = z * fac;
  a[3] = m[3]; a[4] = m[7]; a[5] = m[11];
}

__global__ __launch_bounds__(TC_THREADS) void tc_mat2axisangle_backward_kernel(const float* __restrict__ mat,
                                                                               const float* __restrict__ gax,
                                                                               float* __restrict__ gmat, int n) {
  const int i = blockIdx.x * TC_THREADS + threadIdx.x;
  if (i >= n) return;
  const float* m = mat + 12 * i;
  const float* ga = gax + 6 * i;
  float* gm = gmat + 12 * i;
  const TcQuat q = tc_quat(m);
  float w = q.w, x = q.x, y = q.y, z = q.z;
  const float s = q.s;
  const bool neg_w = w < 0.f;
  if (neg_w) { w = -w; x = -x; y = -y; z = -z; }
  float tmp = x * x + y * y + z * z;
  const float si = sqrtf(tmp);
  const float theta = 2.f * atan2f(si, w);
  const float g0 = ga[0], g1 = ga[1], g2 = ga[2];

  // through fac = fac(w, si): every component starts from the gradient on fac
  float dw = x * g0 + y * g1 + z * g2;
  float dx = dw, dy = dw, dz = dw;
  float fac;
  if (tmp > TC_EPS) {
    fac = theta / si;
    tmp = 2.f / (w * w + si * si);
    dw *= -tmp;
    tmp = (w * tmp - fac) / si;
    dx *= tmp * (x / si);
    dy *= tmp * (y / si);
    dz *= tmp * (z / si);
  } else {
    // the quirk: not the derivative of fac = 2 / w; the 1e-6 floor and everything it touches in double, as the reference
    fac = 2.f / w;
    tmp = 2.f / (w * w + si * si);
    dw *= -tmp;
    const double sie = (double)si + TC_EPS;
    tmp = (float)((double)(w * tmp - fac) / sie);
    dx = (float)((double)dx * ((double)tmp * ((double)x / sie)));
    dy = (float)((double)dy * ((double)tmp * ((double)y / sie)));
    dz = (float)((double)dz * ((double)tmp * ((double)z / sie)));
  }
  dx += fac * g0;
  dy += fac * g1;
  dz += fac * g2;

  if (neg_w) {  // back to the branch's own signs
    w = -w; x = -x; y = -y; z = -z;
    dx = -dx; dy = -dy; dz = -dz; dw = -dw;
  }

  // through the branch's formula: six off-diagonal entries from the three quotients, the diagonal from s
  if (q.branch == 0) {
    gm[9] = dx / s; gm[6] = -dx / s;  // x = (r21 - r12) / s
    gm[2] = dy / s; gm[8] = -dy / s;  // y = (r02 - r20) / s
    gm[4] = dz / s; gm[1] = -dz / s;  // z = (r10 - r01) / s
    float ds = -(x * dx + y * dy + z * dz) / s + 0.25f * dw;
    ds *= 2.f / s;
    gm[0] = ds; gm[5] = ds; gm[10] = ds;
  } else if (q.branch == 1) {
    gm[9] = dw / s; gm[6] = -dw / s;  // w = (r21 - r12) / s
    gm[2] = dz / s; gm[8] = dz / s;   // z = (r02 + r20) / s
    gm[4] = dy / s; gm[1] = dy / s;   // y = (r01 + r10) / s
    float ds = -(w * dw + y * dy + z * dz) / s + 0.25f * dx;
    ds *= 2.f / s;
    gm[0] = ds; gm[5] = -ds; gm[10] = -ds;
  } else if (q.branch == 2) {
    gm[9] = dz / s; gm[6] = dz / s;   // z = (r12 + r21) / s
    gm[2] = dw / s; gm[8] = -dw / s;  // w = (r02 - r20) / s
    gm[4] = dx / s; gm[1] = dx / s;   // x = (r01 + r10) / s
    float ds = -(x * dx + w * dw + z * dz) / s + 0.25f * dy;
    ds *= 2.f / s;
    gm[0] = -ds; gm[5] = ds; gm[10] = -ds;
  } else {
    gm[9] = dy / s; gm[6] = dy / s;   // y = (r12 + r21) / s
    gm[2] = dx / s; gm[8] = dx / s;   // x = (r02 + r20) / s
    gm[4] = dw / s; gm[1] = -dw / s;  // w = (r10 - r01) / s
    float ds = -(x * dx + y * dy + w * dw) / s + 0.25f * dz;
    ds *= 2.f / s;
    gm[0] = -ds; gm[5] = -ds; gm[10] = ds;
  }
  gm[3] = ga[3]; gm[7] = ga[4]; gm[11] = ga[5];
}

// What the four entries refuse, before any launch: 0 = go on, 1 = nothing to do (n == 0), < 0 = the refusal.
// `out` has out_w floats per row, in0 / in1 (in1 may be absent: in1_w == 0) in0_w / in1_w; the kernels declare all three
// __restrict__, so an output that shares a byte with an input is refused.
int tc_check(const void* out, int out_w, const void* in0, int in0_w, const void* in1, int in1_w, int n) {
  if (n < 0) return FSG_E_BADARG;
  if (n == 0) return 1;
  if (!out || !in0 || (in1_w && !in1)) return FSG_E_BADARG;
  if ((long long)n * 12 > 0x7FFFFFFFLL) return FSG_E_TOOBIG;
  const size_t row = (size_t)n * sizeof(float);
  if (fsg_overlap(out, row * out_w, in0, row * in0_w)) return FSG_E_BADARG;
  if (in1_w && fsg_overlap(out, row * out_w, in1, row * in1_w)) return FSG_E_BADARG;
  return 0;
}

dim3 tc_grid(int n) { return dim3((unsigned)((n + TC_THREADS - 1) / TC_THREADS)); }

}  // namespace

extern "C" {

int fsg_axisangle2mat_f32(const float* axisangle, float* mat, int n, void* stream) {
  const int rc = tc_check(mat, 12, axisangle, 6, nullptr, 0, n);
  if (rc) return rc < 0 ? rc : 0;
  hipLaunchKernelGGL(tc_axisangle2mat_kernel, tc_grid(n), dim3(TC_THREADS), 0, fsg_stream(stream), axisangle, mat, n);
  FSG_RETURN_LAUNCH();
}

int fsg_axisangle2mat_backward_f32(const float* grad_mat, const float* axisangle, float* grad_axisangle, int n, void* stream) {
  const int rc = tc_check(grad_axisangle, 6, grad_mat, 12, axisangle, 6, n);
  if (rc) return rc < 0 ? rc : 0;
  hipLaunchKernelGGL(tc_axisangle2mat_backward_kernel, tc_grid(n), dim3(TC_THREADS), 0, fsg_stream(stream), grad_mat, axisangle,
                     grad_axisangle, n);
  FSG_RETURN_LAUNCH();
}

int fsg_mat2axisangle_f32(const float* mat, float* axisangle, int n, void* stream) {
  const int rc = tc_check(axisangle, 6, mat, 12, nullptr, 0, n);
  if (rc) return rc < 0 ? rc : 0;
  hipLaunchKernelGGL(tc_mat2axisangle_kernel, tc_grid(n), dim3(TC_THREADS), 0, fsg_stream(stream), mat, axisangle, n);
  FSG_RETURN_LAUNCH();
}

int fsg_mat2axisangle_backward_f32(const float* mat, const float* grad_axisangle, float* grad_mat, int n, void* stream) {
  const int rc = tc_check(grad_mat, 12, mat, 12, grad_axisangle, 6, n);
  if (rc) return rc < 0 ? rc : 0;
  hipLaunchKernelGGL(tc_mat2axisangle_backward_kernel, tc_grid(n), dim3(TC_THREADS), 0, fsg_stream(stream), mat, grad_axisangle,
                     grad_mat, n);
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
