// fsg_svr_group.hip -- what goes around fsg_svr_normal_f32 when several slices share ONE pose increment (DESIGN.md section 29;
// the contract is in include/fsg_hip.h, fsg_svr_compose_f32 / fsg_svr_group_reduce_f64).
//
//   fsg_svr_compose_f32        a slice's transform = its group's rigid motion of the volume frame applied to the slice's base
//                              transform, and the derivative of its 12 entries with respect to the GROUP's 6 parameters: the
//                              `jac` fsg_svr_normal_f32 takes.  Products and sums only: the pose arithmetic (sin, cos, the
//                              small-angle branch) stays in fsg_transform_convert.hip, whose outputs this unit combines.
//   fsg_svr_group_reduce_f64   a group's 32 sums = its members' rows of `stats` added in double in the listed order.
//
// The heavy pass is fsg_svr.hip's, untouched: a group's normal equations are the sum of its slices' rows once each slice's jac
// is taken with respect to the group's parameters.  Both kernels here are a few hundred threads of a handful of operations;
// they cost their launches.  No atomics, no LDS, no shuffles: every output element has one writer and a fixed operation order.
//
// A group id and a member index are DATA: each is range-tested in accepting form before it selects a row, and one that fails
// selects none.
#include "fsg_common.h"

namespace {

// (a0 * b0 + a1 * b1) + a2 * b2, one rounding per operation
__device__ __forceinline__ float dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
  return ((a0 * b0) + (a1 * b1)) + (a2 * b2);
}

// One thread per (slice, parameter a): column a of the slice's jac; the thread of a == 0 also stores the transform.
__global__ __launch_bounds__(256) void svr_compose_kernel(const float* __restrict__ gmat, const float* __restrict__ gjac,
                                                          const float* __restrict__ base, const int32_t* __restrict__ group,
                                                          float* __restrict__ tr, float* __restrict__ jac, int n, int G) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * 6) return;
  const int s = i / 6, a = i - 6 * s;
  const float* __restrict__ B = base + (size_t)s * 12;
  float* __restrict__ T = tr + (size_t)s * 12;
  float* __restrict__ J = jac + (size_t)s * 72;
  const int g = group[s];
  if (!(g >= 0 && g < G)) {  // fixed: the base row as it is, no derivative
    if (a == 0) {
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = B[k];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) J[k * 6 + a] = 0.f;
    return;
  }
  const float* __restrict__ Q = gmat + (size_t)g * 12;  // [Q | d], row-major 3 x 4
  const float* __restrict__ DQ = gjac + (size_t)g * 72;  // [entry][parameter]
  float R1[3][3];  // R' = Q R
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) R1[r][c] = dot3(Q[4 * r], B[c], Q[4 * r + 1], B[4 + c], Q[4 * r + 2], B[8 + c]);
  }
  const float d0 = Q[3], d1 = Q[7], d2 = Q[11];
  if (a == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) T[4 * r + c] = R1[r][c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) T[4 * c + 3] = B[4 * c + 3] + dot3(R1[0][c], d0, R1[1][c], d1, R1[2][c], d2);  // t + R'^T d
  }
  float dR[3][3];  // dQ_a R
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      dR[r][c] = dot3(DQ[(4 * r) * 6 + a], B[c], DQ[(4 * r + 1) * 6 + a], B[4 + c], DQ[(4 * r + 2) * 6 + a], B[8 + c]);
  }
  const float e0 = DQ[3 * 6 + a], e1 = DQ[7 * 6 + a], e2 = DQ[11 * 6 + a];  // dd_a
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) J[(4 * r + c) * 6 + a] = dR[r][c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)  // (dQ_a R)^T d + R'^T dd_a
    J[(4 * c + 3) * 6 + a] = dot3(dR[0][c], d0, dR[1][c], d1, dR[2][c], d2) + dot3(R1[0][c], e0, R1[1][c], e1, R1[2][c], e2);
}

// One thread per (group, slot).  A member index outside [0, n) and a range of `offsets` outside [0, n_members] add nothing.
__global__ __launch_bounds__(256) void svr_group_reduce_kernel(const double* __restrict__ stats, const int32_t* __restrict__ members,
                                                               const int32_t* __restrict__ offsets, double* __restrict__ gstats,
                                                               int n, int n_members, int G) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G * FSG_SVR_SLOTS) return;
  const int g = i / FSG_SVR_SLOTS, k = i - FSG_SVR_SLOTS * g;
  const int lo = offsets[g], hi = offsets[g + 1];
  double v = 0.0;
  if (lo >= 0 && hi <= n_members) {
    for (int j = lo; j < hi; ++j) {
      const int m = members[j];
      if (m >= 0 && m < n) v = v + stats[(size_t)m * FSG_SVR_SLOTS + k];
    }
  }
  gstats[i] = v;
}

}  // namespace

extern "C" {

int fsg_svr_compose_f32(const float* group_mat, const float* group_jac, const float* base, const int32_t* group, float* transforms,
                        float* jac, int n, int G, void* stream) {
  // every refusal comes before the first write
  if (!group_mat || !group_jac || !base || !group || !transforms || !jac) return FSG_E_BADARG;
  if (n <= 0 || G <= 0) return FSG_E_BADARG;
  if (n > 65535 || G > 65535) return FSG_E_TOOBIG;
  if (((uintptr_t)group_mat & 3) || ((uintptr_t)group_jac & 3) || ((uintptr_t)base & 3) || ((uintptr_t)group & 3) ||
      ((uintptr_t)transforms & 3) || ((uintptr_t)jac & 3))
    return FSG_E_ALIGN;
  const size_t tb = (size_t)n * 12 * sizeof(float), jb = (size_t)n * 72 * sizeof(float);
  const void* in[4] = {group_mat, group_jac, base, group};
  const size_t inb[4] = {(size_t)G * 12 * sizeof(float), (size_t)G * 72 * sizeof(float), tb, (size_t)n * sizeof(int32_t)};
  for (int k = 0; k < 4; ++k)
    if (fsg_overlap(transforms, tb, in[k], inb[k]) || fsg_overlap(jac, jb, in[k], inb[k])) return FSG_E_BADARG;
  if (fsg_overlap(transforms, tb, jac, jb)) return FSG_E_BADARG;
  hipLaunchKernelGGL(svr_compose_kernel, dim3((unsigned)((n * 6 + 255) / 256)), dim3(256), 0, fsg_stream(stream), group_mat,
                     group_jac, base, group, transforms, jac, n, G);
  FSG_RETURN_LAUNCH();
}

int fsg_svr_group_reduce_f64(const double* stats, const int32_t* members, const int32_t* offsets, double* gstats, int n,
                             int n_members, int G, void* stream) {
  if (!stats || !members || !offsets || !gstats) return FSG_E_BADARG;
  if (n <= 0 || G <= 0 || n_members <= 0) return FSG_E_BADARG;
  if (n > 65535 || G > 65535 || n_members > 65535) return FSG_E_TOOBIG;
  if (((uintptr_t)stats & 7) || ((uintptr_t)gstats & 7) || ((uintptr_t)members & 3) || ((uintptr_t)offsets & 3)) return FSG_E_ALIGN;
  const size_t gb = (size_t)G * FSG_SVR_SLOTS * sizeof(double);
  if (fsg_overlap(gstats, gb, stats, (size_t)n * FSG_SVR_SLOTS * sizeof(double)) ||
      fsg_overlap(gstats, gb, members, (size_t)n_members * sizeof(int32_t)) ||
      fsg_overlap(gstats, gb, offsets, ((size_t)G + 1) * sizeof(int32_t)))
    return FSG_E_BADARG;
  hipLaunchKernelGGL(svr_group_reduce_kernel, dim3((unsigned)((G * FSG_SVR_SLOTS + 255) / 256)), dim3(256), 0, fsg_stream(stream),
                     stats, members, offsets, gstats, n, n_members, G);
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
