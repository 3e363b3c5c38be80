// fsg_sa.h -- what the slice-acquisition translation units share (fsg_slice_acq.hip: forward and adjoint;
// fsg_slice_acq_bwd.hip: backward of the forward; fsg_slice_acq_adjoint_bwd.hip: backward of the adjoint): the kernel-argument
// block, the LDS image of the PSF and of the per-axis tap products and its fill for any workgroup shape, the pixel-centre
// arithmetic, the trilinear cell (corner weights, the eight corners in their one order, sa_tri8, the PSF coordinate of a snapped
// voxel), the lever arms, the fixed-order workgroup fold sa_fold<TERMS, SLOTS> (the 12 transform sums of the two backward units,
// the 30 sums of fsg_svr.hip) with the size of its partials, the fixed-point quantisers with their finalising kernel, and the
// argument checks.  Internal linkage: each unit has its own copy.  The SA_* corner macros stay defined for the including unit.
#pragma once
#include "fsg_common.h"

namespace {

struct SaParams {
  const float* tr;          // (n, 3, 4)
  const float* psf;         // (pd, ph, pw)
  const uint8_t* vmask;     // (D,H,W) or null
  const uint8_t* smask;     // (n,h,w) or null
  const int32_t* sid;       // adjoint only: slice z of the launch reads slices[sid[z]] (null: identity)
  int D, H, W;
  int pd, ph, pw;
  int n, h, w;
  float res;
  // forward, linear PSF: which slices a launch takes (per workgroup, from the slice's own transform): 0 all, 1 those with
  // sa_direct_cost(T) <= fwd_thr (direct gathers), 2 the others (plate kernel)
  int fwd_select;
  float fwd_thr;
  float fwd_wy;  // weight of the slice x axis' y component in sa_direct_cost (10 for PSFs of 400 elements and more, 30 below)
};

constexpr int SA_TILE = 16;
constexpr int SA_MAX_PSF = 4096;  // elements (16 KB of LDS)
constexpr int SA_MAX_AXIS = 64;

// LDS image of the PSF and of the per-axis products of one slice's rotation with the tap offsets.
struct SaLds {
  float* psf;   // [pd*ph*pw]
  float* tx;    // [3][pw]   r_{a,0} * ix_p
  float* ty;    // [3][ph]   r_{a,1} * iy_p
  float* tz;    // [3][pd]   r_{a,2} * iz_p
};

__device__ __forceinline__ SaLds sa_lds_layout(float* base, const SaParams& P) {
  SaLds L;
  L.psf = base;
  L.tx = L.psf + P.pd * P.ph * P.pw;
  L.ty = L.tx + 3 * P.pw;
  L.tz = L.ty + 3 * P.ph;
  return L;
}

// tid: the thread's linear id in its workgroup of `nthreads` (16x16 blocks: sa_tid(); the 256-thread adjoint: threadIdx.x)
__device__ __forceinline__ int sa_tid() { return threadIdx.y * SA_TILE + threadIdx.x; }

__device__ __forceinline__ void sa_fill_lds(const SaLds& L, const SaParams& P, const float* __restrict__ T, int tid,
                                            int nthreads) {
  const int np = P.pd * P.ph * P.pw;
  for (int e = tid; e < np; e += nthreads) L.psf[e] = P.psf[e];
  // float * int in the reference == float * (float)int
  for (int e = tid; e < 3 * P.pw; e += nthreads) {
    const int a = e / P.pw, i = e - a * P.pw;
    L.tx[e] = T[a * 4 + 0] * (float)(i - P.pw / 2);
  }
  for (int e = tid; e < 3 * P.ph; e += nthreads) {
    const int a = e / P.ph, i = e - a * P.ph;
    L.ty[e] = T[a * 4 + 1] * (float)(i - P.ph / 2);
  }
  for (int e = tid; e < 3 * P.pd; e += nthreads) {
    const int a = e / P.pd, i = e - a * P.pd;
    L.tz[e] = T[a * 4 + 2] * (float)(i - P.pd / 2);
  }
}

// pixel position in slice axes, translation added (slice_acq_cuda_kernel.cu:46-48): formed in double (the literal `2.`
// promotes), kept in fp32.
__device__ __forceinline__ void sa_pixel(const SaParams& P, const float* __restrict__ T, int ix, int iy, float& _x, float& _y,
                                         float& _z) {
  _x = (float)(((double)ix - (P.w - 1) / 2.) * (double)P.res + (double)T[3]);
  _y = (float)(((double)iy - (P.h - 1) / 2.) * (double)P.res + (double)T[7]);
  _z = T[11];
}

// pixel centre in voxel coordinates (slice_acq_cuda_kernel.cu:46-56): the rotation in fp32, the volume centre added in double.
__device__ __forceinline__ void sa_centre(const SaParams& P, const float* __restrict__ T, int ix, int iy, float& xc,
                                          float& yc, float& zc) {
  float _x, _y, _z;
  sa_pixel(P, T, ix, iy, _x, _y, _z);
  xc = T[0] * _x + T[1] * _y + T[2] * _z;
  yc = T[4] * _x + T[5] * _y + T[6] * _z;
  zc = T[8] * _x + T[9] * _y + T[10] * _z;
  xc = (float)((double)xc + (P.W - 1) / 2.);
  yc = (float)((double)yc + (P.H - 1) / 2.);
  zc = (float)((double)zc + (P.D - 1) / 2.);
}

// (The triple loop over the PSF taps stays written out in every kernel: walked through one shared function template taking the
// body as a lambda, the compiler allocates registers differently -- other VGPR counts and occupancies in the adjoint and both
// backward kernels, scratch in the LDS adjoint -- and the forward's interp_psf kernel measured 0.5 % slower.)

// ---- the trilinear cell: corner weights, the eight corners in their fixed order, the PSF re-interpolated at a voxel ----
// Weight factors of corner (A,B,C) along x, y, z; `wx, wy, wz` are the caller's fractions.
#define SA_FX(A) ((A) ? wx : (1 - wx))
#define SA_FY(B) ((B) ? wy : (1 - wy))
#define SA_FZ(C) ((C) ? wz : (1 - wz))
// M(offset, A, B, C) for the eight corners of a cell with strides (1, SY, SZ).  The order is part of the bit contract with the
// float64 / fp32 restatements: every sum over the corners is written through this list.
#define SA_CORNERS8(M, SY, SZ) \
  M(0, 0, 0, 0) M(1, 1, 0, 0) M(SY, 0, 1, 0) M(SZ, 0, 0, 1) M(1 + SY, 1, 1, 0) M(1 + SZ, 1, 0, 1) M(SY + SZ, 0, 1, 1) \
  M(SY + SZ + 1, 1, 1, 1)
// One corner's term of d(trilinear sum)/d(position): the caller's `dx, dy, dz` gain -/+ (the other two factors) * t.
#define SA_DCORNER(TVAL, A, B, C)                                    \
  t = (TVAL);                                                        \
  dx = (A) ? dx + SA_FY(B) * SA_FZ(C) * t : dx - SA_FY(B) * SA_FZ(C) * t; \
  dy = (B) ? dy + SA_FX(A) * SA_FZ(C) * t : dy - SA_FX(A) * SA_FZ(C) * t; \
  dz = (C) ? dz + SA_FX(A) * SA_FY(B) * t : dz - SA_FX(A) * SA_FY(B) * t;

// trilinear sum over the cell at q (strides 1, sy, sz), eight terms added to 0 in the list's order
__device__ __forceinline__ float sa_tri8(const float* q, int sy, int sz, float wx, float wy, float wz) {
  float v = 0.f;
#define SA_TRI_TERM(OFF, A, B, C) v += SA_FX(A) * SA_FY(B) * SA_FZ(C) * q[(OFF)];
  SA_CORNERS8(SA_TRI_TERM, sy, sz)
#undef SA_TRI_TERM
  return v;
}

// interp_psf (slice_acq_cuda_kernel.cu:79-101): the PSF coordinate of the offset (dx, dy, dz) of a snapped voxel from the pixel
// centre (the literal `2.` promotes to double), and -- once the caller has found it inside the PSF grid -- its cell in the LDS
// image of the PSF with the fractions in it.  The range test stays with the caller because its two forms are NOT the same: the
// backward units accept (`!(xp >= 0 && ... && xp < pw - 1 ...)`: a NaN coordinate is outside), the forward and the adjoint reject
// (`xp < 0 || ...`: the reference's form, NaN goes on).
__device__ __forceinline__ void sa_psf_coord(const SaParams& P, const float* __restrict__ T, float dx, float dy, float dz,
                                             float& xp, float& yp, float& zp) {
  xp = (float)((double)(T[0] * dx + T[4] * dy + T[8] * dz) + (P.pw - 1) / 2.);
  yp = (float)((double)(T[1] * dx + T[5] * dy + T[9] * dz) + (P.ph - 1) / 2.);
  zp = (float)((double)(T[2] * dx + T[6] * dy + T[10] * dz) + (P.pd - 1) / 2.);
}
struct SaPsfCell {
  const float* q;
  float wx, wy, wz;
};
__device__ __forceinline__ SaPsfCell sa_psf_cell(const SaLds& L, const SaParams& P, float xp, float yp, float zp) {
  const float xf = floorf(xp), yf = floorf(yp), zf = floorf(zp);
  return SaPsfCell{L.psf + (int)zf * (P.pw * P.ph) + (int)yf * P.pw + (int)xf, xp - xf, yp - yf, zp - zf};
}

// ---- the lever arms of the 12 transform sums (both backward units) ----
// NEAREST_PSF: (dx, dy, dz) = d psf' / d (PSF coordinate) times the tap's factor; l = the rounded voxel relative to the volume
// centre.  The PSF moves under a fixed voxel: rotation columns gain d * l, the translation loses d.
__device__ __forceinline__ void sa_lever_nn(float (&g)[12], float dx, float dy, float dz, float lx, float ly, float lz) {
  g[0] += dx * lx; g[1] += dy * lx; g[2] += dz * lx;
  g[4] += dx * ly; g[5] += dy * ly; g[6] += dz * ly;
  g[8] += dx * lz; g[9] += dy * lz; g[10] += dz * lz;
  g[3] -= dx; g[7] -= dy; g[11] -= dz;
}
// LINEAR: (dx, dy, dz) = d (trilinear sample) / d (sampling position) times the tap's factor; l = pixel + translation + tap
// offset in slice axes.
__device__ __forceinline__ void sa_lever_lin(float (&g)[12], const float* __restrict__ T, float dx, float dy, float dz, float lx,
                                             float ly, float lz) {
  g[0] += dx * lx; g[1] += dx * ly; g[2] += dx * lz;
  g[4] += dy * lx; g[5] += dy * ly; g[6] += dy * lz;
  g[8] += dz * lx; g[9] += dz * ly; g[10] += dz * lz;
  g[3] += dx * T[0] + dy * T[4] + dz * T[8];
  g[7] += dx * T[1] + dy * T[5] + dz * T[9];
  g[11] += dx * T[2] + dy * T[6] + dz * T[10];
}

// ---- the fixed-order fold of a workgroup's per-lane sums: the 12 transform sums of the two backward units (sa_fold<12>), the
// 30 sums of fsg_svr.hip (sa_fold<30, 32>) ----
constexpr int SAB_WAVES = SA_TILE * SA_TILE / FSG_WAVE;

// Every thread of the 16x16 workgroup calls this with its TERMS sums (a pixel without a contribution carries zeros).  Lanes of a
// wave: a fixed shuffle tree; waves of the workgroup: LDS (`red`, [SAB_WAVES][SLOTS]), added in wave order; one partial of
// SLOTS floats per workgroup at ws[slice][tile].  All SLOTS are stored, zeros from TERMS on: the workspace needs no zeroing.
template <int TERMS, int SLOTS = TERMS>
__device__ __forceinline__ void sa_fold(const float (&v)[TERMS], float* red, float* __restrict__ ws, int in) {
  const int tid = sa_tid(), lane = tid & (FSG_WAVE - 1), wave = tid / FSG_WAVE;
#pragma unroll
  for (int k = 0; k < TERMS; ++k) {
    float s = v[k];
#pragma unroll
    for (int o = FSG_WAVE / 2; o > 0; o >>= 1) s += __shfl_down(s, o, FSG_WAVE);
    if (lane == 0) red[wave * SLOTS + k] = s;
  }
  __syncthreads();
  if (tid < SLOTS) {
    float s = 0.f;
    if (tid < TERMS) {
      s = red[tid];
#pragma unroll
      for (int q = 1; q < SAB_WAVES; ++q) s += red[q * SLOTS + tid];
    }
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x, tiles = (size_t)gridDim.x * gridDim.y;
    ws[((size_t)in * tiles + tile) * SLOTS + tid] = s;
  }
}

// grad_transforms[slice][k] = the slice's tile partials added in tile order.  One wave per slice, 12 lanes busy.
__global__ __launch_bounds__(FSG_WAVE) void sa_bwd_reduce_kernel(const float* __restrict__ ws, int tiles,
                                                                 float* __restrict__ gtr) {
  const int in = blockIdx.x, k = threadIdx.x;
  if (k >= 12) return;
  const float* p = ws + (size_t)in * tiles * 12 + k;
  float v = 0.f;
  for (int t = 0; t < tiles; ++t) v += p[(size_t)t * 12];
  gtr[in * 12 + k] = v;
}

// ---- fixed point: the quantisers, the two-limb integer and the finalising pass of the deterministic accumulators (SaSumFix of
// the adjoint in fsg_slice_acq.hip, SabSumFix of the backward's grad_vol in fsg_slice_acq_bwd.hip), moved here unaltered ----
typedef unsigned long long sa_u64;
constexpr int SA_DET_HI_BITS = FSG_SA_DET_FRAC_BITS - FSG_SA_DET_LIMB_BITS;  // the high limb counts 2^-32
constexpr double SA_DET_ONE = (double)(1ull << SA_DET_HI_BITS);
constexpr double SA_DET_LIMB = (double)(1ull << FSG_SA_DET_LIMB_BITS);

// round-half-even(c * k) for k a power of two: the product is exact in double, one rounding (the pixel weight's 2^-32)
__device__ __forceinline__ sa_u64 sa_fix(float c, double k) { return (sa_u64)__double2ll_rn((double)c * k); }
__device__ __forceinline__ float sa_unfix(long long q, float k) { return __ll2float_rn(q) * k; }
// Q = round-half-even(c * k * 2^LIMB) as hi * 2^LIMB + lo: d = c * k is exact in double, d - rint(d) is exact (at most 1/2,
// a multiple of ulp(d)), and rint(x + even integer) = rint(x) + that integer.  |lo| <= 2^(LIMB-1).  A contribution of
// 2^-(F-24) and more (d >= 2^-16: ulp(d) >= 2^-LIMB) enters exactly.
struct sa_q2 { sa_u64 hi, lo; };
__device__ __forceinline__ sa_q2 sa_fix2(float c, double k) {
  const double d = (double)c * k, h = rint(d);
  return sa_q2{(sa_u64)(long long)h, (sa_u64)__double2ll_rn((d - h) * SA_DET_LIMB)};
}
// a cell is {value hi, value lo [, weight hi, weight lo]}; zero limbs are not sent
__device__ __forceinline__ void sa_add2(sa_u64* cell, const sa_q2 q) {
  if (q.hi) atomicAdd(cell, q.hi);
  if (q.lo) atomicAdd(cell + 1, q.lo);
}
// hi * 2^LIMB + lo -> float32 with ONE rounding to nearest even, times 2^(ex - LIMB): the carry of lo goes into hi, the
// magnitude is cut to 63 bits that keep a sticky bit far below the rounding position, one conversion rounds, ldexp is exact
__device__ __forceinline__ float sa_unfix2(long long hi, long long lo, int ex) {
  constexpr long long ONE = 1ll << FSG_SA_DET_LIMB_BITS;
  const long long carry = lo >> FSG_SA_DET_LIMB_BITS;  // arithmetic shift: floor
  hi += carry;
  lo -= carry * ONE;  // 0 <= lo < ONE
  const bool neg = hi < 0;
  sa_u64 mh = (sa_u64)hi, ml = (sa_u64)lo;
  if (neg) {  // -(hi * ONE + lo) = (-hi - 1) * ONE + (ONE - lo) for lo > 0
    mh = lo ? (sa_u64)(-(hi + 1)) : (sa_u64)0 - (sa_u64)hi;
    ml = lo ? (sa_u64)(ONE - lo) : 0;
  }
  int t = FSG_SA_DET_LIMB_BITS;
  if (mh) t = min(t, __clzll((long long)mh) - 1);
  t = max(t, 0);  // (mh = 2^63, the overflowed sum of an out-of-range input: any value will do)
  const int down = FSG_SA_DET_LIMB_BITS - t;
  sa_u64 x = (mh << t) | (ml >> down);
  if (down && (ml & ((1ull << down) - 1))) x |= 1;  // sticky: x has its top bit at 62 here, rounding happens at bit 38
  const float f = ldexpf(__ll2float_rn((long long)x), down + ex - FSG_SA_DET_LIMB_BITS);
  return neg ? -f : f;
}

// accumulators -> float32, one rounding each (sa_unfix2); every voxel is written, an untouched accumulator gives +0.
// ex_v = log2(value_scale) - 32 (the backward: log2(grad_scale) - 32, limbs = 2), ex_w = -32: the exponent of the high limb's unit.
__global__ __launch_bounds__(256) void sa_det_finalize_kernel(const long long* __restrict__ acc, int limbs,
                                                              float* __restrict__ vol, float* __restrict__ vol_weight, int ex_v,
                                                              int ex_w, size_t n) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    const long long* cell = acc + e * limbs;
    vol[e] = sa_unfix2(cell[0], cell[1], ex_v);
    if (limbs == 4) vol_weight[e] = sa_unfix2(cell[2], cell[3], ex_w);
  }
}

inline int sa_check(const SaParams& P, size_t& lds, bool torch_mode) {
  if (!P.tr || !P.psf) return FSG_E_BADARG;
  if (P.D < 2 || P.H < 2 || P.W < 2 || P.n <= 0 || P.h <= 0 || P.w <= 0 || P.pd <= 0 || P.ph <= 0 || P.pw <= 0)
    return FSG_E_BADARG;
  if ((size_t)P.D * P.H * P.W > (size_t)0x7FFFFFFF || (size_t)P.n * P.h * P.w > (size_t)0x7FFFFFFF) return FSG_E_TOOBIG;
  if (P.pd > SA_MAX_AXIS || P.ph > SA_MAX_AXIS || P.pw > SA_MAX_AXIS || P.pd * P.ph * P.pw > SA_MAX_PSF) return FSG_E_TOOBIG;
  if (P.n > 65535) return FSG_E_TOOBIG;
  const size_t np = (size_t)P.pd * P.ph * P.pw;
  lds = torch_mode ? np * 4 * sizeof(float) : (np + 3 * (size_t)(P.pd + P.ph + P.pw)) * sizeof(float);
  return 0;
}

inline dim3 sa_grid(const SaParams& P) {
  return dim3((unsigned)((P.w + SA_TILE - 1) / SA_TILE), (unsigned)((P.h + SA_TILE - 1) / SA_TILE), (unsigned)P.n);
}

// bytes of the tile partials of sa_fold<TERMS, slots>, one partial of `slots` floats per workgroup of sa_grid (slots = 12: a
// multiple of 48, so what follows them in a workspace stays 16-byte aligned)
inline size_t sa_partial_bytes(int n, int h, int w, int slots) {
  const size_t tiles = (size_t)((w + SA_TILE - 1) / SA_TILE) * (size_t)((h + SA_TILE - 1) / SA_TILE);
  return (size_t)n * tiles * slots * sizeof(float);
}

}  // namespace
