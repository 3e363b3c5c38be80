// fsg_sa.h -- what the slice-acquisition translation units share (fsg_slice_acq.hip: forward and adjoint;
// fsg_slice_acq_bwd.hip: backward of the forward; fsg_slice_acq_adjoint_bwd.hip: backward of the adjoint): the kernel-argument
// block, the LDS image of the PSF and of the per-axis tap products, the pixel-centre arithmetic, the argument checks and the
// fixed-order reduction of the 12 transform sums.  Internal linkage: each unit has its own copy.
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

__device__ __forceinline__ void sa_fill_lds(const SaLds& L, const SaParams& P, const float* __restrict__ T) {
  const int tid = threadIdx.y * SA_TILE + threadIdx.x;
  const int np = P.pd * P.ph * P.pw;
  for (int e = tid; e < np; e += SA_TILE * SA_TILE) L.psf[e] = P.psf[e];
  // float * int in the reference == float * (float)int
  for (int e = tid; e < 3 * P.pw; e += SA_TILE * SA_TILE) {
    const int a = e / P.pw, i = e - a * P.pw;
    L.tx[e] = T[a * 4 + 0] * (float)(i - P.pw / 2);
  }
  for (int e = tid; e < 3 * P.ph; e += SA_TILE * SA_TILE) {
    const int a = e / P.ph, i = e - a * P.ph;
    L.ty[e] = T[a * 4 + 1] * (float)(i - P.ph / 2);
  }
  for (int e = tid; e < 3 * P.pd; e += SA_TILE * SA_TILE) {
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

// ---- the fixed-order reduction of the 12 transform sums, shared by the two backward units ----
constexpr int SAB_WAVES = SA_TILE * SA_TILE / FSG_WAVE;

// Every thread of the workgroup calls this with its 12 sums (a pixel without a contribution carries twelve zeros).  Lanes of a
// wave: a fixed shuffle tree; waves of the workgroup: LDS (`red`, [SAB_WAVES][12]), added in wave order; one 12-float partial
// per workgroup at ws[slice][tile].
__device__ __forceinline__ void sa_fold12(const float (&g)[12], float* red, float* __restrict__ ws, int in) {
  const int tid = threadIdx.y * SA_TILE + threadIdx.x, lane = tid & (FSG_WAVE - 1), wave = tid / FSG_WAVE;
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    float v = g[k];
#pragma unroll
    for (int o = FSG_WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, FSG_WAVE);
    if (lane == 0) red[wave * 12 + k] = v;
  }
  __syncthreads();
  if (tid < 12) {
    float v = red[tid];
#pragma unroll
    for (int q = 1; q < SAB_WAVES; ++q) v += red[q * 12 + tid];
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x, tiles = (size_t)gridDim.x * gridDim.y;
    ws[((size_t)in * tiles + tile) * 12 + tid] = v;
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

}  // namespace
