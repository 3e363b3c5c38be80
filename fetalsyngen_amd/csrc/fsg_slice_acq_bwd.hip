// fsg_slice_acq_bwd.hip -- backward of the slice-acquisition FORWARD operator: gradients of `slices` with respect to the
// volume and to the (n,3,4) slice transforms (reference SliceAcqFunction.backward, slice_acq_cuda_kernel.cu:173-470,
// host side :993-1030).  The backward of the adjoint is fsg_slice_acq_adjoint_bwd.hip; the fold of the 12 transform sums (sa_fold<12>)
// and sa_bwd_reduce_kernel, which both units use, are in fsg_sa.h.
//
// The rule (include/fsg_hip.h), per pixel inside slices_mask with grad_slices != 0:
//   pass 1  weight = sum over the in-volume taps of the PSF value (FSG_SA_NEAREST_PSF: re-interpolated at the rounded voxel,
//           taps whose PSF coordinate falls outside the PSF grid skipped).  vol_mask plays NO part in it, unlike the forward's
//           own weight; weight == 0 ends the pixel (the forward tests weight > 0).  gs = grad_slices / weight.
//   pass 2  grad_vol += gs * psf * corner weight at the up-to-8 unmasked corners (LINEAR), gs * psf' at the rounded voxel if
//           unmasked (NEAREST_PSF); the 12 transform gradients from the derivative of the trilinear weights with respect to
//           the sampling position, the weight held constant.
//
// MI355X shape of the work: as the forward, one 256-thread workgroup = a 16x16 pixel tile of ONE slice, the PSF and the per-axis
// products r_ij * tap_offset in LDS.  grad_vol goes out with fp32 vector atomics (memory-side, not ordered), or, in the
// deterministic entry, as two 64-bit integer atomics per contribution into fixed-point accumulators (SabSumFix below).  The transform
// gradients never touch an atomic: each lane keeps its 12 sums in registers, a wave folds them with shuffles in a fixed order,
// the four waves meet in LDS and are added in wave order, the workgroup stores ONE 12-float partial at ws[slice][tile], and
// sa_bwd_reduce_kernel adds a slice's tiles in index order.  The result is a pure function of the inputs.
//
// Every range test is written in ACCEPTING form, `if (!(x >= 0 && x < hx ...)) continue;`: a NaN or Inf coordinate (non-finite
// transforms or res_slice) fails it and the tap is skipped, so no address is ever formed from a value that was not proven to be
// inside its array.
#include "fsg_sa.h"

namespace {

// The accumulator policies of grad_vol (as SaSumF32 / SaSumFix of the adjoint, fsg_slice_acq.hip).  A policy holds its own
// destination and states the one thing in which the two modes differ: what becomes of a contribution, the float32 value
// formed by the body.  Nothing else differs: pass 1, the weight, gs, the masks, the range tests and the 12 transform sums are
// the same instructions on the same values with either policy.
//   SabSumF32  unsafeAtomicAdd into grad_vol (fsg_slice_acq_backward_f32): the arithmetic as it was.
//   SabSumFix  the contribution quantised once to a multiple of 2^-72 * grad_scale (sa_fix2, k = 2^32 / grad_scale) and added
//              as two 64-bit limbs with integer atomics into 2 limbs per voxel (fsg_slice_acq_backward_det_f32); a limb that
//              is zero is not sent.  sa_det_finalize_kernel converts every accumulator with one rounding.
// No address depends on the contribution: a non-finite one gives an unspecified sum, never a fault.
// `add` takes the cell's voxel and the corner's offset apart and forms (base + iv) + off, the float kernel's own pointer
// arithmetic; with base + (iv + off), or with the body's SaParams taken by reference, four of the twelve float instantiations
// came out with other register counts (68 -> 72 VGPRs for one), so both are part of keeping the float path as it was.
struct SabSumF32 {
  float* __restrict__ gvol;
  __device__ __forceinline__ void add(int iv, int off, float c) const { unsafeAtomicAdd(gvol + iv + off, c); }
};
struct SabSumFix {
  sa_u64* __restrict__ acc;  // 2 limbs per voxel
  double k;
  __device__ __forceinline__ void add(int iv, int off, float c) const {
    sa_add2(acc + 2 * (size_t)iv + 2 * (size_t)off, sa_fix2(c, k));
  }
};

template <bool NN, bool VM, bool GV, bool GT, class Sum>
__device__ __forceinline__ void sa_backward_body(const SaParams P, const float* __restrict__ vol,
                                                 const float* __restrict__ gslices, float* __restrict__ ws, const Sum sum) {
  extern __shared__ float smem[];
  const int in = blockIdx.z;
  const float* __restrict__ T = P.tr + (size_t)in * 12;
  const SaLds L = sa_lds_layout(smem, P);
  float* red = L.tz + 3 * P.pd;  // [SAB_WAVES][12]
  sa_fill_lds(L, P, T, sa_tid(), SA_TILE * SA_TILE);
  __syncthreads();
  const int ix = blockIdx.x * SA_TILE + threadIdx.x, iy = blockIdx.y * SA_TILE + threadIdx.y;
  const bool inside = ix < P.w && iy < P.h;
  const size_t idx = ((size_t)in * P.h + (inside ? iy : 0)) * P.w + (inside ? ix : 0);
  float gs = inside && !(P.smask && !P.smask[idx]) ? gslices[idx] : 0.f;
  float g[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) g[k] = 0.f;

  // no thread leaves before the reduction: a pixel without a contribution carries twelve zeros into it
  if (gs != 0.f) {
    float _x, _y, _z, xc, yc, zc;
    sa_pixel(P, T, ix, iy, _x, _y, _z);
    sa_centre(P, T, ix, iy, xc, yc, zc);
    const int Sy = P.W, Sz = P.H * P.W;
    const int sy = P.pw, sz = P.pw * P.ph;
    const float hx = (float)(P.W - 1), hy = (float)(P.H - 1), hz = (float)(P.D - 1);
    const float qx = (float)(P.pw - 1), qy = (float)(P.ph - 1), qz = (float)(P.pd - 1);

    // ---- pass 1: the pixel's weight (vol_mask not consulted) ----
    float weight = 0.f;
    int ip = 0;
    for (int kz = 0; kz < P.pd; ++kz) {
      const float zx = L.tz[kz], zy = L.tz[P.pd + kz], zz = L.tz[2 * P.pd + kz];
      for (int ky = 0; ky < P.ph; ++ky) {
        const float yx = L.ty[ky], yy = L.ty[P.ph + ky], yz = L.ty[2 * P.ph + ky];
        for (int kx = 0; kx < P.pw; ++kx, ++ip) {
          float pv = L.psf[ip];
          if (pv == 0.f) continue;  // wave-uniform
          const float x = xc + L.tx[kx] + yx + zx;
          const float y = yc + L.tx[P.pw + kx] + yy + zy;
          const float z = zc + L.tx[2 * P.pw + kx] + yz + zz;
          if (!(x >= 0 && y >= 0 && z >= 0 && x < hx && y < hy && z < hz)) continue;
          if (NN) {
            float xp, yp, zp;
            sa_psf_coord(P, T, roundf(x) - xc, roundf(y) - yc, roundf(z) - zc, xp, yp, zp);
            if (!(xp >= 0 && yp >= 0 && zp >= 0 && xp < qx && yp < qy && zp < qz)) continue;
            const SaPsfCell c = sa_psf_cell(L, P, xp, yp, zp);
            pv = sa_tri8(c.q, sy, sz, c.wx, c.wy, c.wz);
          }
          weight += pv;
        }
      }
    }

    // ---- pass 2: scatter the volume gradient, gather the transform gradient ----
    if (weight != 0.f) {  // (`!= 0`, not the forward's `> 0`: the reference's own test; NaN goes on and stays a value)
      gs = gs / weight;
      ip = 0;
      for (int kz = 0; kz < P.pd; ++kz) {
        const float zx = L.tz[kz], zy = L.tz[P.pd + kz], zz = L.tz[2 * P.pd + kz];
        for (int ky = 0; ky < P.ph; ++ky) {
          const float yx = L.ty[ky], yy = L.ty[P.ph + ky], yz = L.ty[2 * P.ph + ky];
          for (int kx = 0; kx < P.pw; ++kx, ++ip) {
            const float pv = L.psf[ip];
            if (pv == 0.f) continue;
            const float x = xc + L.tx[kx] + yx + zx;
            const float y = yc + L.tx[P.pw + kx] + yy + zy;
            const float z = zc + L.tx[2 * P.pw + kx] + yz + zz;
            if (!(x >= 0 && y >= 0 && z >= 0 && x < hx && y < hy && z < hz)) continue;
            if (NN) {
              const float xr = roundf(x), yr = roundf(y), zr = roundf(z);
              float xp, yp, zp;
              sa_psf_coord(P, T, xr - xc, yr - yc, zr - zc, xp, yp, zp);
              if (!(xp >= 0 && yp >= 0 && zp >= 0 && xp < qx && yp < qy && zp < qz)) continue;
              const SaPsfCell c = sa_psf_cell(L, P, xp, yp, zp);
              const float* q = c.q;
              const float wx = c.wx, wy = c.wy, wz = c.wz;
              const int iv = (int)zr * Sz + (int)yr * Sy + (int)xr;
              if (VM && !P.vmask[iv]) continue;
              if (GV) sum.add(iv, 0, sa_tri8(q, sy, sz, wx, wy, wz) * gs);
              if (GT) {
                // d psf' / d (PSF coordinate), times gs * vol: the rounded voxel is fixed, the PSF moves under it
                float dx = 0.f, dy = 0.f, dz = 0.f, t;
#define SAB_PSF_CORNER(OFF, A, B, C) SA_DCORNER(q[(OFF)], A, B, C)
                SA_CORNERS8(SAB_PSF_CORNER, sy, sz)
#undef SAB_PSF_CORNER
                t = gs * vol[iv];
                dx *= t; dy *= t; dz *= t;
                // lever arm: the rounded voxel relative to the volume centre (exact in fp32: half-integers below 2^23)
                sa_lever_nn(g, dx, dy, dz, xr - hx * 0.5f, yr - hy * 0.5f, zr - hz * 0.5f);
              }
            } else {
              const float xf = floorf(x), yf = floorf(y), zf = floorf(z);
              const float wx = x - xf, wy = y - yf, wz = z - zf;
              const int iv = (int)zf * Sz + (int)yf * Sy + (int)xf;
              const float pg = pv * gs;
              if (GV) {
#define SAB_VOL_CORNER(OFF, A, B, C) \
  if (!VM || P.vmask[iv + (OFF)]) sum.add(iv, (OFF), SA_FX(A) * SA_FY(B) * SA_FZ(C) * pg);
                SA_CORNERS8(SAB_VOL_CORNER, Sy, Sz)
#undef SAB_VOL_CORNER
              }
              if (GT) {
                // d (trilinear sample) / d (sampling position), times gs * psf, over the unmasked corners
                float dx = 0.f, dy = 0.f, dz = 0.f, t;
#define SAB_LIN_CORNER(OFF, A, B, C) \
  if (!VM || P.vmask[iv + (OFF)]) { SA_DCORNER(pg * vol[iv + (OFF)], A, B, C) }
                SA_CORNERS8(SAB_LIN_CORNER, Sy, Sz)
#undef SAB_LIN_CORNER
                // lever arm: pixel + translation + tap offset, in slice axes
                sa_lever_lin(g, T, dx, dy, dz, _x + (float)(kx - P.pw / 2), _y + (float)(ky - P.ph / 2),
                             _z + (float)(kz - P.pd / 2));
              }
            }
          }
        }
      }
    }
  }

  // the fold of fsg_sa.h: shuffle tree per wave, waves in order through LDS, one partial per workgroup
  if (GT) sa_fold<12>(g, red, ws, in);
}

// The kernels: the body with each accumulator.  A kernel takes its destination as a __restrict__ argument of its own and builds
// the policy from it (a pointer that arrives inside a by-value struct loses `noalias`: DESIGN section 17).  The fixed-point
// siblings exist only where grad_vol is requested; without it the float kernel <.., false, true> serves both entries.
template <bool NN, bool VM, bool GV, bool GT>
__global__ __launch_bounds__(SA_TILE* SA_TILE) void sa_backward_kernel(SaParams P, const float* __restrict__ vol,
                                                                       const float* __restrict__ gslices,
                                                                       float* __restrict__ gvol, float* __restrict__ ws) {
  sa_backward_body<NN, VM, GV, GT>(P, vol, gslices, ws, SabSumF32{gvol});
}
template <bool NN, bool VM, bool GT>
__global__ __launch_bounds__(SA_TILE* SA_TILE) void sa_backward_det_kernel(SaParams P, const float* __restrict__ vol,
                                                                           const float* __restrict__ gslices,
                                                                           sa_u64* __restrict__ acc, double k,
                                                                           float* __restrict__ ws) {
  sa_backward_body<NN, VM, true, GT>(P, vol, gslices, ws, SabSumFix{acc, k});
}

// acc != null: grad_vol in fixed point (the caller passes it only when grad_vol is requested)
template <bool NN, bool VM>
void sa_backward_launch(const SaParams& P, const float* vol, const float* gslices, float* gvol, sa_u64* acc, double k, float* ws,
                        bool gt, dim3 grid, size_t lds, hipStream_t st) {
  const dim3 block(SA_TILE, SA_TILE);
  if (acc && gt) hipLaunchKernelGGL((sa_backward_det_kernel<NN, VM, true>), grid, block, lds, st, P, vol, gslices, acc, k, ws);
  else if (acc) hipLaunchKernelGGL((sa_backward_det_kernel<NN, VM, false>), grid, block, lds, st, P, vol, gslices, acc, k, ws);
  else if (gvol && gt) hipLaunchKernelGGL((sa_backward_kernel<NN, VM, true, true>), grid, block, lds, st, P, vol, gslices, gvol, ws);
  else if (gvol) hipLaunchKernelGGL((sa_backward_kernel<NN, VM, true, false>), grid, block, lds, st, P, vol, gslices, gvol, ws);
  else hipLaunchKernelGGL((sa_backward_kernel<NN, VM, false, true>), grid, block, lds, st, P, vol, gslices, gvol, ws);
}

// What the two entries share.  det_ws == null: the float entry.  Otherwise `ex` = log2(grad_scale).
int sa_backward_run(const SaParams& P, size_t lds, const float* vol, const float* grad_slices, float* grad_vol,
                    float* grad_transforms, int mode, void* ws, void* det_ws, size_t det_bytes, int ex, hipStream_t st) {
  const size_t nvox = (size_t)P.D * P.H * P.W;
  sa_u64* acc = grad_vol ? static_cast<sa_u64*>(det_ws) : nullptr;
  if (grad_vol) {
    // the float mode sums into grad_vol itself; the fixed-point mode into the accumulators, and grad_vol is written whole later
    const hipError_t e = acc ? hipMemsetAsync(acc, 0, det_bytes, st) : hipMemsetAsync(grad_vol, 0, nvox * sizeof(float), st);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid = sa_grid(P);
  lds += (size_t)SAB_WAVES * 12 * sizeof(float);
  float* wsf = static_cast<float*>(ws);
  const bool gt = grad_transforms != nullptr;
  const double k = ldexp(SA_DET_ONE, -ex);  // 2^32 / grad_scale
  if (mode == FSG_SA_NEAREST_PSF) {
    if (P.vmask) sa_backward_launch<true, true>(P, vol, grad_slices, grad_vol, acc, k, wsf, gt, grid, lds, st);
    else sa_backward_launch<true, false>(P, vol, grad_slices, grad_vol, acc, k, wsf, gt, grid, lds, st);
  } else {
    if (P.vmask) sa_backward_launch<false, true>(P, vol, grad_slices, grad_vol, acc, k, wsf, gt, grid, lds, st);
    else sa_backward_launch<false, false>(P, vol, grad_slices, grad_vol, acc, k, wsf, gt, grid, lds, st);
  }
  if (gt) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    // every workgroup of the first launch stored its partial, so every element of grad_transforms is written here
    hipLaunchKernelGGL(sa_bwd_reduce_kernel, dim3((unsigned)P.n), dim3(FSG_WAVE), 0, st, (const float*)wsf, (int)(grid.x * grid.y),
                       grad_transforms);
  }
  if (acc) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const unsigned blocks = fsg_blocks(nvox, 256, 8192);
    hipLaunchKernelGGL(sa_det_finalize_kernel, dim3(blocks), dim3(256), 0, st, (const long long*)acc, 2, grad_vol,
                       (float*)nullptr, ex - SA_DET_HI_BITS, -SA_DET_HI_BITS, nvox);
  }
  FSG_RETURN_LAUNCH();
}

}  // namespace

extern "C" {

size_t fsg_slice_acq_backward_ws_bytes(int n, int h, int w) {
  return n <= 0 || h <= 0 || w <= 0 ? 0 : sa_partial_bytes(n, h, w, 12);
}

int fsg_slice_acq_backward_f32(const float* transforms, const float* vol, const uint8_t* vol_mask, const float* psf, int pd,
                               int ph, int pw, const float* grad_slices, const uint8_t* slices_mask, float* grad_vol,
                               float* grad_transforms, int D, int H, int W, int n, int h, int w, float res_slice, int mode,
                               void* ws, size_t ws_bytes, void* stream) {
  // every refusal comes before the first write
  if (!vol || !grad_slices || (!grad_vol && !grad_transforms)) return FSG_E_BADARG;
  if (mode != FSG_SA_LINEAR && mode != FSG_SA_NEAREST_PSF) return FSG_E_BADARG;
  SaParams P{transforms, psf, vol_mask, slices_mask, nullptr, D, H, W, pd, ph, pw, n, h, w, res_slice};
  size_t lds = 0;
  const int rc = sa_check(P, lds, false);
  if (rc) return rc;
  if (grad_transforms) {
    if (!ws || ws_bytes < fsg_slice_acq_backward_ws_bytes(n, h, w)) return FSG_E_BADARG;
    if ((uintptr_t)ws & 7) return FSG_E_ALIGN;
  }
  return sa_backward_run(P, lds, vol, grad_slices, grad_vol, grad_transforms, mode, ws, nullptr, 0, 0, fsg_stream(stream));
}

size_t fsg_slice_acq_backward_det_ws_bytes(int D, int H, int W) {
  return D <= 0 || H <= 0 || W <= 0 ? 0 : (size_t)D * H * W * 2 * sizeof(long long);
}

int fsg_slice_acq_backward_det_f32(const float* transforms, const float* vol, const uint8_t* vol_mask, const float* psf, int pd,
                                   int ph, int pw, const float* grad_slices, const uint8_t* slices_mask, float* grad_vol,
                                   float* grad_transforms, int D, int H, int W, int n, int h, int w, float res_slice, int mode,
                                   void* ws, size_t ws_bytes, void* det_ws, size_t det_ws_bytes, float grad_scale,
                                   void* stream) {
  // every refusal comes before the first write
  if (!vol || !grad_slices || (!grad_vol && !grad_transforms)) return FSG_E_BADARG;
  if (mode != FSG_SA_LINEAR && mode != FSG_SA_NEAREST_PSF) return FSG_E_BADARG;
  int ex = 0;
  if (!(grad_scale > 0.f) || frexpf(grad_scale, &ex) != 0.5f || ex - 1 < -20 || ex - 1 > 20) return FSG_E_BADARG;
  SaParams P{transforms, psf, vol_mask, slices_mask, nullptr, D, H, W, pd, ph, pw, n, h, w, res_slice};
  size_t lds = 0;
  const int rc = sa_check(P, lds, false);
  if (rc) return rc;
  if (grad_transforms) {
    if (!ws || ws_bytes < fsg_slice_acq_backward_ws_bytes(n, h, w)) return FSG_E_BADARG;
    if ((uintptr_t)ws & 7) return FSG_E_ALIGN;
  }
  const size_t need = fsg_slice_acq_backward_det_ws_bytes(D, H, W);
  if (grad_vol) {
    if (!det_ws || det_ws_bytes < need) return FSG_E_BADARG;
    if ((uintptr_t)det_ws & 7) return FSG_E_ALIGN;
  }
  return sa_backward_run(P, lds, vol, grad_slices, grad_vol, grad_transforms, mode, ws, grad_vol ? det_ws : nullptr, need, ex - 1,
                         fsg_stream(stream));
}

}  // extern "C"
