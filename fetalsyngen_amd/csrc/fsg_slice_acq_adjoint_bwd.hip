// fsg_slice_acq_adjoint_bwd.hip -- backward of the slice-acquisition ADJOINT operator: gradients of `vol = A^T(slices)` with
// respect to the slices and to the (n,3,4) slice transforms (reference SliceAcqAdjointFunction.backward,
// slice_acq_cuda_kernel.cu:695-950, host side :1079-1132, equalisation of the gradient :672-693 with is_grad = true).
//
// The rule (include/fsg_hip.h):
//   pre-pass (equalize only)  g'[i] = grad_vol[i] / max(vol_weight[i], 1e-3) where vol_weight[i] > 0, grad_vol[i] elsewhere, into
//           the workspace.  The reference divides the incoming gradient in place; here grad_vol is read only.
//   per pixel inside slices_mask, ONE pass over the non-zero PSF taps whose position is inside the volume:
//     LINEAR       val_ = sum over the unmasked corners of corner weight * g'[corner]; val += psf * val_; weight += psf (the tap
//                  counts whatever vol_mask says).  Transforms: per unmasked corner s = (slices[p] - vol[corner]) * g'[corner]
//                  (equalize) or slices[p] * g'[corner]; d = psf * sum of s * d(corner weight)/d(position).
//     NEAREST_PSF  a masked voxel, then a PSF coordinate outside the PSF grid, skip the tap BEFORE it is counted; psf' is the PSF
//                  re-interpolated at the rounded voxel; val += psf' * g'[voxel]; weight += psf'.  Transforms: d = (d psf' / d PSF
//                  coordinate) * s with s as above at the voxel.
//   end of pixel   weight > 0: grad_slices[p] = val / weight and the 12 sums are divided by weight; otherwise the pixel gives 0.
//
// MI355X shape of the work: as the forward and its backward, one 256-thread workgroup = a 16x16 pixel tile of ONE slice, the PSF
// and the per-axis products r_ij * tap_offset in LDS.  The kernel only GATHERS: g' (and vol, vol_mask) are read under the PSF
// straight from global memory, grad_slices is one plain store per thread, and the transform gradients go through the fixed-order
// fold of fsg_sa.h (sa_fold<12>: shuffle tree per wave, waves in order through LDS, one 12-float partial per workgroup, tiles added in index
// order by sa_bwd_reduce_kernel).  No atomics anywhere: both outputs are pure functions of the inputs.
//
// Every range test is written in ACCEPTING form, `if (!(x >= 0 && x < hx ...)) continue;`: a NaN or Inf coordinate (non-finite
// transforms or res_slice) fails it and the tap is skipped, so no address is ever formed from a value that was not proven to be
// inside its array.
#include "fsg_sa.h"

namespace {

// g' = grad_vol / max(vol_weight, 1e-3) where vol_weight > 0 (:672-693, is_grad = true).  The reference's `1e-3` is a double
// literal: the comparison and the division by it are done in double, the division by the weight itself in fp32.
__global__ __launch_bounds__(256) void saa_equalize_grad_kernel(const float* __restrict__ gvol, const float* __restrict__ vw,
                                                                float* __restrict__ out, size_t n) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
    float v = gvol[e];
    const float w = vw[e];
    if (w > 0) v = ((double)w < 1e-3) ? (float)((double)v / 1e-3) : v / w;
    out[e] = v;
  }
}

// G: g' (the workspace copy under equalize, the caller's grad_vol otherwise).  vol: the equalised forward output (EQ only).
template <bool NN, bool VM, bool EQ, bool GS, bool GT>
__global__ __launch_bounds__(SA_TILE* SA_TILE) void sa_adjoint_backward_kernel(SaParams P, const float* __restrict__ G,
                                                                               const float* __restrict__ vol,
                                                                               const float* __restrict__ slices,
                                                                               float* __restrict__ gslices,
                                                                               float* __restrict__ ws) {
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
  const bool live = inside && !(P.smask && !P.smask[idx]);
  float g[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) g[k] = 0.f;
  float val = 0.f, weight = 0.f;

  // no thread leaves before the reduction: a pixel without a contribution carries twelve zeros into it
  if (live) {
    const float s = GT ? slices[idx] : 0.f;
    float _x, _y, _z, xc, yc, zc;
    sa_pixel(P, T, ix, iy, _x, _y, _z);
    sa_centre(P, T, ix, iy, xc, yc, zc);
    const int Sy = P.W, Sz = P.H * P.W;
    const int sy = P.pw, sz = P.pw * P.ph;
    const float hx = (float)(P.W - 1), hy = (float)(P.H - 1), hz = (float)(P.D - 1);
    const float qx = (float)(P.pw - 1), qy = (float)(P.ph - 1), qz = (float)(P.pd - 1);
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
          float val_ = 0.f;
          if (NN) {
            const float xr = roundf(x), yr = roundf(y), zr = roundf(z);
            const int iv = (int)zr * Sz + (int)yr * Sy + (int)xr;
            if (VM && !P.vmask[iv]) continue;  // before the tap is counted: the forward's weight does count it
            float xp, yp, zp;
            sa_psf_coord(P, T, xr - xc, yr - yc, zr - zc, xp, yp, zp);
            if (!(xp >= 0 && yp >= 0 && zp >= 0 && xp < qx && yp < qy && zp < qz)) continue;
            const SaPsfCell c = sa_psf_cell(L, P, xp, yp, zp);
            const float* q = c.q;
            const float wx = c.wx, wy = c.wy, wz = c.wz;
            val_ = G[iv];
            pv = sa_tri8(q, sy, sz, wx, wy, wz);
            if (GT) {
              // d psf' / d (PSF coordinate), times s * g': the rounded voxel is fixed, the PSF moves under it
              float dx = 0.f, dy = 0.f, dz = 0.f, t;
#define SAA_PSF_CORNER(OFF, A, B, C) SA_DCORNER(q[(OFF)], A, B, C)
              SA_CORNERS8(SAA_PSF_CORNER, sy, sz)
#undef SAA_PSF_CORNER
              t = (EQ ? s - vol[iv] : s) * val_;
              dx *= t; dy *= t; dz *= t;
              // lever arm: the rounded voxel relative to the volume centre (exact in fp32: half-integers below 2^23)
              sa_lever_nn(g, dx, dy, dz, xr - hx * 0.5f, yr - hy * 0.5f, zr - hz * 0.5f);
            }
          } else {
            const float xf = floorf(x), yf = floorf(y), zf = floorf(z);
            const float wx = x - xf, wy = y - yf, wz = z - zf;
            const int iv = (int)zf * Sz + (int)yf * Sy + (int)xf;
            if (GS) {
#define SAA_VAL_CORNER(OFF, A, B, C) \
  if (!VM || P.vmask[iv + (OFF)]) val_ += SA_FX(A) * SA_FY(B) * SA_FZ(C) * G[iv + (OFF)];
              SA_CORNERS8(SAA_VAL_CORNER, Sy, Sz)
#undef SAA_VAL_CORNER
            }
            if (GT) {
              // d (trilinear sample of s * g') / d (sampling position) over the unmasked corners, times psf
              float dx = 0.f, dy = 0.f, dz = 0.f, t;
#define SAA_LIN_CORNER(OFF, A, B, C) \
  if (!VM || P.vmask[iv + (OFF)]) { SA_DCORNER((EQ ? s - vol[iv + (OFF)] : s) * G[iv + (OFF)], A, B, C) }
              SA_CORNERS8(SAA_LIN_CORNER, Sy, Sz)
#undef SAA_LIN_CORNER
              dx *= pv; dy *= pv; dz *= pv;
              // lever arm: pixel + translation + tap offset, in slice axes
              sa_lever_lin(g, T, dx, dy, dz, _x + (float)(kx - P.pw / 2), _y + (float)(ky - P.ph / 2),
                           _z + (float)(kz - P.pd / 2));
            }
          }
          if (GS) val += pv * val_;
          weight += pv;
        }
      }
    }
  }

  // `> 0` (the adjoint forward drops the pixel below 0.5): a NaN weight fails the test and the pixel gives zeros
  const bool kept = weight > 0.f;
  if (GS && inside) gslices[idx] = kept ? val / weight : 0.f;
  if (GT) {
#pragma unroll
    for (int k = 0; k < 12; ++k) g[k] = kept ? g[k] / weight : 0.f;
    sa_fold<12>(g, red, ws, in);
  }
}

template <bool NN, bool VM, bool EQ>
void sa_adjoint_backward_launch(const SaParams& P, const float* G, const float* vol, const float* slices, float* gslices,
                                float* ws, bool gt, dim3 grid, size_t lds, hipStream_t st) {
  const dim3 block(SA_TILE, SA_TILE);
  if (gslices && gt)
    hipLaunchKernelGGL((sa_adjoint_backward_kernel<NN, VM, EQ, true, true>), grid, block, lds, st, P, G, vol, slices, gslices, ws);
  else if (gslices)
    hipLaunchKernelGGL((sa_adjoint_backward_kernel<NN, VM, EQ, true, false>), grid, block, lds, st, P, G, vol, slices, gslices, ws);
  else
    hipLaunchKernelGGL((sa_adjoint_backward_kernel<NN, VM, EQ, false, true>), grid, block, lds, st, P, G, vol, slices, gslices, ws);
}

template <bool NN, bool VM>
void sa_adjoint_backward_dispatch(const SaParams& P, bool eq, const float* G, const float* vol, const float* slices,
                                float* gslices, float* ws, bool gt, dim3 grid, size_t lds, hipStream_t st) {
  if (eq) sa_adjoint_backward_launch<NN, VM, true>(P, G, vol, slices, gslices, ws, gt, grid, lds, st);
  else sa_adjoint_backward_launch<NN, VM, false>(P, G, vol, slices, gslices, ws, gt, grid, lds, st);
}

}  // namespace

extern "C" {

size_t fsg_slice_acq_adjoint_backward_ws_bytes(int D, int H, int W, int n, int h, int w, int equalize, int want_transforms) {
  if (D <= 0 || H <= 0 || W <= 0 || n <= 0 || h <= 0 || w <= 0) return 0;
  return (want_transforms ? sa_partial_bytes(n, h, w, 12) : 0) + (equalize ? (size_t)D * H * W * sizeof(float) : 0);
}

int fsg_slice_acq_adjoint_backward_f32(const float* transforms, const float* grad_vol, const float* vol_weight, const float* vol,
                                       const uint8_t* vol_mask, const float* psf, int pd, int ph, int pw, const float* slices,
                                       const uint8_t* slices_mask, float* grad_slices, float* grad_transforms, int D, int H,
                                       int W, int n, int h, int w, float res_slice, int mode, int equalize, void* ws,
                                       size_t ws_bytes, void* stream) {
  // every refusal comes before the first write
  if (!grad_vol || !slices || (!grad_slices && !grad_transforms)) return FSG_E_BADARG;
  if (mode != FSG_SA_LINEAR && mode != FSG_SA_NEAREST_PSF) return FSG_E_BADARG;
  if (equalize && (!vol_weight || !vol)) return FSG_E_BADARG;
  SaParams P{transforms, psf, vol_mask, slices_mask, nullptr, D, H, W, pd, ph, pw, n, h, w, res_slice};
  size_t lds = 0;
  const int rc = sa_check(P, lds, false);
  if (rc) return rc;
  const bool gt = grad_transforms != nullptr, eq = equalize != 0;
  const size_t need = fsg_slice_acq_adjoint_backward_ws_bytes(D, H, W, n, h, w, eq, gt);
  if (need) {
    if (!ws || ws_bytes < need) return FSG_E_BADARG;
    if ((uintptr_t)ws & 7) return FSG_E_ALIGN;
  }
  hipStream_t st = fsg_stream(stream);
  float* partials = static_cast<float*>(ws);
  const float* G = grad_vol;
  if (eq) {
    float* ge = reinterpret_cast<float*>(static_cast<char*>(ws) + (gt ? sa_partial_bytes(n, h, w, 12) : 0));
    const size_t nv = (size_t)D * H * W;
    const unsigned blocks = fsg_blocks(nv, 256, 8192);
    hipLaunchKernelGGL(saa_equalize_grad_kernel, dim3(blocks), dim3(256), 0, st, grad_vol, vol_weight, ge, nv);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    G = ge;
  }
  const dim3 grid = sa_grid(P);
  lds += (size_t)SAB_WAVES * 12 * sizeof(float);
  if (mode == FSG_SA_NEAREST_PSF) {
    if (vol_mask) sa_adjoint_backward_dispatch<true, true>(P, eq, G, vol, slices, grad_slices, partials, gt, grid, lds, st);
    else sa_adjoint_backward_dispatch<true, false>(P, eq, G, vol, slices, grad_slices, partials, gt, grid, lds, st);
  } else {
    if (vol_mask) sa_adjoint_backward_dispatch<false, true>(P, eq, G, vol, slices, grad_slices, partials, gt, grid, lds, st);
    else sa_adjoint_backward_dispatch<false, false>(P, eq, G, vol, slices, grad_slices, partials, gt, grid, lds, st);
  }
  if (gt) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    // every workgroup of the first launch stored its partial, so every element of grad_transforms is written here
    hipLaunchKernelGGL(sa_bwd_reduce_kernel, dim3((unsigned)n), dim3(FSG_WAVE), 0, st, (const float*)partials,
                       (int)(grid.x * grid.y), grad_transforms);
  }
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
