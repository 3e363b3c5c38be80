// fsg_svr.hip -- per-slice Levenberg-Marquardt slice-to-volume registration (the contract is in
// include/fsg_hip.h, fsg_svr_*).
//
//   fsg_svr_normal_f32   one pass over the PSF taps gives, per pixel, the simulated value s, its 12 derivatives with respect to
//                        the slice's transform (the sums sa_backward_body forms for gs = 1 / weight: the same SA_DCORNER /
//                        sa_lever_lin operations in the same order, the weight held constant), their projection on the 6 pose
//                        parameters through `jac`, and the pixel's 30 terms of H = sum w J J^T (upper triangle), g = sum w e J,
//                        sum w e^2, sum w and the pixel count.  FSG_SA_LINEAR geometry only, no vol_mask.
//   fsg_svr_update_f32   the damped step and the accept / reject decision, one thread per slice in double.
//
// MI355X shape of the work: as the backward of the forward, one 256-thread workgroup = a 16x16 pixel tile of ONE slice, the PSF
// and the per-axis tap products in LDS (sa_fill_lds), the slice's 72 jac entries beside them.  No atomics: each lane keeps its
// 30 terms in registers, a wave folds them with a fixed shuffle tree, the four waves meet in LDS and are added in wave order
// (sa_fold<30, 32> of fsg_sa.h, the fold of the two backward units at another width),
// the workgroup stores ONE 32-float partial at ws[slice][tile], and svr_reduce_kernel adds a slice's tiles in double in
// tile-index order.  The result is a pure function of one slice's inputs.
//
// Every range test is in ACCEPTING form, so a NaN or Inf coordinate skips the tap and no address is formed from a value that
// was not proven to be inside its array.  The iteration cap and the width of a row are the header's (FSG_SOLVER_MAX_ITER,
// FSG_SVR_SLOTS); the overlap and finite tests are fsg_common.h's.
#include "fsg_sa.h"

namespace {

constexpr int SVR_TERMS = 30;  // 21 + 6 + 1 + 1 + 1
// a partial and a row of `stats` are FSG_SVR_SLOTS = 32 wide; slots 30, 31 are 0

__global__ __launch_bounds__(SA_TILE* SA_TILE) void svr_normal_kernel(SaParams P, const float* __restrict__ vol,
                                                                      const float* __restrict__ jac,
                                                                      const float* __restrict__ slices,
                                                                      const float* __restrict__ sweight, float min_weight,
                                                                      float* __restrict__ ws) {
  extern __shared__ float smem[];
  const int in = blockIdx.z;
  const float* __restrict__ T = P.tr + (size_t)in * 12;
  const SaLds L = sa_lds_layout(smem, P);
  float* jl = L.tz + 3 * P.pd;  // [12][6]
  float* red = jl + 72;         // [SAB_WAVES][FSG_SVR_SLOTS]
  sa_fill_lds(L, P, T, sa_tid(), SA_TILE * SA_TILE);
  if (sa_tid() < 72) jl[sa_tid()] = jac[(size_t)in * 72 + sa_tid()];
  __syncthreads();
  const int ix = blockIdx.x * SA_TILE + threadIdx.x, iy = blockIdx.y * SA_TILE + threadIdx.y;
  const bool inside = ix < P.w && iy < P.h;
  const size_t idx = ((size_t)in * P.h + (inside ? iy : 0)) * P.w + (inside ? ix : 0);
  const bool active = inside && !(P.smask && !P.smask[idx]);
  float out[SVR_TERMS];
#pragma unroll
  for (int k = 0; k < SVR_TERMS; ++k) out[k] = 0.f;

  // no thread leaves before the fold
  if (active) {
    float _x, _y, _z, xc, yc, zc;
    sa_pixel(P, T, ix, iy, _x, _y, _z);
    sa_centre(P, T, ix, iy, xc, yc, zc);
    const int Sy = P.W, Sz = P.H * P.W;
    const float hx = (float)(P.W - 1), hy = (float)(P.H - 1), hz = (float)(P.D - 1);

    // ---- pass 1: the pixel's weight, as fsg_slice_acq_backward_f32 in LINEAR ----
    float weight = 0.f;
    int ip = 0;
    for (int kz = 0; kz < P.pd; ++kz) {
      const float zx = L.tz[kz], zy = L.tz[P.pd + kz], zz = L.tz[2 * P.pd + kz];
      for (int ky = 0; ky < P.ph; ++ky) {
        const float yx = L.ty[ky], yy = L.ty[P.ph + ky], yz = L.ty[2 * P.ph + ky];
        for (int kx = 0; kx < P.pw; ++kx, ++ip) {
          const float pv = L.psf[ip];
          if (pv == 0.f) continue;  // wave-uniform
          const float x = xc + L.tx[kx] + yx + zx;
          const float y = yc + L.tx[P.pw + kx] + yy + zy;
          const float z = zc + L.tx[2 * P.pw + kx] + yz + zz;
          if (!(x >= 0 && y >= 0 && z >= 0 && x < hx && y < hy && z < hz)) continue;
          weight += pv;
        }
      }
    }

    // ---- pass 2: the value and its 12 derivatives ----
    if (weight > 0.f && weight >= min_weight) {  // a NaN weight takes no part
      const float gs = 1.f / weight;
      float val = 0.f;
      float g[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) g[k] = 0.f;
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
            const float xf = floorf(x), yf = floorf(y), zf = floorf(z);
            const float wx = x - xf, wy = y - yf, wz = z - zf;
            const float* __restrict__ q = vol + ((int)zf * Sz + (int)yf * Sy + (int)xf);
            const float pg = pv * gs;
            float dx = 0.f, dy = 0.f, dz = 0.f, t, tri = 0.f;
            // one walk over the eight corners: the trilinear sample (sa_tri8's terms in its order) and its derivative
#define SVR_CORNER(OFF, A, B, C)                    \
  {                                                 \
    const float c_ = q[(OFF)];                      \
    tri += SA_FX(A) * SA_FY(B) * SA_FZ(C) * c_;     \
    SA_DCORNER(pg * c_, A, B, C)                    \
  }
            SA_CORNERS8(SVR_CORNER, Sy, Sz)
#undef SVR_CORNER
            val += pv * tri;
            sa_lever_lin(g, T, dx, dy, dz, _x + (float)(kx - P.pw / 2), _y + (float)(ky - P.ph / 2),
                         _z + (float)(kz - P.pd / 2));
          }
        }
      }
      const float s = val / weight;
      const float e = s - slices[idx];
      const float w = sweight ? sweight[idx] : 1.f;
      const float we = w * e;
      float J[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k) acc += jl[k * 6 + a] * g[k];
        J[a] = acc;
      }
      int o = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const float wj = w * J[a];
#pragma unroll
        for (int b = a; b < 6; ++b) out[o++] = wj * J[b];
      }
#pragma unroll
      for (int a = 0; a < 6; ++a) out[21 + a] = we * J[a];
      out[27] = we * e;
      out[28] = w;
      out[29] = 1.f;
    }
  }
  sa_fold<SVR_TERMS, FSG_SVR_SLOTS>(out, red, ws, in);  // all 32 slots: the workspace needs no zeroing
}

// stats[slice][k] = the slice's tile partials added in double in tile-index order.  One wave per slice, 32 lanes busy.
__global__ __launch_bounds__(FSG_WAVE) void svr_reduce_kernel(const float* __restrict__ ws, int tiles, double* __restrict__ stats) {
  const int in = blockIdx.x, k = threadIdx.x;
  if (k >= FSG_SVR_SLOTS) return;
  const float* p = ws + (size_t)in * tiles * FSG_SVR_SLOTS + k;
  double v = 0.0;
  for (int t = 0; t < tiles; ++t) v = v + (double)p[(size_t)t * FSG_SVR_SLOTS];
  stats[(size_t)in * FSG_SVR_SLOTS + k] = k < SVR_TERMS ? v : 0.0;
}

// ---- the state block of a solve (layout in fsg_hip.h): svr_state is its one statement here, svr_state_bytes measures it ----
struct SvrState {
  double* stats_cur;   // [n][32]
  double* lambda;      // [n]
  double* m0;          // [n]
  double* cost_h;      // [K+1][n]
  double* lambda_h;    // [K+1][n]
  float* theta_cur;    // [n][6]
  int32_t* frozen;     // [n]
  int32_t* accepted_h; // [K+1][n]
  int32_t* frozen_h;   // [K+1][n]
  void* end;           // one past frozen_h
};

__host__ __device__ inline SvrState svr_state(void* p, size_t n, int K) {
  const size_t s = (size_t)K + 1;
  SvrState S;
  S.stats_cur = (double*)p;
  S.lambda = S.stats_cur + FSG_SVR_SLOTS * n;
  S.m0 = S.lambda + n;
  S.cost_h = S.m0 + n;
  S.lambda_h = S.cost_h + s * n;
  S.theta_cur = (float*)(S.lambda_h + s * n);
  S.frozen = (int32_t*)(S.theta_cur + 6 * n);
  S.accepted_h = S.frozen + n;
  S.frozen_h = S.accepted_h + s * n;
  S.end = S.frozen_h + s * n;
  return S;
}

inline size_t svr_state_bytes(size_t n, int K) { return fsg_carved_bytes(fsg_origin, svr_state(fsg_origin, n, K).end); }

struct SvrOpts {
  double lambda0, factor, lambda_min, lambda_max, min_overlap, tol;
};

// One thread per slice; double, + - * / only (the factorisation is Cholesky's square-root-free form A = L D L^T, whose pivots
// are the squares of Cholesky's own, so `pivot > 0` is the same test and every operation is correctly rounded).
__global__ __launch_bounds__(256) void svr_update_kernel(const double* __restrict__ stats_trial, float* __restrict__ theta_trial,
                                                         void* state, int n, int k, int K, SvrOpts O) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const SvrState S = svr_state(state, (size_t)n, K);
  const double* tr = stats_trial + (size_t)i * FSG_SVR_SLOTS;
  double* cur = S.stats_cur + (size_t)i * FSG_SVR_SLOTS;
  float* th_t = theta_trial + (size_t)i * 6;
  float* th_c = S.theta_cur + (size_t)i * 6;
  bool fin = true;
  for (int j = 0; j < SVR_TERMS; ++j) fin = fin && fsg_finite(tr[j]);
  const double cost_t = tr[27] / tr[28], m_t = tr[29];
  bool frozen;
  int accepted = 0;
  double lambda;
  if (k == 0) {
    for (int j = 0; j < FSG_SVR_SLOTS; ++j) cur[j] = tr[j];
    for (int j = 0; j < 6; ++j) th_c[j] = th_t[j];
    S.m0[i] = m_t;
    lambda = O.lambda0;
    frozen = !(m_t >= 1.0) || !(tr[28] > 0.0) || !fin;
  } else {
    frozen = S.frozen[i] != 0;
    lambda = S.lambda[i];
    if (!frozen) {
      const double cost_old = cur[27] / cur[28];
      if (fin && m_t >= O.min_overlap * S.m0[i] && cost_t < cost_old) {
        accepted = 1;
        for (int j = 0; j < FSG_SVR_SLOTS; ++j) cur[j] = tr[j];
        for (int j = 0; j < 6; ++j) th_c[j] = th_t[j];
        lambda = fmax(lambda / O.factor, O.lambda_min);
        if (cost_old - cost_t <= O.tol * cost_old) frozen = true;
      } else {
        lambda = lambda * O.factor;
        if (lambda > O.lambda_max) frozen = true;
      }
    }
  }
  // ---- the next trial ----  (loops of fixed length, fully unrolled: A, L and D stay in registers; a slice that does not move
  // computes on and its values are dropped, a failed pivot included: its quotients never reach memory)
  double d[6];
  bool bad = false;
  {
    double A[6][6], b[6], z[6];
    int o = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int c = a; c < 6; ++c) { A[a][c] = cur[o]; A[c][a] = cur[o]; ++o; }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) b[a] = cur[21 + a];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const bool live = A[a][a] != 0.0;
      const double damped = A[a][a] + lambda * A[a][a];  // Marquardt: H + lambda diag(H)
#pragma unroll
      for (int c = 0; c < 6; ++c) {  // a parameter the data do not see: unit row and column, no step
        A[a][c] = live ? A[a][c] : 0.0;
        A[c][a] = live ? A[c][a] : 0.0;
      }
      A[a][a] = live ? damped : 1.0;
      b[a] = live ? b[a] : 0.0;
    }
    // A = L D L^T in place: L below the diagonal, D on it
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double dj = A[j][j];
#pragma unroll
      for (int p = 0; p < j; ++p) dj = dj - A[j][p] * A[j][p] * A[p][p];
      bad = bad || !(dj > 0.0);
      A[j][j] = dj;
#pragma unroll
      for (int r = j + 1; r < 6; ++r) {
        double v = A[r][j];
#pragma unroll
        for (int p = 0; p < j; ++p) v = v - A[r][p] * A[j][p] * A[p][p];
        A[r][j] = v / dj;
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {  // L z = g
      double v = b[r];
#pragma unroll
      for (int p = 0; p < r; ++p) v = v - A[r][p] * z[p];
      z[r] = v;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) z[r] = z[r] / A[r][r];
#pragma unroll
    for (int r = 5; r >= 0; --r) {  // L^T x = z
      double v = z[r];
#pragma unroll
      for (int p = r + 1; p < 6; ++p) v = v - A[p][r] * d[p];
      d[r] = v;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) d[r] = -d[r];
  }
  if (!frozen && k < K && bad) frozen = true;  // a pivot that is not > 0
  const bool move = !frozen && k < K;
  for (int j = 0; j < 6; ++j) th_t[j] = move ? (float)((double)th_c[j] + d[j]) : th_c[j];
  S.lambda[i] = lambda;
  S.frozen[i] = frozen ? 1 : 0;
  const size_t h = (size_t)k * n + i;
  S.cost_h[h] = cur[27] / cur[28];
  S.lambda_h[h] = lambda;
  S.accepted_h[h] = accepted;
  S.frozen_h[h] = frozen ? 1 : 0;
}

}  // namespace

extern "C" {

size_t fsg_svr_ws_bytes(int n, int h, int w) { return n <= 0 || h <= 0 || w <= 0 ? 0 : sa_partial_bytes(n, h, w, FSG_SVR_SLOTS); }

int fsg_svr_normal_f32(const float* transforms, const float* jac, const float* vol, const float* psf, int pd, int ph, int pw,
                       const float* slices, const uint8_t* slices_mask, const float* slices_weight, double* stats, int D, int H,
                       int W, int n, int h, int w, float res_slice, float min_weight, int mode, void* ws, size_t ws_bytes,
                       void* stream) {
  // every refusal comes before the first write
  if (!jac || !vol || !slices || !stats) return FSG_E_BADARG;
  if (mode != FSG_SA_LINEAR) return FSG_E_BADARG;
  if (!(min_weight >= 0.f)) return FSG_E_BADARG;  // negative or NaN
  SaParams P{transforms, psf, nullptr, slices_mask, nullptr, D, H, W, pd, ph, pw, n, h, w, res_slice};
  size_t lds = 0;
  const int rc = sa_check(P, lds, false);
  if (rc) return rc;
  if (!ws || ws_bytes < fsg_svr_ws_bytes(n, h, w)) return FSG_E_BADARG;
  if (((uintptr_t)ws & 7) || ((uintptr_t)stats & 7)) return FSG_E_ALIGN;
  lds += (size_t)(72 + SAB_WAVES * FSG_SVR_SLOTS) * sizeof(float);
  const dim3 grid = sa_grid(P);
  hipStream_t st = fsg_stream(stream);
  hipLaunchKernelGGL(svr_normal_kernel, grid, dim3(SA_TILE, SA_TILE), lds, st, P, vol, jac, slices, slices_weight, min_weight,
                     static_cast<float*>(ws));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  // every workgroup of the first launch stored its partial, so every slot of stats is written here
  hipLaunchKernelGGL(svr_reduce_kernel, dim3((unsigned)n), dim3(FSG_WAVE), 0, st, (const float*)ws, (int)(grid.x * grid.y), stats);
  FSG_RETURN_LAUNCH();
}

size_t fsg_svr_state_bytes(int n, int n_iter) {
  if (n <= 0 || n_iter < 1 || n_iter > FSG_SOLVER_MAX_ITER) return 0;
  return svr_state_bytes((size_t)n, n_iter);
}

int fsg_svr_update_f32(const double* stats_trial, float* theta_trial, void* state, size_t state_bytes, int n, int k, int n_iter,
                       double lambda0, double factor, double lambda_min, double lambda_max, double min_overlap, double tol,
                       void* stream) {
  if (n <= 0 || n_iter < 1 || n_iter > FSG_SOLVER_MAX_ITER || k < 0 || k > n_iter) return FSG_E_BADARG;
  if (!stats_trial || !theta_trial || !state || state_bytes < fsg_svr_state_bytes(n, n_iter)) return FSG_E_BADARG;
  if (!(lambda0 > 0.0) || !(factor > 1.0) || !(lambda_min > 0.0) || !(lambda_max >= lambda_min) || !(min_overlap >= 0.0) ||
      !(tol >= 0.0))
    return FSG_E_BADARG;
  if (((uintptr_t)state & 7) || ((uintptr_t)stats_trial & 7) || ((uintptr_t)theta_trial & 3)) return FSG_E_ALIGN;
  const size_t sb = (size_t)n * FSG_SVR_SLOTS * sizeof(double), tb = (size_t)n * 6 * sizeof(float);
  if (fsg_overlap(state, state_bytes, stats_trial, sb) || fsg_overlap(state, state_bytes, theta_trial, tb) ||
      fsg_overlap(theta_trial, tb, stats_trial, sb))
    return FSG_E_BADARG;
  const SvrOpts O{lambda0, factor, lambda_min, lambda_max, min_overlap, tol};
  hipLaunchKernelGGL(svr_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fsg_stream(stream), stats_trial,
                     theta_trial, state, n, k, n_iter, O);
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
