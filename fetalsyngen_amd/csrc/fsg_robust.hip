// fsg_robust.hip -- outlier weights for srr / svr: the robust-statistics EM of the slice-to-volume family (DESIGN.md section
// 25; the contract, the rule and the layout of the state block are in include/fsg_hip.h, fsg_robust_*).
//
//   fsg_robust_estep_f32    one streaming pass over y and s = A x: per pixel the inlier posterior p, per workgroup one partial
//                           of the six per-slice sums (count, sum p, sum p e^2, sum (1-p)^2, min y, max y).
//   fsg_robust_update_f32   one workgroup: folds a slice's partials in double, then the pixel parameters (sigma, c), one sweep
//                           of the two-class slice EM, and the two floats (kappa, inv2var) the next estep reads.
//   fsg_robust_weights_f32  the last pass: out = ws_k (* p) on the pixels that take part, 0 elsewhere.
//
// MI355X shape of the work: the passes are pure streaming (9 to 13 bytes a pixel, no reuse), so the workgroup is 256 threads
// that each own FOUR consecutive pixels of one slice, 1024 pixels a workgroup: with 16-byte alignment every lane issues one
// 16-byte load per array and a wave reads 1 KiB contiguously.  No LDS beyond the 4 x 8 floats where the waves meet, about 30
// VGPRs: occupancy is not the limit, HBM is.  No atomics: fixed shuffle tree per wave, waves in order, one 8-float partial per
// workgroup in a workspace that needs no zeroing, a slice's partials added in double in index order by the update.
// The iteration cap and the width of a slice's row are the header's (FSG_SOLVER_MAX_ITER, FSG_ROBUST_ROW); the overlap and
// finite tests, the measuring of the state block and the workgroup fold are fsg_common.h's; the streaming geometry, the shape
// check, the 4-pixel loads and stores, the gate and the fold of a slice's partials (N, sum p, sum p e^2, sum (1-p)^2, min y,
// max y, 0, 0) are fsg_pixels.h's, shared with fsg_imatch.hip.
#include "fsg_pixels.h"
#include <math.h>

namespace {

struct RbState {  // pointers into the state block for (n, T); layout in fsg_hip.h, stated here once by rb_state and measured by rb_state_bytes
  double* consts;   // [4] R, m, sigma_min, 0
  double* rows;     // [n][6]
  double* u;        // [n]
  double* sigma;    // [s]
  double* c;        // [s]
  double* mu1;      // [s]
  double* mu2;      // [s]
  double* ws;       // [s][n]
  float* scal;      // [2] kappa, inv2var
  int32_t* frozen;  // [s]
  void* end;        // one past frozen
};

__host__ __device__ inline RbState rb_state(void* p, size_t n, int T) {
  const size_t s = (size_t)T + 1;
  RbState S;
  S.consts = (double*)p;
  S.rows = S.consts + 4;
  S.u = S.rows + FSG_ROBUST_ROW * n;
  S.sigma = S.u + n;
  S.c = S.sigma + s;
  S.mu1 = S.c + s;
  S.mu2 = S.mu1 + s;
  S.ws = S.mu2 + s;
  S.scal = (float*)(S.ws + s * n);
  S.frozen = (int32_t*)(S.scal + 2);
  S.end = S.frozen + s;
  return S;
}

inline size_t rb_state_bytes(size_t n, int T) { return fsg_carved_bytes(fsg_origin, rb_state(fsg_origin, n, T).end); }

struct RbIn {
  const float* y;
  const float* s;
  const uint8_t* mask;
  const float* sw;
  float min_weight;
  int hw;
};

// The four pixels of a thread: e = fl(y - s), `part` = the pixel is in Omega.  A pixel past the end of the slice takes no part
// and no address is formed for it.
template <bool VEC>
__device__ __forceinline__ void rb_load(const RbIn& I, size_t base, int e0, float (&y)[4], float (&e)[4], bool (&part)[4]) {
  const int cnt = I.hw - e0 < 4 ? I.hw - e0 : 4;  // >= 1 for a thread that is called
  const size_t a = base + e0;
  float s[4], wg[4] = {0.f, 0.f, 0.f, 0.f};
  px_load4<VEC>(I.y, a, cnt, y);
  px_load4<VEC>(I.s, a, cnt, s);
  if (I.sw) px_load4<VEC>(I.sw, a, cnt, wg);
  const uint32_t mk = px_mask4<VEC>(I.mask, a, cnt);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    e[j] = y[j] - s[j];
    const bool ok = j < cnt && px_gate(px_mask_bit(mk, j), I.sw != nullptr, wg[j], I.min_weight);
    part[j] = ok && fabsf(e[j]) <= PX_FLT_MAX;  // NaN and Inf fail
  }
}

// p = 1 / (1 + kappa * expf(e^2 * inv2var)), one rounding per operation; an overflowing expf gives 0
__device__ __forceinline__ float rb_posterior(float e2, float kappa, float inv2var) {
  const float x = expf(e2 * inv2var);
  return x <= PX_FLT_MAX ? 1.f / (1.f + kappa * x) : 0.f;
}

template <bool VEC>
__global__ __launch_bounds__(PX_THREADS) void rb_estep_kernel(RbIn I, int n, int T, int first, const void* state,
                                                              float* __restrict__ ws) {
  __shared__ float red[PX_THREADS / FSG_WAVE][PX_SLOTS];
  const int k = blockIdx.y, tid = threadIdx.x;
  const int e0 = (blockIdx.x * PX_THREADS + tid) * 4;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  float mn = INFINITY, mx = -INFINITY;
  // no thread leaves before the fold
  if (e0 < I.hw) {
    const RbState S = rb_state(const_cast<void*>(state), (size_t)n, T);
    const float kappa = first ? 0.f : S.scal[0], inv2var = first ? 0.f : S.scal[1];
    float y[4], e[4];
    bool part[4];
    rb_load<VEC>(I, (size_t)k * I.hw, e0, y, e, part);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!part[j]) continue;
      const float e2 = e[j] * e[j];
      const float p = first ? 1.f : rb_posterior(e2, kappa, inv2var);
      const float q = 1.f - p;
      v[0] += 1.f;
      v[1] += p;
      v[2] += p * e2;
      v[3] += q * q;
      mn = fminf(mn, y[j]);
      mx = fmaxf(mx, y[j]);
    }
  }
  fsg_fold_sums_minmax<FSG_ROBUST_ROW - 2, PX_SLOTS, PX_THREADS>(v, mn, mx, red, ws + ((size_t)k * gridDim.x + blockIdx.x) * PX_SLOTS);
}

struct RbOpts {
  double c0, sigma_floor, slice_floor;
  int min_pixels;
};

__device__ __forceinline__ double rb_normal_pdf(double u, double mu, double v) {
  const double d = u - mu;
  return exp(-(d * d) / (2.0 * v)) / sqrt(6.283185307179586 * v);
}

// One workgroup.  Phase A, a thread per slice: the row and u.  Phase B, wave 0: every sum over the slices, in slice-index
// order.  Phase C, a thread per slice: the new slice weight.
__global__ __launch_bounds__(PX_THREADS) void rb_update_kernel(void* state, const float* __restrict__ ws, int chunks, int n, int t,
                                                               int T, RbOpts O) {
  __shared__ double sh[6];  // frozen, mu1, mu2, v1, v2, mix
  const RbState S = rb_state(state, (size_t)n, T);
  const int tid = threadIdx.x;
  const double* wold = t > 0 ? S.ws + (size_t)(t - 1) * n : nullptr;
  double* wnew = S.ws + (size_t)t * n;
  for (int k = tid; k < n; k += PX_THREADS) {
    double r[FSG_ROBUST_ROW - 2], mn, mx;
    const bool any = px_fold_slice(ws + (size_t)k * chunks * PX_SLOTS, chunks, r, mn, mx);
    double* row = S.rows + (size_t)k * FSG_ROBUST_ROW;
#pragma unroll
    for (int j = 0; j < FSG_ROBUST_ROW - 2; ++j) row[j] = r[j];
    row[FSG_ROBUST_ROW - 2] = mn;
    row[FSG_ROBUST_ROW - 1] = mx;
    const bool ok = r[0] >= (double)O.min_pixels && any;
    S.u[k] = ok ? sqrt(r[3] / r[0]) : 0.0;
  }
  __syncthreads();
  // Wave 0, all 64 lanes in step: a lane loads the figures of ONE slice (64 slices per trip, one memory latency), then the
  // wave walks the 64 in index order, every lane adding the broadcast values: the sums of a serial loop over the slices, in
  // its order, without its one memory latency per slice.  Every lane holds the same scalars; lane 0 stores them.
  if (tid < FSG_WAVE) {
    bool frozen = t > 0 && S.frozen[t - 1] != 0;
    double m, smin;
    if (t == 0) {
      double mn, mx;
      px_wave_range<FSG_ROBUST_ROW>(S.rows, n, mn, mx);
      const double R = mx - mn;
      const bool good = fsg_finite(R) && R > 0.0 && fsg_finite(1.0 / R);
      if (tid == 0) {
        S.consts[0] = good ? R : 0.0;
        S.consts[1] = good ? 1.0 / R : 0.0;
        S.consts[2] = good ? O.sigma_floor * R : 0.0;
        S.consts[3] = 0.0;
      }
      m = good ? 1.0 / R : 0.0;
      smin = good ? O.sigma_floor * R : 0.0;
      frozen = !good;
    } else {
      m = S.consts[1];
      smin = S.consts[2];
    }
    double S0 = 0.0, S2 = 0.0, Nw = 0.0;
    double sw = 0.0, swu = 0.0, so = 0.0, sou = 0.0, umax = 0.0, nok = 0.0;
    for (int base = 0; base < n; base += FSG_WAVE) {
      const int k = base + tid, cnt = n - base < FSG_WAVE ? n - base : FSG_WAVE;
      const bool in = k < n;
      const double* row = S.rows + (size_t)(in ? k : 0) * FSG_ROBUST_ROW;
      const double lN = in ? row[0] : 0.0, lp = in ? row[1] : 0.0, le = in ? row[2] : 0.0, lu = in ? S.u[k] : 0.0;
      const double lw = !in ? 0.0 : (wold ? wold[k] : 1.0);
      for (int j = 0; j < cnt; ++j) {
        const double N = __shfl(lN, j, FSG_WAVE), sp = __shfl(lp, j, FSG_WAVE), se = __shfl(le, j, FSG_WAVE);
        const double u = __shfl(lu, j, FSG_WAVE), wj = __shfl(lw, j, FSG_WAVE);
        const bool ok = N >= (double)O.min_pixels && N > 0.0;
        const double w = ok ? wj : 0.0;
        S0 = S0 + w * sp;
        S2 = S2 + w * se;
        Nw = Nw + w * N;
        if (ok) {  // the slice mixture's moments under the old weights (used for t >= 1)
          sw = sw + wj;
          swu = swu + wj * u;
          so = so + (1.0 - wj);
          sou = sou + (1.0 - wj) * u;
          umax = fmax(umax, u);
          nok = nok + 1.0;
        }
      }
    }
    const double var = fmax(S2 / S0, smin * smin);
    const double c = t == 0 ? O.c0 : S0 / Nw;
    const double kappa = ((1.0 - c) / c) * m * sqrt(6.283185307179586 * var), inv2var = 1.0 / (2.0 * var);
    const float kf = (float)kappa, vf = (float)inv2var;
    frozen = frozen || !(Nw > 0.0) || !(S0 > 0.0) || !fsg_finite(S2) || !fsg_finite(var) || !(var > 0.0) || !fsg_finite(c) ||
             !(fabsf(kf) <= PX_FLT_MAX) || !(fabsf(vf) <= PX_FLT_MAX) || !(kf >= 0.f);
    double mu1 = 0.0, mu2 = 0.0, v1 = 0.0, v2 = 0.0, mix = 1.0;
    if (t > 0 && !frozen) {  // wave-uniform
      const double fl2 = O.slice_floor * O.slice_floor;
      mu1 = swu / sw;
      mu2 = so > 0.0 ? sou / so : (umax + mu1) / 2.0;
      double a1 = 0.0, a2 = 0.0;
      for (int base = 0; base < n; base += FSG_WAVE) {
        const int k = base + tid, cnt = n - base < FSG_WAVE ? n - base : FSG_WAVE;
        const bool in = k < n;
        const double lN = in ? S.rows[(size_t)k * FSG_ROBUST_ROW] : 0.0, lu = in ? S.u[k] : 0.0, lw = in ? wold[k] : 0.0;
        for (int j = 0; j < cnt; ++j) {
          const double N = __shfl(lN, j, FSG_WAVE), u = __shfl(lu, j, FSG_WAVE), w = __shfl(lw, j, FSG_WAVE);
          if (!(N >= (double)O.min_pixels && N > 0.0)) continue;
          a1 = a1 + w * ((u - mu1) * (u - mu1));
          a2 = a2 + (1.0 - w) * ((u - mu2) * (u - mu2));
        }
      }
      v1 = fmax(a1 / sw, fl2);
      v2 = so > 0.0 ? a2 / so : 0.0;
      if (!(v2 > 0.0)) v2 = ((mu2 - mu1) * (mu2 - mu1)) / 4.0;
      v2 = fmax(v2, fl2);
      mix = sw / nok;
      frozen = !fsg_finite(mu1) || !fsg_finite(mu2) || !fsg_finite(v1) || !fsg_finite(v2) || !fsg_finite(mix);
    }
    if (tid == 0) {
      S.sigma[t] = frozen ? 0.0 : sqrt(var);
      S.c[t] = frozen ? 0.0 : c;
      S.mu1[t] = frozen ? 0.0 : mu1;
      S.mu2[t] = frozen ? 0.0 : mu2;
      S.frozen[t] = frozen ? 1 : 0;
      S.scal[0] = frozen ? 0.f : kf;
      S.scal[1] = frozen ? 0.f : vf;
      sh[0] = frozen ? 1.0 : 0.0;
      sh[1] = mu1; sh[2] = mu2; sh[3] = v1; sh[4] = v2; sh[5] = mix;
    }
  }
  __syncthreads();
  const bool frozen = sh[0] != 0.0;
  const double mu1 = sh[1], mu2 = sh[2], v1 = sh[3], v2 = sh[4], mix = sh[5];
  for (int k = tid; k < n; k += PX_THREADS) {
    const double N = S.rows[(size_t)k * FSG_ROBUST_ROW];
    const bool ok = N >= (double)O.min_pixels && N > 0.0;
    double w = ok ? 1.0 : 0.0;
    if (ok && t > 0 && !frozen) {
      const double u = S.u[k];
      if (u < mu1) w = 1.0;
      else if (u > mu2) w = 0.0;
      else {
        const double g1 = rb_normal_pdf(u, mu1, v1) * mix, g2 = rb_normal_pdf(u, mu2, v2) * (1.0 - mix);
        const double den = g1 + g2;
        // both densities underflowed, or a zero variance: the class of the nearer mean
        w = (den > 0.0 && fsg_finite(den) && fsg_finite(g1)) ? g1 / den : (fabs(u - mu1) <= fabs(u - mu2) ? 1.0 : 0.0);
      }
    }
    wnew[k] = w;
  }
}

template <bool VEC>
__global__ __launch_bounds__(PX_THREADS) void rb_weights_kernel(RbIn I, int n, int T, int both, const void* state,
                                                                float* __restrict__ out) {
  const int k = blockIdx.y;
  const int e0 = (blockIdx.x * PX_THREADS + threadIdx.x) * 4;
  if (e0 >= I.hw) return;
  const RbState S = rb_state(const_cast<void*>(state), (size_t)n, T);
  const float wk = (float)S.ws[(size_t)T * n + k], kappa = S.scal[0], inv2var = S.scal[1];
  float y[4], e[4], o[4];
  bool part[4];
  const size_t base = (size_t)k * I.hw;
  rb_load<VEC>(I, base, e0, y, e, part);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v = 0.f;
    if (part[j]) v = both ? wk * rb_posterior(e[j] * e[j], kappa, inv2var) : wk;
    o[j] = v;
  }
  px_store4<VEC>(out, base + e0, I.hw - e0 < 4 ? I.hw - e0 : 4, o);
}

// what estep and weights share: sizes, pointers, options, the state and its alignment
int rb_check_pixels(const float* y, const float* s, const float* sw, float min_weight, int n, int h, int w, int n_em,
                    const void* state, size_t state_bytes) {
  if (n <= 0 || h <= 0 || w <= 0 || n_em < 1 || n_em > FSG_SOLVER_MAX_ITER) return FSG_E_BADARG;
  if (!y || !s || !state) return FSG_E_BADARG;
  if (!(min_weight >= 0.f)) return FSG_E_BADARG;  // negative or NaN
  const int rc = px_check_shape(n, h, w);
  if (rc) return rc;
  if (state_bytes < rb_state_bytes((size_t)n, n_em)) return FSG_E_BADARG;
  if (((uintptr_t)y & 3) || ((uintptr_t)s & 3) || ((uintptr_t)sw & 3)) return FSG_E_ALIGN;
  if ((uintptr_t)state & 7) return FSG_E_ALIGN;
  return 0;
}

// `p` shares a byte with one of the pixel arrays of a call or with the state
bool rb_hits_inputs(const void* p, size_t bytes, const RbIn& I, size_t pix, const void* state, size_t state_bytes) {
  return px_hits(p, bytes, {{I.y, pix * 4}, {I.s, pix * 4}, {I.sw, pix * 4}, {I.mask, pix}, {state, state_bytes}});
}

}  // namespace

extern "C" {

size_t fsg_robust_ws_bytes(int n, int h, int w) {
  if (px_check_shape(n, h, w)) return 0;
  return (size_t)n * (size_t)px_chunks(h, w) * PX_SLOTS * sizeof(float);
}

size_t fsg_robust_state_bytes(int n, int n_em) {
  if (n <= 0 || n_em < 1 || n_em > FSG_SOLVER_MAX_ITER) return 0;
  return rb_state_bytes((size_t)n, n_em);
}

int fsg_robust_estep_f32(const float* y, const float* s, const uint8_t* slices_mask, const float* sim_weight, float min_weight,
                         int n, int h, int w, int t, int n_em, const void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                         void* stream) {
  // every refusal comes before the first write
  const int rc = rb_check_pixels(y, s, sim_weight, min_weight, n, h, w, n_em, state, state_bytes);
  if (rc) return rc;
  if (t < 0 || t > n_em) return FSG_E_BADARG;
  if (!ws || ws_bytes < fsg_robust_ws_bytes(n, h, w)) return FSG_E_BADARG;
  if ((uintptr_t)ws & 7) return FSG_E_ALIGN;
  const RbIn I{y, s, slices_mask, sim_weight, min_weight, h * w};
  if (rb_hits_inputs(ws, fsg_robust_ws_bytes(n, h, w), I, (size_t)n * h * w, state, rb_state_bytes((size_t)n, n_em))) return FSG_E_BADARG;
  const dim3 grid((unsigned)px_chunks(h, w), (unsigned)n);
  hipStream_t st = fsg_stream(stream);
  if (px_vec(I.hw, {y, s, sim_weight}, slices_mask))
    hipLaunchKernelGGL(rb_estep_kernel<true>, grid, dim3(PX_THREADS), 0, st, I, n, n_em, t == 0 ? 1 : 0, state, (float*)ws);
  else
    hipLaunchKernelGGL(rb_estep_kernel<false>, grid, dim3(PX_THREADS), 0, st, I, n, n_em, t == 0 ? 1 : 0, state, (float*)ws);
  FSG_RETURN_LAUNCH();
}

int fsg_robust_update_f32(void* state, size_t state_bytes, const void* ws, size_t ws_bytes, int n, int h, int w, int t, int n_em,
                          double c0, double sigma_floor, double slice_floor, int min_pixels, void* stream) {
  if (n <= 0 || h <= 0 || w <= 0 || n_em < 1 || n_em > FSG_SOLVER_MAX_ITER || t < 0 || t > n_em) return FSG_E_BADARG;
  const int rc = px_check_shape(n, h, w);
  if (rc) return rc;
  if (!state || !ws || state_bytes < rb_state_bytes((size_t)n, n_em) || ws_bytes < fsg_robust_ws_bytes(n, h, w)) return FSG_E_BADARG;
  if (!(c0 > 0.0 && c0 <= 1.0) || !(sigma_floor >= 0.0 && sigma_floor <= 1.7976931348623157e308) ||
      !(slice_floor >= 0.0 && slice_floor <= 1.7976931348623157e308) || min_pixels < 0)
    return FSG_E_BADARG;
  if (((uintptr_t)state & 7) || ((uintptr_t)ws & 7)) return FSG_E_ALIGN;
  if (fsg_overlap(state, rb_state_bytes((size_t)n, n_em), ws, fsg_robust_ws_bytes(n, h, w))) return FSG_E_BADARG;
  const RbOpts O{c0, sigma_floor, slice_floor, min_pixels};
  hipLaunchKernelGGL(rb_update_kernel, dim3(1), dim3(PX_THREADS), 0, fsg_stream(stream), state, (const float*)ws, px_chunks(h, w),
                     n, t, n_em, O);
  FSG_RETURN_LAUNCH();
}

int fsg_robust_weights_f32(const float* y, const float* s, const uint8_t* slices_mask, const float* sim_weight, float min_weight,
                           int n, int h, int w, int n_em, int level, const void* state, size_t state_bytes, float* out,
                           void* stream) {
  const int rc = rb_check_pixels(y, s, sim_weight, min_weight, n, h, w, n_em, state, state_bytes);
  if (rc) return rc;
  if (!out || (level != FSG_ROBUST_SLICE && level != FSG_ROBUST_BOTH)) return FSG_E_BADARG;
  if ((uintptr_t)out & 3) return FSG_E_ALIGN;
  const RbIn I{y, s, slices_mask, sim_weight, min_weight, h * w};
  const size_t pix = (size_t)n * h * w;
  if (rb_hits_inputs(out, pix * 4, I, pix, state, rb_state_bytes((size_t)n, n_em))) return FSG_E_BADARG;
  const dim3 grid((unsigned)px_chunks(h, w), (unsigned)n);
  hipStream_t st = fsg_stream(stream);
  if (px_vec(I.hw, {y, s, sim_weight, out}, slices_mask))
    hipLaunchKernelGGL(rb_weights_kernel<true>, grid, dim3(PX_THREADS), 0, st, I, n, n_em, level == FSG_ROBUST_BOTH ? 1 : 0, state, out);
  else
    hipLaunchKernelGGL(rb_weights_kernel<false>, grid, dim3(PX_THREADS), 0, st, I, n, n_em, level == FSG_ROBUST_BOTH ? 1 : 0, state,
                       out);
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
