// fsg_imatch.hip -- slice intensity matching for srr: one scale and one smooth multiplicative bias field per acquired slice
// (the contract, the rule and the layout of the state block are in include/fsg_hip.h, fsg_imatch_*).
//
//   fsg_imatch_sums_f32   one streaming pass over y, s = A x (and bias0, the weights, the mask): per workgroup one partial of the
//                         five per-slice sums (count, sum omega c s, sum omega c c, min y, max y).
//   fsg_imatch_scale_f32  one workgroup: folds a slice's partials in double, the least-squares gain of every slice, the gauge
//                         (mean gain 1), the floor of the logarithm, the freeze.
//   fsg_imatch_bias_f32   three launches: the row pass forms P = omega log(d / s) and Q = omega on the fly and writes them blurred
//                         along the row; the column pass blurs an LDS tile with its halo along the column, divides, adds bias0
//                         and leaves one partial of the slice mean per tile; the third folds those in double.
//   fsg_imatch_apply_f32  the last pass: bias = b1 - mean, corrected = scale * expf(-bias) * y.
//
// MI355X shape of the work.  sums and apply are pure streaming: 256 threads that each own FOUR consecutive pixels of one slice,
// 16-byte loads where the pointers allow, the workgroup fold of fsg_common.h; their geometry, shape check, loads, stores and gate
// and the fold of a slice's partials (N, A, B, min y, max y, 0, 0, 0) are fsg_pixels.h's, shared with fsg_robust.hip.
// The row pass is a workgroup per 256 pixels of one row: its 256 + 2 Rr planes' values are formed once into 3 KiB of LDS (1.4 times the pixels at Rr = 48, 1.05 at Rr = 6), then
// 2 Rr + 1 LDS reads and fmafs per plane and pixel.  The column pass is a tile of 64 rows by 32 columns (a wave reads two runs of
// 128 bytes) with an Rr halo above and below over both planes in dynamic LDS, (64 + 2 Rr) * 32 * 8 bytes: 19 KiB at Rr = 6, 28 KiB
// at 24, 40 KiB at 48, so three to eight workgroups share a CU's 160 KiB; a thread walks 8 rows of its column.  Fusing the two
// passes would need a (T + 2 Rr)^2 tile of both planes: 128 KiB for T = 32 at Rr = 48, one workgroup a CU that computes nine
// times the pixels it keeps, hence two launches and 12 bytes a pixel of planes between them.  No atomics anywhere.
#include "fsg_pixels.h"
#include "fsg_sa.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int IM_THREADS = PX_THREADS;    // of the bias field's kernels too
constexpr int IM_MEAN_SLOTS = 2;          // floats of a partial of the means: sum omega b1, sum omega
constexpr int IM_ROW_W = 256;             // pixels of one row per workgroup of the row pass
constexpr int IM_TH = 64, IM_TW = 32;     // tile of the column pass
constexpr int IM_TROWS = IM_THREADS / IM_TW;  // thread rows of the column pass: a thread walks IM_TH / IM_TROWS rows
static_assert(IM_THREADS == SA_TILE * SA_TILE, "the column pass folds with sa_fold");

struct ImState {  // pointers into the state block for n slices; layout in fsg_hip.h, stated here once and measured by im_state_bytes
  double* consts;   // [4] R, floor, g, number of ok slices
  double* rows;     // [n][FSG_IMATCH_ROW]
  double* raw;      // [n]
  double* mean;     // [n]
  float* scale;     // [n]
  int32_t* ok;      // [n]
  int32_t* frozen;  // [1]
  void* end;
};

__host__ __device__ inline ImState im_state(void* p, size_t n) {
  ImState S;
  S.consts = (double*)p;
  S.rows = S.consts + 4;
  S.raw = S.rows + FSG_IMATCH_ROW * n;
  S.mean = S.raw + n;
  S.scale = (float*)(S.mean + n);
  S.ok = (int32_t*)(S.scale + n);
  S.frozen = S.ok + n;
  S.end = S.frozen + 1;
  return S;
}

inline size_t im_state_bytes(size_t n) { return fsg_carved_bytes(fsg_origin, im_state(fsg_origin, n).end); }
inline int im_tiles_x(int w) { return (w + IM_TW - 1) / IM_TW; }
inline int im_tiles_y(int h) { return (h + IM_TH - 1) / IM_TH; }
inline size_t im_sums_bytes(int n, int h, int w) { return (size_t)n * (size_t)px_chunks(h, w) * PX_SLOTS * sizeof(float); }
inline size_t im_means_bytes(int n, int h, int w) {
  return (size_t)n * (size_t)im_tiles_x(w) * (size_t)im_tiles_y(h) * IM_MEAN_SLOTS * sizeof(float);
}

struct ImIn {
  const float* y;
  const float* s;
  const uint8_t* mask;
  const float* sw;
  const float* pw;
  const float* b0;
  float min_weight;
  int hw;
};

struct ImTaps {
  int R;
  float g[FSG_IMATCH_MAX_RADIUS + 1];
};

struct ImPix {
  float c, om;
  bool part;
};

// one pixel: c = fl(expf(-bias0) * y), omega, and whether it is in Omega
__device__ __forceinline__ ImPix im_pixel(const ImIn& I, float y, float s, bool mk, float sw, float pw, float b0) {
  ImPix p;
  p.c = I.b0 ? expf(-b0) * y : y;
  p.om = I.pw ? pw : 1.f;
  bool ok = px_gate(mk, I.sw != nullptr, sw, I.min_weight);
  ok = ok && fabsf(y) <= PX_FLT_MAX && fabsf(s) <= PX_FLT_MAX && fabsf(p.c) <= PX_FLT_MAX;
  if (I.pw) ok = ok && pw > 0.f && pw <= PX_FLT_MAX;
  p.part = ok;
  return p;
}

__device__ __forceinline__ ImPix im_pixel_at(const ImIn& I, size_t a, float& s) {
  s = I.s[a];
  return im_pixel(I, I.y[a], s, I.mask ? I.mask[a] != 0 : true, I.sw ? I.sw[a] : 0.f, I.pw ? I.pw[a] : 0.f, I.b0 ? I.b0[a] : 0.f);
}

template <bool VEC>
__global__ __launch_bounds__(IM_THREADS) void im_sums_kernel(ImIn I, float* __restrict__ ws) {
  __shared__ float red[IM_THREADS / FSG_WAVE][PX_SLOTS];
  const int k = blockIdx.y, tid = threadIdx.x;
  const int e0 = (blockIdx.x * IM_THREADS + tid) * 4;
  float v[FSG_IMATCH_ROW - 2] = {0.f, 0.f, 0.f};
  float mn = INFINITY, mx = -INFINITY;
  // no thread leaves before the fold
  if (e0 < I.hw) {
    const int cnt = I.hw - e0 < 4 ? I.hw - e0 : 4;
    const size_t a = (size_t)k * I.hw + e0;
    float y[4], s[4], sw[4] = {0.f, 0.f, 0.f, 0.f}, pw[4] = {0.f, 0.f, 0.f, 0.f}, b0[4] = {0.f, 0.f, 0.f, 0.f};
    px_load4<VEC>(I.y, a, cnt, y);
    px_load4<VEC>(I.s, a, cnt, s);
    if (I.sw) px_load4<VEC>(I.sw, a, cnt, sw);
    if (I.pw) px_load4<VEC>(I.pw, a, cnt, pw);
    if (I.b0) px_load4<VEC>(I.b0, a, cnt, b0);
    const uint32_t mk = px_mask4<VEC>(I.mask, a, cnt);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= cnt) continue;
      const ImPix p = im_pixel(I, y[j], s[j], px_mask_bit(mk, j), sw[j], pw[j], b0[j]);
      if (!p.part) continue;
      const float t = I.pw ? p.om * p.c : p.c;
      v[0] += 1.f;
      v[1] += t * s[j];
      v[2] += t * p.c;
      mn = fminf(mn, y[j]);
      mx = fmaxf(mx, y[j]);
    }
  }
  fsg_fold_sums_minmax<FSG_IMATCH_ROW - 2, PX_SLOTS, IM_THREADS>(v, mn, mx, red, ws + ((size_t)k * gridDim.x + blockIdx.x) * PX_SLOTS);
}

// One workgroup.  Phase A, a thread per slice: the row, own_k and raw_k.  Phase B, wave 0: R, the gauge (the wave-walk of
// rb_update_kernel: a lane loads one slice, the wave adds the 64 in index order) and the freeze.  Phase C, a thread per slice.
__global__ __launch_bounds__(IM_THREADS) void im_scale_kernel(void* state, const float* __restrict__ ws, int chunks, int n,
                                                              double log_floor, int min_pixels) {
  __shared__ double sh[2];  // frozen, g
  const ImState S = im_state(state, (size_t)n);
  const int tid = threadIdx.x;
  for (int k = tid; k < n; k += IM_THREADS) {
    double r[FSG_IMATCH_ROW - 2], mn, mx;
    const bool any = px_fold_slice(ws + (size_t)k * chunks * PX_SLOTS, chunks, r, mn, mx);
    double* row = S.rows + (size_t)k * FSG_IMATCH_ROW;
    const bool sums_ok = fsg_finite(r[1]) && fsg_finite(r[2]);
    row[0] = r[0];
    row[1] = sums_ok ? r[1] : 0.0;
    row[2] = sums_ok ? r[2] : 0.0;
    row[3] = mn;
    row[4] = mx;
    const double q = r[1] / r[2];
    const bool own = r[0] >= (double)min_pixels && any && sums_ok && r[1] > 0.0 && r[2] > 0.0 && fsg_finite(q);
    S.raw[k] = own ? q : 0.0;
    S.ok[k] = own ? 1 : 0;
  }
  __syncthreads();
  if (tid < FSG_WAVE) {
    double mn, mx;
    px_wave_range<FSG_IMATCH_ROW>(S.rows, n, mn, mx);
    const double R = mx - mn, floor_ = log_floor * R;
    double sum = 0.0, nok = 0.0;
    for (int base = 0; base < n; base += FSG_WAVE) {
      const int k = base + tid, cnt = n - base < FSG_WAVE ? n - base : FSG_WAVE;
      const bool in = k < n;
      const double lraw = in ? S.raw[k] : 0.0, lown = in && S.ok[k] != 0 ? 1.0 : 0.0;
      for (int j = 0; j < cnt; ++j) {
        const double raw = __shfl(lraw, j, FSG_WAVE), own = __shfl(lown, j, FSG_WAVE);
        if (own != 0.0) {
          sum = sum + raw;
          nok = nok + 1.0;
        }
      }
    }
    const double g = sum / nok;
    bool frozen = !(fsg_finite(R) && R > 0.0) || !fsg_finite(floor_) || !(nok > 0.0) || !(fsg_finite(g) && g > 0.0);
    int bad = 0;  // a scale that leaves fp32
    if (!frozen)
      for (int k = tid; k < n; k += FSG_WAVE) {
        const float sc = (float)(S.raw[k] / g);
        if (S.ok[k] != 0 && !(sc > 0.f && sc <= PX_FLT_MAX)) bad = 1;
      }
#pragma unroll
    for (int o = FSG_WAVE / 2; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, FSG_WAVE);
    frozen = frozen || bad != 0;
    if (tid == 0) {
      S.consts[0] = frozen ? 0.0 : R;
      S.consts[1] = frozen ? 0.0 : floor_;
      S.consts[2] = frozen ? 0.0 : g;
      S.consts[3] = frozen ? 0.0 : nok;
      S.frozen[0] = frozen ? 1 : 0;
      sh[0] = frozen ? 1.0 : 0.0;
      sh[1] = g;
    }
  }
  __syncthreads();
  const bool frozen = sh[0] != 0.0;
  const double g = sh[1];
  for (int k = tid; k < n; k += IM_THREADS) {
    const bool ok = S.ok[k] != 0 && !frozen;
    S.scale[k] = ok ? (float)(S.raw[k] / g) : 1.f;
    S.ok[k] = ok ? 1 : 0;
    S.mean[k] = 0.0;
  }
}

// Row pass: workgroup = IM_ROW_W pixels of row blockIdx.y of slice blockIdx.z.  P and Q of the run and its halo are formed into
// LDS (zeros outside the slice, which the tap loop never reads), then every thread blurs its pixel.
__global__ __launch_bounds__(IM_THREADS) void im_rows_kernel(ImIn I, ImTaps T, int h, int w, int n, const void* state,
                                                             float* __restrict__ P1, float* __restrict__ Q1, float* __restrict__ Q0) {
  __shared__ float sp[IM_ROW_W + 2 * FSG_IMATCH_MAX_RADIUS], sq[IM_ROW_W + 2 * FSG_IMATCH_MAX_RADIUS];
  __shared__ float tap[FSG_IMATCH_MAX_RADIUS + 1];
  const int k = blockIdx.z, i = blockIdx.y, j0 = blockIdx.x * IM_ROW_W, tid = threadIdx.x, R = T.R;
  const ImState S = im_state(const_cast<void*>(state), (size_t)n);
  const bool ok = S.ok[k] != 0;
  const float scale = S.scale[k], floor_ = (float)S.consts[1];
  if (tid <= R) tap[tid] = T.g[tid];
  const size_t rowbase = ((size_t)k * h + i) * w;
  for (int u = tid; u < IM_ROW_W + 2 * R; u += IM_THREADS) {
    const int j = j0 - R + u;
    float p = 0.f, q = 0.f;
    if (ok && j >= 0 && j < w) {
      float s;
      const ImPix x = im_pixel_at(I, rowbase + j, s);
      const float d = scale * x.c;
      if (x.part && d > floor_ && s > floor_) {
        const float r = logf(d / s);
        if (fabsf(r) <= PX_FLT_MAX) {
          p = I.pw ? x.om * r : r;
          q = x.om;
        }
      }
    }
    sp[u] = p;
    sq[u] = q;
  }
  __syncthreads();
  const int j = j0 + tid;
  if (j >= w) return;
  const int lo = -R > -j ? -R : -j, hi = R < w - 1 - j ? R : w - 1 - j;
  float ap = 0.f, aq = 0.f;
  for (int t = lo; t <= hi; ++t) {
    const float g = tap[t < 0 ? -t : t];
    ap = fmaf(g, sp[tid + R + t], ap);
    aq = fmaf(g, sq[tid + R + t], aq);
  }
  P1[rowbase + j] = ap;
  Q1[rowbase + j] = aq;
  Q0[rowbase + j] = sq[tid + R];
}

// Column pass: workgroup (16 x 16 threads, used as IM_TROWS rows of IM_TW) = the tile of IM_TH rows by IM_TW columns at
// (blockIdx.y, blockIdx.x) of slice blockIdx.z.  tile: [2][IM_TH + 2 R][IM_TW], P1 then Q1, zeros outside the slice.
__global__ __launch_bounds__(IM_THREADS) void im_cols_kernel(ImTaps T, const float* __restrict__ b0, int h, int w,
                                                             const float* __restrict__ P1, const float* __restrict__ Q1,
                                                             const float* __restrict__ Q0, float* __restrict__ bias,
                                                             float* __restrict__ ws) {
  extern __shared__ float tile[];
  __shared__ float tap[FSG_IMATCH_MAX_RADIUS + 1];
  __shared__ float red[SAB_WAVES * IM_MEAN_SLOTS];
  const int tid = sa_tid(), lx = tid % IM_TW, ly = tid / IM_TW, R = T.R, rows = IM_TH + 2 * R;
  const int k = blockIdx.z, i0 = blockIdx.y * IM_TH, j = blockIdx.x * IM_TW + lx;
  float* tp = tile;
  float* tq = tile + (size_t)rows * IM_TW;
  if (tid <= R) tap[tid] = T.g[tid];
  const size_t sbase = (size_t)k * h * w;
  for (int u = ly; u < rows; u += IM_TROWS) {
    const int i = i0 - R + u;
    float p = 0.f, q = 0.f;
    if (i >= 0 && i < h && j < w) {
      p = P1[sbase + (size_t)i * w + j];
      q = Q1[sbase + (size_t)i * w + j];
    }
    tp[u * IM_TW + lx] = p;
    tq[u * IM_TW + lx] = q;
  }
  __syncthreads();
  float v[IM_MEAN_SLOTS] = {0.f, 0.f};
  for (int m = 0; m < IM_TH / IM_TROWS; ++m) {
    const int li = ly + IM_TROWS * m, i = i0 + li;
    if (i >= h || j >= w) continue;
    const int lo = -R > -i ? -R : -i, hi = R < h - 1 - i ? R : h - 1 - i;
    float ap = 0.f, aq = 0.f;
    for (int t = lo; t <= hi; ++t) {
      const float g = tap[t < 0 ? -t : t];
      ap = fmaf(g, tp[(li + R + t) * IM_TW + lx], ap);
      aq = fmaf(g, tq[(li + R + t) * IM_TW + lx], aq);
    }
    const float inc = aq >= FLT_MIN ? ap / aq : 0.f;
    const size_t a = sbase + (size_t)i * w + j;
    const float b1 = b0 ? b0[a] + inc : inc;
    bias[a] = b1;
    const float om = Q0[a];
    if (om > 0.f) {  // Omega_b
      v[0] += om * b1;
      v[1] += om;
    }
  }
  sa_fold<IM_MEAN_SLOTS>(v, red, ws, k);
}

// a thread per slice: the tiles' partials in double in tile order
__global__ __launch_bounds__(IM_THREADS) void im_means_kernel(void* state, const float* __restrict__ ws, int tiles, int n) {
  const int k = blockIdx.x * IM_THREADS + threadIdx.x;
  if (k >= n) return;
  const ImState S = im_state(state, (size_t)n);
  const float* p = ws + (size_t)k * tiles * IM_MEAN_SLOTS;
  double num = 0.0, den = 0.0;
  for (int b = 0; b < tiles; ++b) {
    num = num + (double)p[(size_t)b * IM_MEAN_SLOTS];
    den = den + (double)p[(size_t)b * IM_MEAN_SLOTS + 1];
  }
  const double m = num / den;
  S.mean[k] = (S.ok[k] != 0 && den > 0.0 && fsg_finite(m)) ? m : 0.0;
}

template <bool VEC>
__global__ __launch_bounds__(IM_THREADS) void im_apply_kernel(const float* __restrict__ y, const float* __restrict__ b0, int with_bias,
                                                              int hw, int n, const void* state, float* bias,
                                                              float* __restrict__ corrected) {
  const int k = blockIdx.y;
  const int e0 = (blockIdx.x * IM_THREADS + threadIdx.x) * 4;
  if (e0 >= hw) return;
  const ImState S = im_state(const_cast<void*>(state), (size_t)n);
  const float scale = S.scale[k], m = (float)S.mean[k];
  const bool shift = with_bias && S.ok[k] != 0;
  const int cnt = hw - e0 < 4 ? hw - e0 : 4;
  const size_t a = (size_t)k * hw + e0;
  float yy[4], b[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
  px_load4<VEC>(y, a, cnt, yy);
  if (with_bias) px_load4<VEC>(bias, a, cnt, b);
  else if (b0) px_load4<VEC>(b0, a, cnt, b);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (shift) b[j] = b[j] - m;
    const float c = expf(-b[j]) * yy[j];
    o[j] = scale * c;
  }
  px_store4<VEC>(bias, a, cnt, b);
  px_store4<VEC>(corrected, a, cnt, o);
}

// what sums and bias share: sizes, the pixel arrays and their alignment
int im_check_pixels(const float* y, const float* s, const float* sw, float min_weight, const float* pw, const float* b0, int n,
                    int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0 || !y || !s) return FSG_E_BADARG;
  if (!(min_weight >= 0.f)) return FSG_E_BADARG;  // negative or NaN
  const int rc = px_check_shape(n, h, w);
  if (rc) return rc;
  if (((uintptr_t)y | (uintptr_t)s | (uintptr_t)sw | (uintptr_t)pw | (uintptr_t)b0) & 3) return FSG_E_ALIGN;
  return 0;
}

// `p` shares a byte with one of the six pixel arrays of a call
bool im_hits_inputs(const void* p, size_t bytes, const ImIn& I, size_t pix) {
  return px_hits(p, bytes, {{I.y, pix * 4}, {I.s, pix * 4}, {I.mask, pix}, {I.sw, pix * 4}, {I.pw, pix * 4}, {I.b0, pix * 4}});
}

}  // namespace

extern "C" {

size_t fsg_imatch_ws_bytes(int n, int h, int w) {
  if (px_check_shape(n, h, w)) return 0;
  return im_sums_bytes(n, h, w) + im_means_bytes(n, h, w);
}

size_t fsg_imatch_state_bytes(int n) {
  if (n <= 0 || n > 65535) return 0;
  return im_state_bytes((size_t)n);
}

size_t fsg_imatch_plane_bytes(int n, int h, int w) {
  if (px_check_shape(n, h, w)) return 0;
  return (size_t)n * (size_t)h * (size_t)w * 3 * sizeof(float);
}

int fsg_imatch_sums_f32(const float* y, const float* s, const uint8_t* slices_mask, const float* sim_weight, float min_weight,
                        const float* pix_weight, const float* bias0, int n, int h, int w, void* ws, size_t ws_bytes,
                        void* stream) {
  // every refusal comes before the first write
  const int rc = im_check_pixels(y, s, sim_weight, min_weight, pix_weight, bias0, n, h, w);
  if (rc) return rc;
  if (!ws || ws_bytes < fsg_imatch_ws_bytes(n, h, w)) return FSG_E_BADARG;
  if ((uintptr_t)ws & 7) return FSG_E_ALIGN;
  const ImIn I{y, s, slices_mask, sim_weight, pix_weight, bias0, min_weight, h * w};
  if (im_hits_inputs(ws, fsg_imatch_ws_bytes(n, h, w), I, (size_t)n * h * w)) return FSG_E_BADARG;
  const dim3 grid((unsigned)px_chunks(h, w), (unsigned)n);
  hipStream_t st = fsg_stream(stream);
  if (px_vec(h * w, {y, s, sim_weight, pix_weight, bias0}, slices_mask))
    hipLaunchKernelGGL(im_sums_kernel<true>, grid, dim3(IM_THREADS), 0, st, I, (float*)ws);
  else
    hipLaunchKernelGGL(im_sums_kernel<false>, grid, dim3(IM_THREADS), 0, st, I, (float*)ws);
  FSG_RETURN_LAUNCH();
}

int fsg_imatch_scale_f32(void* state, size_t state_bytes, const void* ws, size_t ws_bytes, int n, int h, int w, double log_floor,
                         int min_pixels, void* stream) {
  if (n <= 0 || h <= 0 || w <= 0 || !state || !ws) return FSG_E_BADARG;
  const int rc = px_check_shape(n, h, w);
  if (rc) return rc;
  if (state_bytes < im_state_bytes((size_t)n) || ws_bytes < fsg_imatch_ws_bytes(n, h, w)) return FSG_E_BADARG;
  if (!(log_floor >= 0.0 && log_floor <= 1.7976931348623157e308) || min_pixels < 0) return FSG_E_BADARG;
  if (((uintptr_t)state & 7) || ((uintptr_t)ws & 7)) return FSG_E_ALIGN;
  if (fsg_overlap(state, im_state_bytes((size_t)n), ws, fsg_imatch_ws_bytes(n, h, w))) return FSG_E_BADARG;
  hipLaunchKernelGGL(im_scale_kernel, dim3(1), dim3(IM_THREADS), 0, fsg_stream(stream), state, (const float*)ws, px_chunks(h, w), n,
                     log_floor, min_pixels);
  FSG_RETURN_LAUNCH();
}

int fsg_imatch_bias_f32(const float* y, const float* s, const uint8_t* slices_mask, const float* sim_weight, float min_weight,
                        const float* pix_weight, const float* bias0, double sigma, int n, int h, int w, void* state,
                        size_t state_bytes, void* planes, size_t plane_bytes, void* ws, size_t ws_bytes, float* bias,
                        void* stream) {
  const int rc = im_check_pixels(y, s, sim_weight, min_weight, pix_weight, bias0, n, h, w);
  if (rc) return rc;
  if (!state || !planes || !ws || !bias) return FSG_E_BADARG;
  if (h > 65535) return FSG_E_TOOBIG;  // the row pass has a workgroup row per slice row
  if (!(sigma > 0.0 && sigma <= 1.7976931348623157e308) || 3.0 * sigma > (double)FSG_IMATCH_MAX_RADIUS) return FSG_E_BADARG;
  const size_t pix = (size_t)n * h * w, stb = im_state_bytes((size_t)n), wsb = fsg_imatch_ws_bytes(n, h, w), plb = pix * 12;
  if (state_bytes < stb || ws_bytes < wsb || plane_bytes < plb) return FSG_E_BADARG;
  if (((uintptr_t)state & 7) || ((uintptr_t)ws & 7) || ((uintptr_t)planes & 15) || ((uintptr_t)bias & 3)) return FSG_E_ALIGN;
  const ImIn I{y, s, slices_mask, sim_weight, pix_weight, bias0, min_weight, h * w};
  const void* outs[4] = {state, planes, ws, bias};
  const size_t outb[4] = {stb, plb, wsb, pix * 4};
  for (int a = 0; a < 4; ++a) {
    if (im_hits_inputs(outs[a], outb[a], I, pix)) return FSG_E_BADARG;
    for (int b = a + 1; b < 4; ++b)
      if (fsg_overlap(outs[a], outb[a], outs[b], outb[b])) return FSG_E_BADARG;
  }
  ImTaps T;
  T.R = (int)ceil(3.0 * sigma);
  T.g[0] = 1.f;  // exp(-0), also for a sigma whose square underflows
  for (int t = 1; t <= FSG_IMATCH_MAX_RADIUS; ++t) T.g[t] = t <= T.R ? (float)exp(-(double)(t * t) / (2.0 * sigma * sigma)) : 0.f;
  float* P1 = (float*)planes;
  float* Q1 = P1 + pix;
  float* Q0 = Q1 + pix;
  float* wm = (float*)((char*)ws + im_sums_bytes(n, h, w));
  hipStream_t st = fsg_stream(stream);
  hipLaunchKernelGGL(im_rows_kernel, dim3((unsigned)((w + IM_ROW_W - 1) / IM_ROW_W), (unsigned)h, (unsigned)n), dim3(IM_THREADS), 0, st,
                     I, T, h, w, n, (const void*)state, P1, Q1, Q0);
  const size_t lds = (size_t)(IM_TH + 2 * T.R) * IM_TW * 2 * sizeof(float);
  hipLaunchKernelGGL(im_cols_kernel, dim3((unsigned)im_tiles_x(w), (unsigned)im_tiles_y(h), (unsigned)n), dim3(SA_TILE, SA_TILE), lds,
                     st, T, bias0, h, w, (const float*)P1, (const float*)Q1, (const float*)Q0, bias, wm);
  hipLaunchKernelGGL(im_means_kernel, dim3((unsigned)((n + IM_THREADS - 1) / IM_THREADS)), dim3(IM_THREADS), 0, st, state,
                     (const float*)wm, im_tiles_x(w) * im_tiles_y(h), n);
  FSG_RETURN_LAUNCH();
}

int fsg_imatch_apply_f32(const float* y, const float* bias0, int mode, int n, int h, int w, const void* state,
                         size_t state_bytes, float* bias, float* corrected, void* stream) {
  if (n <= 0 || h <= 0 || w <= 0 || !y || !state || !bias || !corrected) return FSG_E_BADARG;
  if (mode != FSG_IMATCH_SCALE_ONLY && mode != FSG_IMATCH_WITH_BIAS) return FSG_E_BADARG;
  const int rc = px_check_shape(n, h, w);
  if (rc) return rc;
  const size_t pix = (size_t)n * h * w, stb = im_state_bytes((size_t)n);
  if (state_bytes < stb) return FSG_E_BADARG;
  if (((uintptr_t)y | (uintptr_t)bias0 | (uintptr_t)bias | (uintptr_t)corrected) & 3) return FSG_E_ALIGN;
  if ((uintptr_t)state & 7) return FSG_E_ALIGN;
  for (const void* out : {(const void*)bias, (const void*)corrected})
    if (px_hits(out, pix * 4, {{y, pix * 4}, {bias0, pix * 4}, {state, stb}})) return FSG_E_BADARG;
  if (fsg_overlap(bias, pix * 4, corrected, pix * 4)) return FSG_E_BADARG;
  const dim3 grid((unsigned)px_chunks(h, w), (unsigned)n);
  hipStream_t st = fsg_stream(stream);
  const int with_bias = mode == FSG_IMATCH_WITH_BIAS ? 1 : 0;
  if (px_vec(h * w, {y, bias0, bias, corrected}, nullptr))
    hipLaunchKernelGGL(im_apply_kernel<true>, grid, dim3(IM_THREADS), 0, st, y, bias0, with_bias, h * w, n, state, bias, corrected);
  else
    hipLaunchKernelGGL(im_apply_kernel<false>, grid, dim3(IM_THREADS), 0, st, y, bias0, with_bias, h * w, n, state, bias, corrected);
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
