// fsg_cg.hip -- the vector half of a conjugate-gradient solve of (A^T P W A + mu I) x = A^T P W y + mu z.
//
// The operator half is fsg_slice_acq_forward_f32 / fsg_slice_acq_adjoint_f32 (or _det_f32); this unit holds what lies between
// two applications: the element-wise updates of x, r, p, q, the two dot products of an iteration, and the scalars alpha, beta.
// Every scalar lives in the device block `ws`, indexed by iteration, so the host never reads one and the loop is a fixed
// sequence of launches (include/fsg_hip.h states the layout, the dot-product order and the freeze rule).
//
// Element-wise arithmetic is fp32 with contraction off (the library's flag and fsg_common.h's pragma); dot products are
// summed in double from exact products.  No atomics, no grid barrier, no allocation, no host synchronisation.
// The iteration cap is the header's FSG_SOLVER_MAX_ITER; the overlap test and the measuring of `ws` are fsg_common.h's.
#include "fsg_common.h"
#include <initializer_list>

namespace {

constexpr int CG_THREADS = 256;

struct CgWs {  // pointers into `ws` for (blocks, K); cg_ws is the one statement of the layout here, cg_ws_bytes measures it
  double* rr;
  double* pq;
  double* part_rr;
  double* part_pq;
  float* alpha;
  float* beta;
  int32_t* frozen;
  void* end;  // one past frozen
};

__host__ __device__ inline unsigned cg_blocks(size_t n) {
  size_t b = (n + 1023) / 1024;
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return (unsigned)b;
}

__host__ __device__ inline CgWs cg_ws(void* ws, size_t n, int K) {
  const size_t s = (size_t)K + 1, b = cg_blocks(n);
  CgWs w;
  w.rr = (double*)ws;
  w.pq = w.rr + s;
  w.part_rr = w.pq + s;
  w.part_pq = w.part_rr + b;
  w.alpha = (float*)(w.part_pq + b);
  w.beta = w.alpha + s;
  w.frozen = (int32_t*)(w.beta + s);
  w.end = w.frozen + s;
  return w;
}

inline size_t cg_ws_bytes(size_t n, int K) { return fsg_carved_bytes(fsg_origin, cg_ws(fsg_origin, n, K).end); }

// ---- the dot-product order (a function of n alone) ------------------------------------------------------------------------
// Elements are dealt in groups of four: group g = e / 4 belongs to thread g % T of the launch (T = blocks * 256, thread id =
// block * 256 + thread), and a thread adds its products in increasing e, starting from +0.0.  Whether a group is loaded as one
// 16-byte word or as scalars (unaligned views, the tail group) does not change which thread adds what, nor in which order.
__device__ __forceinline__ double cg_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, FSG_WAVE);  // level o: s[i] = v[i] + v[i ^ o], the same bits in both lanes
  return v;
}

// the workgroup's partial: lanes by the butterfly, then the 4 waves in wave order through LDS; stored by thread 0
__device__ __forceinline__ void cg_store_partial(double acc, double* __restrict__ part) {
  __shared__ double red[CG_THREADS / FSG_WAVE];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  acc = cg_wave_sum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// every workgroup adds the `nb` partials of the PREVIOUS launch in index order, from +0.0: the same bits everywhere
__device__ __forceinline__ double cg_fold(const double* __restrict__ part, unsigned nb) {
  __shared__ double total;
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (unsigned b = 0; b < nb; ++b) s = s + part[b];
    total = s;
  }
  __syncthreads();
  return total;
}

template <bool VEC>
__device__ __forceinline__ void cg_load4(const float* __restrict__ a, size_t e, int cnt, float (&v)[4]) {
  if (VEC && cnt == 4) {
    const float4 t = *reinterpret_cast<const float4*>(a + e);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? a[e + j] : 0.f;
  }
}
template <bool VEC>
__device__ __forceinline__ void cg_store4(float* __restrict__ a, size_t e, int cnt, const float (&v)[4]) {
  if (VEC && cnt == 4) {
    *reinterpret_cast<float4*>(a + e) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) a[e + j] = v[j];
  }
}
// the 0/1 projection V, one byte per voxel; absent = all ones
template <bool VEC>
__device__ __forceinline__ void cg_mask4(const uint8_t* __restrict__ m, size_t e, int cnt, bool (&k)[4]) {
  if (!m) {
    k[0] = k[1] = k[2] = k[3] = true;
  } else if (VEC && cnt == 4) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(m + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = ((w >> (8 * j)) & 255u) != 0;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = j < cnt && m[e + j] != 0;
  }
}

// r = V(b + mu z) - V(t0 + mu x0), p = r, x = V x0 (or 0); partials of <r,r>
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void cg_init_kernel(const float* __restrict__ b, const float* __restrict__ z,
                                                             const float* __restrict__ t0, const float* __restrict__ x0,
                                                             const uint8_t* __restrict__ mask, float mu, size_t n, int K,
                                                             float* __restrict__ r, float* __restrict__ p,
                                                             float* __restrict__ x, void* ws) {
  const CgWs S = cg_ws(ws, n, K);
  const size_t ng = (n + 3) >> 2, T = (size_t)gridDim.x * CG_THREADS;
  double acc = 0.0;
  for (size_t g = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; g < ng; g += T) {
    const size_t e = g << 2;
    const int cnt = n - e < 4 ? (int)(n - e) : 4;
    float vb[4], vz[4], vt[4], vx[4], vr[4], xo[4];
    bool keep[4];
    cg_load4<VEC>(b, e, cnt, vb);
    cg_mask4<VEC>(mask, e, cnt, keep);
    if (z) cg_load4<VEC>(z, e, cnt, vz);
    if (x0) { cg_load4<VEC>(t0, e, cnt, vt); cg_load4<VEC>(x0, e, cnt, vx); }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a = z ? vb[j] + mu * vz[j] : vb[j];
      a = keep[j] ? a : 0.f;
      if (x0) {
        float c = vt[j] + mu * vx[j];
        c = keep[j] ? c : 0.f;
        a = a - c;
      }
      vr[j] = a;
      xo[j] = (x0 && keep[j]) ? vx[j] : 0.f;
      if (j < cnt) acc = acc + (double)a * (double)a;
    }
    cg_store4<VEC>(r, e, cnt, vr);
    cg_store4<VEC>(p, e, cnt, vr);
    cg_store4<VEC>(x, e, cnt, xo);
  }
  cg_store_partial(acc, S.part_rr);
}

// q = V(t + mu p) over t; partials of <p,q>.  k == 1: rr[0] and frozen[0] from the partials of the init launch.
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void cg_q_kernel(const float* __restrict__ p, float* __restrict__ t,
                                                          const uint8_t* __restrict__ mask, float mu, double tol, size_t n,
                                                          int k, int K, void* ws) {
  const CgWs S = cg_ws(ws, n, K);
  int frozen;
  if (k == 1) {
    const double rr0 = cg_fold(S.part_rr, gridDim.x);
    frozen = rr0 <= tol;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      S.rr[0] = rr0; S.frozen[0] = frozen;
      S.pq[0] = 0.0; S.alpha[0] = 0.f; S.beta[0] = 0.f;  // no iteration 0: the slots are zero, so the histories replay whole
    }
  } else {
    frozen = S.frozen[k - 1];
  }
  if (frozen) return;
  const size_t ng = (n + 3) >> 2, T = (size_t)gridDim.x * CG_THREADS;
  double acc = 0.0;
  for (size_t g = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; g < ng; g += T) {
    const size_t e = g << 2;
    const int cnt = n - e < 4 ? (int)(n - e) : 4;
    float vp[4], vt[4], vq[4];
    bool keep[4];
    cg_load4<VEC>(p, e, cnt, vp);
    cg_load4<VEC>(t, e, cnt, vt);
    cg_mask4<VEC>(mask, e, cnt, keep);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = vt[j] + mu * vp[j];
      vq[j] = keep[j] ? a : 0.f;
      if (j < cnt) acc = acc + (double)vp[j] * (double)vq[j];
    }
    cg_store4<VEC>(t, e, cnt, vq);
  }
  cg_store_partial(acc, S.part_pq);
}

// alpha[k] = (float)(rr[k-1] / pq[k]); x += alpha p; r -= alpha q (not stored on the last iteration); partials of the new <r,r>.
// The LAST iteration also carries the one application of x = max(x, 0) of FSG_CG_RELU: fused with the update, or on its own
// when the solve is frozen.
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void cg_step_kernel(const float* __restrict__ p, const float* __restrict__ q,
                                                             float* __restrict__ x, float* __restrict__ r, size_t n, int k,
                                                             int K, int flags, void* ws) {
  const CgWs S = cg_ws(ws, n, K);
  const bool last = k == K, relu = last && (flags & FSG_CG_RELU);
  const size_t ng = (n + 3) >> 2, T = (size_t)gridDim.x * CG_THREADS;
  bool frozen = S.frozen[k - 1] != 0;
  double pq = 0.0;
  if (!frozen) {
    pq = cg_fold(S.part_pq, gridDim.x);
    frozen = !(pq > 0.0);  // a NaN or a direction in the null space: nothing is updated
  }
  const float alpha = frozen ? 0.f : (float)(S.rr[k - 1] / pq);
  if (blockIdx.x == 0 && threadIdx.x == 0) { S.pq[k] = pq; S.alpha[k] = alpha; }
  if (frozen) {
    if (!relu) return;
    for (size_t g = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; g < ng; g += T) {
      const size_t e = g << 2;
      const int cnt = n - e < 4 ? (int)(n - e) : 4;
      float vx[4];
      cg_load4<VEC>(x, e, cnt, vx);
#pragma unroll
      for (int j = 0; j < 4; ++j) vx[j] = vx[j] > 0.f ? vx[j] : 0.f;
      cg_store4<VEC>(x, e, cnt, vx);
    }
    return;
  }
  double acc = 0.0;
  for (size_t g = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; g < ng; g += T) {
    const size_t e = g << 2;
    const int cnt = n - e < 4 ? (int)(n - e) : 4;
    float vp[4], vq[4], vx[4], vr[4];
    cg_load4<VEC>(p, e, cnt, vp);
    cg_load4<VEC>(q, e, cnt, vq);
    cg_load4<VEC>(x, e, cnt, vx);
    cg_load4<VEC>(r, e, cnt, vr);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xn = vx[j] + alpha * vp[j];
      if (relu) xn = xn > 0.f ? xn : 0.f;
      vx[j] = xn;
      vr[j] = vr[j] - alpha * vq[j];
      if (j < cnt) acc = acc + (double)vr[j] * (double)vr[j];
    }
    cg_store4<VEC>(x, e, cnt, vx);
    if (!last) cg_store4<VEC>(r, e, cnt, vr);
  }
  cg_store_partial(acc, S.part_rr);
}

// rr[k], beta[k] = (float)(rr[k] / rr[k-1]), frozen[k]; p = r + beta p unless frozen or the last iteration
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void cg_dir_kernel(const float* __restrict__ r, float* __restrict__ p, double tol,
                                                            size_t n, int k, int K, void* ws) {
  const CgWs S = cg_ws(ws, n, K);
  const double rr_old = S.rr[k - 1];
  bool frozen = S.frozen[k - 1] != 0 || !(S.pq[k] > 0.0);
  double rr = rr_old;
  float beta = 0.f;
  if (!frozen) {
    rr = cg_fold(S.part_rr, gridDim.x);
    beta = (float)(rr / rr_old);
    frozen = rr <= tol;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { S.rr[k] = rr; S.beta[k] = beta; S.frozen[k] = frozen ? 1 : 0; }
  if (frozen || k == K) return;
  const size_t ng = (n + 3) >> 2, T = (size_t)gridDim.x * CG_THREADS;
  for (size_t g = (size_t)blockIdx.x * CG_THREADS + threadIdx.x; g < ng; g += T) {
    const size_t e = g << 2;
    const int cnt = n - e < 4 ? (int)(n - e) : 4;
    float vr[4], vp[4];
    cg_load4<VEC>(r, e, cnt, vr);
    cg_load4<VEC>(p, e, cnt, vp);
#pragma unroll
    for (int j = 0; j < 4; ++j) vp[j] = vr[j] + beta * vp[j];
    cg_store4<VEC>(p, e, cnt, vp);
  }
}

// 0 = go on, 1 = nothing to do, < 0 = the refusal
int cg_check(size_t n, int k, int K, const void* ws, size_t ws_bytes) {
  if (K < 1 || K > FSG_SOLVER_MAX_ITER || k < 1 || k > K) return FSG_E_BADARG;
  if (n == 0) return 1;
  if (!ws || ws_bytes < cg_ws_bytes(n, K)) return FSG_E_BADARG;
  if ((uintptr_t)ws & 7) return FSG_E_ALIGN;
  return 0;
}

bool cg_vec(std::initializer_list<const void*> f32s, const void* mask) {
  uintptr_t a = 0;
  for (const void* p : f32s) a |= (uintptr_t)p;
  return (a & 15) == 0 && ((uintptr_t)mask & 3) == 0;
}

}  // namespace

extern "C" {

size_t fsg_cg_ws_bytes(size_t n, int n_iter) {
  if (n_iter < 1 || n_iter > FSG_SOLVER_MAX_ITER) return 0;
  return cg_ws_bytes(n, n_iter);
}

int fsg_cg_init_f32(const float* b, const float* z, const float* t0, const float* x0, const uint8_t* mask, float mu, size_t n,
                    int n_iter, float* r, float* p, float* x, void* ws, size_t ws_bytes, void* stream) {
  const int c = cg_check(n, 1, n_iter, ws, ws_bytes);
  if (c) return c < 0 ? c : 0;
  if (!b || !r || !p || !x || (x0 && !t0)) return FSG_E_BADARG;
  if (!x0) t0 = nullptr;
  const size_t nb = n * sizeof(float);
  const void* ins[5] = {b, z, t0, x0, mask};
  float* outs[3] = {r, p, x};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 5; ++i)
      if (fsg_overlap(outs[o], nb, ins[i], i == 4 ? n : nb)) return FSG_E_BADARG;
    for (int o2 = o + 1; o2 < 3; ++o2)
      if (fsg_overlap(outs[o], nb, outs[o2], nb)) return FSG_E_BADARG;
    if (fsg_overlap(outs[o], nb, ws, ws_bytes)) return FSG_E_BADARG;
  }
  const dim3 grid(cg_blocks(n)), block(CG_THREADS);
  if (cg_vec({b, z, t0, x0, r, p, x}, mask))
    hipLaunchKernelGGL(cg_init_kernel<true>, grid, block, 0, fsg_stream(stream), b, z, t0, x0, mask, mu, n, n_iter, r, p, x, ws);
  else
    hipLaunchKernelGGL(cg_init_kernel<false>, grid, block, 0, fsg_stream(stream), b, z, t0, x0, mask, mu, n, n_iter, r, p, x, ws);
  FSG_RETURN_LAUNCH();
}

int fsg_cg_q_f32(const float* p, float* t, const uint8_t* mask, float mu, double tol, size_t n, int k, int n_iter, void* ws,
                 size_t ws_bytes, void* stream) {
  const int c = cg_check(n, k, n_iter, ws, ws_bytes);
  if (c) return c < 0 ? c : 0;
  if (!p || !t) return FSG_E_BADARG;
  const size_t nb = n * sizeof(float);
  if (fsg_overlap(t, nb, p, nb) || fsg_overlap(t, nb, mask, n) || fsg_overlap(t, nb, ws, ws_bytes)) return FSG_E_BADARG;
  const dim3 grid(cg_blocks(n)), block(CG_THREADS);
  if (cg_vec({p, t}, mask))
    hipLaunchKernelGGL(cg_q_kernel<true>, grid, block, 0, fsg_stream(stream), p, t, mask, mu, tol, n, k, n_iter, ws);
  else
    hipLaunchKernelGGL(cg_q_kernel<false>, grid, block, 0, fsg_stream(stream), p, t, mask, mu, tol, n, k, n_iter, ws);
  FSG_RETURN_LAUNCH();
}

int fsg_cg_step_f32(const float* p, const float* q, float* x, float* r, size_t n, int k, int n_iter, int flags, void* ws,
                    size_t ws_bytes, void* stream) {
  const int c = cg_check(n, k, n_iter, ws, ws_bytes);
  if (c) return c < 0 ? c : 0;
  if (!p || !q || !x || !r || (flags & ~FSG_CG_RELU)) return FSG_E_BADARG;
  const size_t nb = n * sizeof(float);
  float* outs[2] = {x, r};
  for (int o = 0; o < 2; ++o)
    if (fsg_overlap(outs[o], nb, p, nb) || fsg_overlap(outs[o], nb, q, nb) || fsg_overlap(outs[o], nb, ws, ws_bytes))
      return FSG_E_BADARG;
  if (fsg_overlap(x, nb, r, nb)) return FSG_E_BADARG;
  const dim3 grid(cg_blocks(n)), block(CG_THREADS);
  if (cg_vec({p, q, x, r}, nullptr))
    hipLaunchKernelGGL(cg_step_kernel<true>, grid, block, 0, fsg_stream(stream), p, q, x, r, n, k, n_iter, flags, ws);
  else
    hipLaunchKernelGGL(cg_step_kernel<false>, grid, block, 0, fsg_stream(stream), p, q, x, r, n, k, n_iter, flags, ws);
  FSG_RETURN_LAUNCH();
}

int fsg_cg_dir_f32(const float* r, float* p, double tol, size_t n, int k, int n_iter, void* ws, size_t ws_bytes, void* stream) {
  const int c = cg_check(n, k, n_iter, ws, ws_bytes);
  if (c) return c < 0 ? c : 0;
  if (!r || !p) return FSG_E_BADARG;
  const size_t nb = n * sizeof(float);
  if (fsg_overlap(p, nb, r, nb) || fsg_overlap(p, nb, ws, ws_bytes)) return FSG_E_BADARG;
  const dim3 grid(cg_blocks(n)), block(CG_THREADS);
  if (cg_vec({r, p}, nullptr))
    hipLaunchKernelGGL(cg_dir_kernel<true>, grid, block, 0, fsg_stream(stream), r, p, tol, n, k, n_iter, ws);
  else
    hipLaunchKernelGGL(cg_dir_kernel<false>, grid, block, 0, fsg_stream(stream), r, p, tol, n, k, n_iter, ws);
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
