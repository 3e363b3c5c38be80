// fsg_seedgen.hip -- seed generation: meta-label fusion + stable compaction, batched 1-D Gaussian-mixture EM, assignment.
//
// Replaces scripts/generate_seeds.py of the reference (label fusion :212-222, sklearn GaussianMixture.fit_predict per
// meta-label :199-209).  See DESIGN.md section 10 for the kernel forms and the determinism rule: every floating-point sum that
// feeds a result is reduced wave shuffle -> LDS -> per-block partial -> fixed-order sum in the finalising kernel; there are
// no atomics in this file.
#include "fsg_common.h"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_CHUNK = 4096;  // voxels per workgroup in fusion / compaction (16 per thread)
constexpr int EM_TILE = 4096;   // samples per workgroup per EM pass
constexpr int EM_KMAX = 16;
constexpr int EM_NSLOT = 3 * EM_KMAX + 1;  // S0[c], S1[c], S2[c], log-likelihood
constexpr int EM_JOBW = 8;                 // int64 words per job: xoff, n, k, blk0, nblk, max_iter, init_mode, pad (fsg_hip.h)
constexpr int EM_WINW = 4;                 // int64 words per assignment: job, out pointer, base value, first block

// ----------------------------------------------------------------------------------------------------------------------
// (a) meta-label fusion and stable compaction
// ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int sg_meta_of(const uint8_t* __restrict__ seg_u8, const float* __restrict__ seg_f32,
                                          const float* __restrict__ img, const uint8_t* __restrict__ table, int clear_label,
                                          size_t e, float& v) {
  v = img[e];
  if (v != v) v = 0.0f;  // NaN counts as 0
  int lab;
  if (seg_u8) {
    lab = seg_u8[e];
  } else {
    const float f = seg_f32[e];
    if (f != f) lab = 0;
    else if (f >= 0.0f && f <= 255.0f && f == truncf(f)) lab = (int)f;
    else return 0;  // not a label of any scheme: neither fused nor background
  }
  if (lab == clear_label) lab = 0;
  if (lab == 0) return v != 0.0f ? 4 : 0;
  const int m = table[lab];
  return m <= 4 ? m : 0;
}

__global__ __launch_bounds__(SG_THREADS) void sg_meta_count_kernel(const uint8_t* __restrict__ seg_u8, const float* __restrict__ seg_f32,
                                                                   const float* __restrict__ img, size_t n,
                                                                   const uint8_t* __restrict__ table, int clear_label,
                                                                   uint8_t* __restrict__ meta, uint32_t* __restrict__ blk_counts) {
  __shared__ uint8_t tab[256];
  __shared__ uint32_t red[4][2];
  tab[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * SG_CHUNK;
  uint32_t c12 = 0, c34 = 0;  // two 16-bit counters each (a workgroup sees 4096 voxels)
  for (int it = 0; it < SG_CHUNK / SG_THREADS; ++it) {
    const size_t e = base + (size_t)it * SG_THREADS + threadIdx.x;
    if (e < n) {
      float v;
      const int m = sg_meta_of(seg_u8, seg_f32, img, tab, clear_label, e, v);
      meta[e] = (uint8_t)m;
      c12 += (m == 1 ? 1u : 0u) + (m == 2 ? 0x10000u : 0u);
      c34 += (m == 3 ? 1u : 0u) + (m == 4 ? 0x10000u : 0u);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c12 += __shfl_xor(c12, o, FSG_WAVE);
    c34 += __shfl_xor(c34, o, FSG_WAVE);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { red[wave][0] = c12; red[wave][1] = c34; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t a = red[0][0] + red[1][0] + red[2][0] + red[3][0], b = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    uint32_t* o = blk_counts + (size_t)blockIdx.x * 4;
    o[0] = a & 0xFFFFu; o[1] = a >> 16; o[2] = b & 0xFFFFu; o[3] = b >> 16;
  }
}

// one workgroup: per-meta exclusive prefix over the per-block counts (in place), totals to counts4.  The packed arrays hold
// meta-label 1 first, then 2, 3, 4, so the offset written for (block, m) already includes the totals of the labels below m.
__global__ __launch_bounds__(SG_THREADS) void sg_scan_kernel(uint32_t* __restrict__ blk_counts, uint32_t nblk, uint32_t* __restrict__ counts4) {
  __shared__ uint32_t seg_sum[SG_THREADS][4];
  __shared__ uint32_t label_base[4];
  const uint32_t per = (nblk + SG_THREADS - 1) / SG_THREADS;
  const uint32_t b0 = threadIdx.x * per, b1 = min(b0 + per, nblk);
  uint32_t s[4] = {0, 0, 0, 0};
  for (uint32_t b = b0; b < b1; ++b)
    for (int m = 0; m < 4; ++m) s[m] += blk_counts[(size_t)b * 4 + m];
  for (int m = 0; m < 4; ++m) seg_sum[threadIdx.x][m] = s[m];
  __syncthreads();
  if (threadIdx.x < 4) {
    uint32_t run = 0;
    for (int t = 0; t < SG_THREADS; ++t) { const uint32_t v = seg_sum[t][threadIdx.x]; seg_sum[t][threadIdx.x] = run; run += v; }
    counts4[threadIdx.x] = run;
    label_base[threadIdx.x] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int m = 0; m < 4; ++m) { const uint32_t v = label_base[m]; label_base[m] = run; run += v; }
  }
  __syncthreads();
  for (int m = 0; m < 4; ++m) s[m] = seg_sum[threadIdx.x][m] + label_base[m];
  for (uint32_t b = b0; b < b1; ++b)
    for (int m = 0; m < 4; ++m) { const uint32_t v = blk_counts[(size_t)b * 4 + m]; blk_counts[(size_t)b * 4 + m] = s[m]; s[m] += v; }
}

// stable scatter: within a workgroup the voxels are visited 256 at a time in voxel order; a voxel's slot is the running count
// of its meta-label + the totals of the waves below + its rank among the lanes of its wave (ballot)
__global__ __launch_bounds__(SG_THREADS) void sg_pack_kernel(const uint8_t* __restrict__ meta, const float* __restrict__ img, size_t n,
                                                             const uint32_t* __restrict__ blk_off, float* __restrict__ packed_x,
                                                             int32_t* __restrict__ packed_idx) {
  __shared__ uint32_t wave_tot[4][4];
  const size_t base = (size_t)blockIdx.x * SG_CHUNK;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  uint32_t run[4];
  for (int m = 0; m < 4; ++m) run[m] = blk_off[(size_t)blockIdx.x * 4 + m];
  for (int it = 0; it < SG_CHUNK / SG_THREADS; ++it) {
    const size_t e = base + (size_t)it * SG_THREADS + threadIdx.x;
    const int mine = e < n ? meta[e] : 0;
    uint32_t rank = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const uint64_t bal = __ballot(mine == m + 1);
      if (mine == m + 1) rank = (uint32_t)__popcll(bal & below);
      if (lane == 0) wave_tot[wave][m] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if (mine) {
      uint32_t pos = (mine == 1 ? run[0] : mine == 2 ? run[1] : mine == 3 ? run[2] : run[3]) + rank;
      for (int w = 0; w < wave; ++w) pos += wave_tot[w][mine - 1];
      float v = img[e];
      if (v != v) v = 0.0f;
      packed_x[pos] = v;
      packed_idx[pos] = (int32_t)e;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) run[m] += wave_tot[0][m] + wave_tot[1][m] + wave_tot[2][m] + wave_tot[3][m];
    __syncthreads();
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// (b) batched 1-D EM
// ----------------------------------------------------------------------------------------------------------------------
// Per job and component the E-step reads four floats derived by the finalising kernel from the float64 parameters:
//   a = log w - 0.5 log(2 pi var),  b = 0.5 / var,  mu_hi + mu_lo = mu  (two floats: the mean to ~2^-48 relative, so that
//   x - mu is rounded once, relative to the difference, instead of carrying the absolute rounding of a float mean).
struct EmView {
  const int64_t* jobs;
  const double* tol;
  float* fp;          // [njobs][4][16]
  double* partials;   // [nblocks][49]
  int32_t* blk_job;   // [nblocks]
};

__global__ __launch_bounds__(64) void em_blockmap_kernel(const int64_t* __restrict__ jobs, int32_t* __restrict__ blk_job) {
  const int64_t* J = jobs + (size_t)blockIdx.x * EM_JOBW;
  const int64_t b0 = J[3], nb = J[4];
  for (int64_t b = threadIdx.x; b < nb; b += 64) blk_job[b0 + b] = (int32_t)blockIdx.x;
}

template <bool INIT>
__global__ __launch_bounds__(SG_THREADS) void em_estep_kernel(const float* __restrict__ xs, EmView V, const int32_t* __restrict__ status,
                                                              const double* __restrict__ params) {
  const int j = V.blk_job[blockIdx.x];
  const int64_t* J = V.jobs + (size_t)j * EM_JOBW;
  if (status[j * 4 + 2]) return;           // finished job: nothing to do
  if (INIT && J[6] == 0) return;            // parameters were given: no initial M-step
  const int k = (int)J[2];
  const int64_t n = J[1];
  const float* __restrict__ x = xs + J[0];
  const int64_t i0 = (int64_t)(blockIdx.x - J[3]) * EM_TILE;
  const int64_t i1 = min(i0 + (int64_t)EM_TILE, n);

  __shared__ float sa[EM_KMAX], sb[EM_KMAX], smh[EM_KMAX], sml[EM_KMAX];
  __shared__ double smu[EM_KMAX];
  __shared__ double red[4][EM_NSLOT];
  if (threadIdx.x < k) {
    const float* f = V.fp + (size_t)j * 4 * EM_KMAX;
    sa[threadIdx.x] = f[threadIdx.x];
    sb[threadIdx.x] = f[EM_KMAX + threadIdx.x];
    smh[threadIdx.x] = f[2 * EM_KMAX + threadIdx.x];
    sml[threadIdx.x] = f[3 * EM_KMAX + threadIdx.x];
    smu[threadIdx.x] = params[(size_t)j * 3 * EM_KMAX + EM_KMAX + threadIdx.x];  // pivot of the sums: the current mean
  }
  __syncthreads();

  double s0[EM_KMAX], s1[EM_KMAX], s2[EM_KMAX], ll = 0.0;
#pragma unroll
  for (int c = 0; c < EM_KMAX; ++c) { s0[c] = 0.0; s1[c] = 0.0; s2[c] = 0.0; }

  for (int64_t i = i0 + threadIdx.x; i < i1; i += SG_THREADS) {
    const float xv = x[i];
    const double xd = (double)xv;
    float lp[EM_KMAX];
    float mx = -INFINITY;
    int best = 0;
#pragma unroll
    for (int c = 0; c < EM_KMAX; ++c) {
      if (c < k) {
        const float d = (xv - smh[c]) - sml[c];
        lp[c] = INIT ? -fabsf(d) : sa[c] - d * d * sb[c];
        if (lp[c] > mx) { mx = lp[c]; best = c; }
      }
    }
    if (INIT) {
#pragma unroll
      for (int c = 0; c < EM_KMAX; ++c) {
        if (c < k && c == best) {
          const double dd = xd - smu[c];
          s0[c] += 1.0;
          s1[c] += dd;
          s2[c] += dd * dd;
        }
      }
    } else {
      float sum = 0.0f;
#pragma unroll
      for (int c = 0; c < EM_KMAX; ++c) {
        if (c < k) { lp[c] = expf(lp[c] - mx); sum += lp[c]; }
      }
      ll += (double)(mx + logf(sum));
      const float inv = 1.0f / sum;
#pragma unroll
      for (int c = 0; c < EM_KMAX; ++c) {
        if (c < k) {
          const double r = (double)(lp[c] * inv);
          const double dd = xd - smu[c];
          const double rd = r * dd;
          s0[c] += r;
          s1[c] += rd;
          s2[c] += rd * dd;
        }
      }
    }
  }

  // wave shuffles -> LDS -> one partial per workgroup; every step in a fixed order
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < EM_KMAX; ++c) {
    if (c < k) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        s0[c] += __shfl_xor(s0[c], o, FSG_WAVE);
        s1[c] += __shfl_xor(s1[c], o, FSG_WAVE);
        s2[c] += __shfl_xor(s2[c], o, FSG_WAVE);
      }
      if (lane == 0) { red[wave][c] = s0[c]; red[wave][EM_KMAX + c] = s1[c]; red[wave][2 * EM_KMAX + c] = s2[c]; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ll += __shfl_xor(ll, o, FSG_WAVE);
  if (lane == 0) red[wave][3 * EM_KMAX] = ll;
  __syncthreads();
  if (threadIdx.x < EM_NSLOT) {
    const int c = threadIdx.x % EM_KMAX;
    const bool live = threadIdx.x == 3 * EM_KMAX || c < k;
    const double v = live ? ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x] : 0.0;
    V.partials[(size_t)blockIdx.x * EM_NSLOT + threadIdx.x] = v;
  }
}

enum { EM_FIN_PREP = 0, EM_FIN_INIT = 1, EM_FIN_ITER = 2 };

__device__ __forceinline__ void em_derive(const double w, const double mu, const double var, float* __restrict__ f, int c) {
  f[c] = (float)(log(w) - 0.5 * log(6.283185307179586476925286766559 * var));
  f[EM_KMAX + c] = (float)(0.5 / var);
  const float hi = (float)mu;
  f[2 * EM_KMAX + c] = hi;
  f[3 * EM_KMAX + c] = (float)(mu - (double)hi);
}

// one workgroup per job: fixed-order sum of the job's partials, M-step, lower bound, stopping rule -- all on the device
__global__ __launch_bounds__(SG_THREADS) void em_finalize_kernel(EmView V, int mode, double* __restrict__ params, double* __restrict__ lb,
                                                                 int32_t* __restrict__ status) {
  const int j = blockIdx.x;
  const int64_t* J = V.jobs + (size_t)j * EM_JOBW;
  const int k = (int)J[2];
  const int64_t n = J[1];
  double* P = params + (size_t)j * 3 * EM_KMAX;
  float* f = V.fp + (size_t)j * 4 * EM_KMAX;
  if (mode == EM_FIN_PREP) {
    if (threadIdx.x < k) {
      const bool given = J[6] != 1;
      em_derive(given ? P[threadIdx.x] : 1.0, P[EM_KMAX + threadIdx.x], given ? P[2 * EM_KMAX + threadIdx.x] : 1.0, f, threadIdx.x);
    }
    if (threadIdx.x == 0) {
      lb[j] = -INFINITY;
      status[j * 4 + 0] = 0;
      status[j * 4 + 1] = 0;
      status[j * 4 + 2] = (n == 0 || J[6] == 2) ? 1 : 0;  // no samples, or a job that is only there to be assigned
      status[j * 4 + 3] = 0;
    }
    return;
  }
  if (status[j * 4 + 2]) return;
  if (mode == EM_FIN_INIT && J[6] == 0) return;

  __shared__ double part[4][EM_NSLOT];
  __shared__ double tot[EM_NSLOT];
  const int g = threadIdx.x >> 6, s = threadIdx.x & 63;
  if (s < EM_NSLOT) {
    double acc = 0.0;
    const double* p = V.partials + (size_t)J[3] * EM_NSLOT + s;
    for (int64_t b = g; b < J[4]; b += 4) acc += p[(size_t)b * EM_NSLOT];
    part[g][s] = acc;
  }
  __syncthreads();
  if (threadIdx.x < EM_NSLOT) tot[threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
  __syncthreads();
  if (threadIdx.x < k) {
    const int c = threadIdx.x;
    const double S0 = tot[c], S1 = tot[EM_KMAX + c], S2 = tot[2 * EM_KMAX + c];
    const double eps10 = 10.0 * 2.220446049250313e-16;
    const double nk = S0 + eps10;
    // new mean - previous mean.  sum r x / nk with nk = S0 + 10 eps is (S1 + mu_prev S0) / nk = mu_prev + (S1 - mu_prev 10 eps) / nk:
    // the second term is invisible for a live component and takes an empty one (S0 = 0) to mean 0, as sklearn's M-step does
    const double dlt = (S1 - P[EM_KMAX + c] * eps10) / nk;
    const double mu = P[EM_KMAX + c] + dlt;
    // sum r (x - mu_new)^2 from the sums taken about the previous mean
    const double ss = fmax((S2 - 2.0 * dlt * S1) + dlt * dlt * S0, 0.0);
    const double var = ss / nk + 1e-6;
    const double w = nk / (double)n;
    P[c] = w;
    P[EM_KMAX + c] = mu;
    P[2 * EM_KMAX + c] = var;
    em_derive(w, mu, var, f, c);
  }
  if (threadIdx.x == 0 && mode == EM_FIN_ITER) {
    const double now = tot[3 * EM_KMAX] / (double)n, prev = lb[j];
    const int it = status[j * 4 + 0] + 1;
    lb[j] = now;
    status[j * 4 + 0] = it;
    if (fabs(now - prev) < V.tol[j]) { status[j * 4 + 1] = 1; status[j * 4 + 2] = 1; }
    else if (it >= (int)J[5]) status[j * 4 + 2] = 1;
  }
}

// ----------------------------------------------------------------------------------------------------------------------
// (c) assignment: argmax of the weighted log-densities (the E-step's own float evaluation), renumbered by ascending mean
// ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SG_THREADS) void sg_assign_kernel(const float* __restrict__ xs, const int32_t* __restrict__ idx,
                                                               const int64_t* __restrict__ jobs, const int64_t* __restrict__ wins,
                                                               const int32_t* __restrict__ win_blk, const float* __restrict__ fp,
                                                               const double* __restrict__ params) {
  const int w = win_blk[blockIdx.x];
  const int64_t* W = wins + (size_t)w * EM_WINW;
  const int j = (int)W[0];
  const int64_t* J = jobs + (size_t)j * EM_JOBW;
  const int k = (int)J[2];
  const int64_t n = J[1];
  uint8_t* __restrict__ out = reinterpret_cast<uint8_t*>((uintptr_t)W[1]);
  const int base = (int)W[2];
  __shared__ float sa[EM_KMAX], sb[EM_KMAX], smh[EM_KMAX], sml[EM_KMAX];
  __shared__ int rank[EM_KMAX];
  if (threadIdx.x < k) {
    const float* f = fp + (size_t)j * 4 * EM_KMAX;
    sa[threadIdx.x] = f[threadIdx.x];
    sb[threadIdx.x] = f[EM_KMAX + threadIdx.x];
    smh[threadIdx.x] = f[2 * EM_KMAX + threadIdx.x];
    sml[threadIdx.x] = f[3 * EM_KMAX + threadIdx.x];
    const double* mu = params + (size_t)j * 3 * EM_KMAX + EM_KMAX;
    int r = 0;
    for (int c = 0; c < k; ++c) r += (mu[c] < mu[threadIdx.x] || (mu[c] == mu[threadIdx.x] && c < (int)threadIdx.x)) ? 1 : 0;
    rank[threadIdx.x] = r;
  }
  __syncthreads();
  const int64_t i0 = (int64_t)(blockIdx.x - W[3]) * EM_TILE;
  const int64_t i1 = min(i0 + (int64_t)EM_TILE, n);
  for (int64_t i = i0 + threadIdx.x; i < i1; i += SG_THREADS) {
    int best = 0;
    if (k > 1) {
      const float xv = xs[J[0] + i];
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < EM_KMAX; ++c) {
        if (c < k) {
          const float d = (xv - smh[c]) - sml[c];
          const float lp = sa[c] - d * d * sb[c];
          if (lp > mx) { mx = lp; best = c; }
        }
      }
      best = rank[best];
    }
    out[idx[J[0] + i]] = (uint8_t)(base + best);
  }
}

// the assignment's own block map: winner w owns blocks [first, first + the block count of its job)
__global__ __launch_bounds__(64) void sg_winmap_kernel(const int64_t* __restrict__ jobs, const int64_t* __restrict__ wins,
                                                       int32_t* __restrict__ win_blk) {
  const int64_t* W = wins + (size_t)blockIdx.x * EM_WINW;
  const int64_t b0 = W[3], nb = jobs[(size_t)W[0] * EM_JOBW + 4];
  for (int64_t b = threadIdx.x; b < nb; b += 64) win_blk[b0 + b] = (int32_t)blockIdx.x;
}

struct EmWork {
  int64_t* jobs;
  double* tol;
  float* fp;
  double* partials;
  int32_t* blk_job;
  int64_t* wins;
  int32_t* win_blk;
  size_t bytes;
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

EmWork em_carve(void* work, int njobs, int64_t nblocks) {
  EmWork W;
  char* p = (char*)work;
  size_t o = 0;
  W.jobs = (int64_t*)(p + o); o += up16((size_t)njobs * EM_JOBW * 8);
  W.tol = (double*)(p + o); o += up16((size_t)njobs * 8);
  W.fp = (float*)(p + o); o += up16((size_t)njobs * 4 * EM_KMAX * 4);
  W.partials = (double*)(p + o); o += up16((size_t)(nblocks > 0 ? nblocks : 1) * EM_NSLOT * 8);
  W.blk_job = (int32_t*)(p + o); o += up16((size_t)(nblocks > 0 ? nblocks : 1) * 4);
  W.wins = (int64_t*)(p + o); o += up16((size_t)njobs * EM_WINW * 8);
  W.win_blk = (int32_t*)(p + o); o += up16((size_t)(nblocks > 0 ? nblocks : 1) * 4);
  W.bytes = o;
  return W;
}

// host-side check of a job table; -> total workgroups, or a negative FSG_E_* code
int64_t em_check_jobs(const int64_t* jobs_host, int njobs, size_t nx) {
  if (!jobs_host || njobs < 1) return FSG_E_BADARG;
  int64_t blk = 0;
  for (int j = 0; j < njobs; ++j) {
    const int64_t* J = jobs_host + (size_t)j * EM_JOBW;
    if (J[2] < 1 || J[2] > EM_KMAX) return FSG_E_BADARG;               // k
    if (J[1] < 0 || (J[1] == 0 && J[2] > 1)) return FSG_E_BADARG;      // n
    if (J[1] > 0x7fffffffll) return FSG_E_TOOBIG;
    if (J[0] < 0 || (uint64_t)J[0] + (uint64_t)J[1] > (uint64_t)nx) return FSG_E_BADARG;  // the job must lie inside x
    if (J[5] < 1) return FSG_E_BADARG;                                 // max_iter
    if (J[6] < 0 || J[6] > 2) return FSG_E_BADARG;                     // init mode
    const int64_t nb = (J[1] + EM_TILE - 1) / EM_TILE;
    if (J[3] != blk || J[4] != nb) return FSG_E_BADARG;                // block ranges are consecutive and cover the job
    blk += nb;
    if (blk > 0x7fffffffll) return FSG_E_TOOBIG;
  }
  return blk;
}

}  // namespace

extern "C" {

size_t fsg_seed_meta_work_bytes(size_t n) { return ((n + SG_CHUNK - 1) / SG_CHUNK) * 4 * sizeof(uint32_t); }

int fsg_seed_meta_pack(const uint8_t* seg_u8, const float* seg_f32, const float* image, size_t n, const uint8_t* table256,
                       int clear_label, uint8_t* meta, uint32_t* counts4, float* packed_x, int32_t* packed_idx, void* work,
                       void* stream) {
  if ((!seg_u8 && !seg_f32) || (seg_u8 && seg_f32) || !image || !table256 || !meta || !counts4 || !packed_x || !packed_idx ||
      !work || n == 0 || clear_label < -1 || clear_label > 255)
    return FSG_E_BADARG;
  if (n > 0x7fffffffull) return FSG_E_TOOBIG;
  const unsigned nblk = (unsigned)((n + SG_CHUNK - 1) / SG_CHUNK);
  uint32_t* blk = (uint32_t*)work;
  hipStream_t s = fsg_stream(stream);
  hipLaunchKernelGGL(sg_meta_count_kernel, dim3(nblk), dim3(SG_THREADS), 0, s, seg_u8, seg_f32, image, n, table256, clear_label, meta, blk);
  hipLaunchKernelGGL(sg_scan_kernel, dim3(1), dim3(SG_THREADS), 0, s, blk, nblk, counts4);
  hipLaunchKernelGGL(sg_pack_kernel, dim3(nblk), dim3(SG_THREADS), 0, s, meta, image, n, blk, packed_x, packed_idx);
  FSG_RETURN_LAUNCH();
}

int fsg_em1d_tile(void) { return EM_TILE; }

size_t fsg_em1d_work_bytes(int njobs, int64_t nblocks) {
  if (njobs < 1 || nblocks < 0) return 0;
  return em_carve(nullptr, njobs, nblocks).bytes;
}

int fsg_em1d_fit(const float* x, size_t nx, int njobs, const int64_t* jobs_host, const double* tol_host, double* params,
                 double* lower_bound, int32_t* status, void* work, size_t work_bytes, void* stream) {
  if (!x || !tol_host || !params || !lower_bound || !status || !work) return FSG_E_BADARG;
  const int64_t nblocks = em_check_jobs(jobs_host, njobs, nx);
  if (nblocks < 0) return (int)nblocks;
  int64_t iters = 0;
  bool any_init = false;
  for (int j = 0; j < njobs; ++j) {
    if (!(tol_host[j] >= 0.0)) return FSG_E_BADARG;
    const int64_t* J = jobs_host + (size_t)j * EM_JOBW;
    if (J[6] != 2 && J[1] > 0 && J[5] > iters) iters = J[5];
    any_init = any_init || (J[6] == 1 && J[1] > 0);
  }
  const EmWork W = em_carve(work, njobs, nblocks);
  if (work_bytes < W.bytes || (((uintptr_t)work) & 15)) return FSG_E_BADARG;
  hipStream_t s = fsg_stream(stream);
  hipError_t e = hipMemcpyAsync(W.jobs, jobs_host, (size_t)njobs * EM_JOBW * 8, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyAsync(W.tol, tol_host, (size_t)njobs * 8, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return (int)e;
  EmView V{W.jobs, W.tol, W.fp, W.partials, W.blk_job};
  hipLaunchKernelGGL(em_blockmap_kernel, dim3(njobs), dim3(64), 0, s, W.jobs, W.blk_job);
  hipLaunchKernelGGL(em_finalize_kernel, dim3(njobs), dim3(SG_THREADS), 0, s, V, (int)EM_FIN_PREP, params, lower_bound, status);
  if (nblocks > 0) {
    if (any_init) {
      hipLaunchKernelGGL(em_estep_kernel<true>, dim3((unsigned)nblocks), dim3(SG_THREADS), 0, s, x, V, status, params);
      hipLaunchKernelGGL(em_finalize_kernel, dim3(njobs), dim3(SG_THREADS), 0, s, V, (int)EM_FIN_INIT, params, lower_bound, status);
    }
    for (int64_t it = 0; it < iters; ++it) {
      hipLaunchKernelGGL(em_estep_kernel<false>, dim3((unsigned)nblocks), dim3(SG_THREADS), 0, s, x, V, status, params);
      hipLaunchKernelGGL(em_finalize_kernel, dim3(njobs), dim3(SG_THREADS), 0, s, V, (int)EM_FIN_ITER, params, lower_bound, status);
    }
  }
  FSG_RETURN_LAUNCH();
}

int fsg_seed_assign(const float* x, size_t nx, const int32_t* idx, int njobs, const int64_t* jobs_host, int nwin,
                    const int64_t* wins_host, const double* params, void* work, size_t work_bytes, void* stream) {
  if (!x || !idx || !params || !work || !wins_host || nwin < 1) return FSG_E_BADARG;
  const int64_t nblocks = em_check_jobs(jobs_host, njobs, nx);
  if (nblocks < 0) return (int)nblocks;
  if (nwin > njobs) return FSG_E_BADARG;
  int64_t blk = 0;
  for (int w = 0; w < nwin; ++w) {
    const int64_t* Wn = wins_host + (size_t)w * EM_WINW;
    if (Wn[0] < 0 || Wn[0] >= njobs || Wn[1] == 0 || Wn[2] < 0 || Wn[2] + jobs_host[(size_t)Wn[0] * EM_JOBW + 2] > 256) return FSG_E_BADARG;
    if (Wn[3] != blk) return FSG_E_BADARG;
    blk += jobs_host[(size_t)Wn[0] * EM_JOBW + 4];
  }
  if (blk > nblocks) return FSG_E_BADARG;  // the block map was sized for the fit
  const EmWork W = em_carve(work, njobs, nblocks);
  if (work_bytes < W.bytes || (((uintptr_t)work) & 15)) return FSG_E_BADARG;
  if (blk == 0) return 0;
  hipStream_t s = fsg_stream(stream);
  hipError_t e = hipMemcpyAsync(W.wins, wins_host, (size_t)nwin * EM_WINW * 8, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyAsync(W.jobs, jobs_host, (size_t)njobs * EM_JOBW * 8, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sg_winmap_kernel, dim3(nwin), dim3(64), 0, s, W.jobs, W.wins, W.win_blk);
  hipLaunchKernelGGL(sg_assign_kernel, dim3((unsigned)blk), dim3(SG_THREADS), 0, s, x, idx, W.jobs, W.wins, W.win_blk, W.fp, params);
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
