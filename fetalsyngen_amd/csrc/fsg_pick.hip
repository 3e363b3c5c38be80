// fsg_pick.hip -- weighted random voxel picks of a mask, entirely on the device (fsg_voxel_pick_*, contract in fsg_hip.h).
//
// The stages pick "k distinct random voxels of a mask", uniformly or with a weight volume (BlurCortex).  The host draws
// m >= k uniforms; everything that is O(mask) happens here, and one copy of k + 2 words goes back:
//
//   (a) pick_bucket_kernel   one streaming pass: eligible count and float64 weight sum of every FSG_NZ_BUCKET-voxel bucket
//   (b) pick_scan_kernel     one workgroup: prefix of the bucket sums, then the bucket of every candidate by bisection
//   (c) pick_locate_kernel   one wave per candidate: re-reads its bucket, finds the voxel with the sums of (a)
//   (d) pick_dedup_kernel    one workgroup: the first k distinct candidates in candidate order, -1 padding
//
// Order of the float64 sums (fixed, so that (a) and (c) agree bit for bit and two runs give one answer): a bucket is 16
// chunks of 256 voxels; in a chunk, lane l of a wave owns voxels 4l .. 4l+3 and adds them in turn, the 64 lane sums are
// scanned by lane shifts, the 16 chunk totals are added in turn starting from 0.  Bucket sums are added in turn inside
// contiguous segments and the segment totals in turn again: both levels only ever add a non-negative term to a running
// sum, so the prefix is non-decreasing and an empty bucket never moves it.  No floating-point atomics anywhere.
#include "fsg_common.h"

namespace {

constexpr int PK_BUCKET = FSG_NZ_BUCKET;
constexpr int PK_CHUNK = 256;                     // voxels per wave step: 64 lanes x 4
constexpr int PK_NCHUNK = PK_BUCKET / PK_CHUNK;   // 16
constexpr int PK_MAX_M = 4096;
constexpr int PK_MAX_K = 1024;
constexpr int PK_SCAN_THREADS = 1024;

struct PickHead {   // start of the workspace
  double total;
  long long eligible;
  int last_bucket;  // last bucket with an eligible voxel, -1 if none
  int pad;
};

struct PickWs {
  PickHead* head;
  double* prefix;    // nb + 1: prefix[b] = sum of the buckets before b, prefix[nb] = total
  int32_t* counts;   // nb
  double* target;    // PK_MAX_M: u[q] * total
  int32_t* cbucket;  // PK_MAX_M
  long long* cand;   // PK_MAX_M
};

size_t pick_ws_layout(size_t n, void* base, PickWs* w) {
  const size_t nb = (n + PK_BUCKET - 1) / PK_BUCKET;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 15) & ~(size_t)15; return o; };
  const size_t o_head = take(sizeof(PickHead)), o_prefix = take(8 * (nb + 1)), o_counts = take(4 * (nb + 1));
  const size_t o_target = take(8 * (size_t)PK_MAX_M), o_cb = take(4 * (size_t)PK_MAX_M), o_cand = take(8 * (size_t)PK_MAX_M);
  if (w) {
    char* p = (char*)base;
    w->head = (PickHead*)(p + o_head);
    w->prefix = (double*)(p + o_prefix);
    w->counts = (int32_t*)(p + o_counts);
    w->target = (double*)(p + o_target);
    w->cbucket = (int32_t*)(p + o_cb);
    w->cand = (long long*)(p + o_cand);
  }
  return off;
}

template <typename T>
__device__ __forceinline__ bool pk_pred(T v, int mode, float value) {
  const float f = (float)v;
  return mode == 0 ? f > value : (mode == 1 ? f == value : f != value);
}

// the four voxels e .. e+3 of a lane: eligible weights (0 where the voxel does not count) and an eligibility mask.
// e is a multiple of 4; 16-byte (float) / 4-byte (uint8) loads when the base pointers allow and the quad is inside.
template <typename T>
__device__ __forceinline__ unsigned pk_load4(const T* __restrict__ pred, const float* __restrict__ weight, size_t n, size_t e,
                                             int mode, float value, bool vec, double w[4]) {
  T p[4];
  float x[4] = {1.f, 1.f, 1.f, 1.f};
  if (vec && e + 3 < n) {
    if constexpr (sizeof(T) == 4) {
      const float4 q = *reinterpret_cast<const float4*>(pred + e);
      p[0] = (T)q.x; p[1] = (T)q.y; p[2] = (T)q.z; p[3] = (T)q.w;
    } else {
      const uchar4 q = *reinterpret_cast<const uchar4*>(pred + e);
      p[0] = (T)q.x; p[1] = (T)q.y; p[2] = (T)q.z; p[3] = (T)q.w;
    }
    if (weight) {
      const float4 q = *reinterpret_cast<const float4*>(weight + e);
      x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = e + j < n;
      p[j] = in ? pred[e + j] : (T)0;
      x[j] = in ? (weight ? weight[e + j] : 1.f) : 0.f;  // outside: weight 0, never eligible
    }
  }
  unsigned mask = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool ok = pk_pred(p[j], mode, value) && x[j] > 0.f;  // NaN and negative weights count as 0
    w[j] = ok ? (double)x[j] : 0.0;
    mask |= ok ? (1u << j) : 0u;
  }
  return mask;
}

// inclusive scan over the 64 lanes by lane shifts (fixed order)
__device__ __forceinline__ double pk_wave_scan(double x, int lane) {
#pragma unroll
  for (int o = 1; o < FSG_WAVE; o <<= 1) {
    const double y = __shfl_up(x, o, FSG_WAVE);
    if (lane >= o) x += y;
  }
  return x;
}

// ---- (a) ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pick_bucket_kernel(const T* __restrict__ pred, const float* __restrict__ weight, size_t n,
                                                          int mode, float value, int vec, double* __restrict__ sums,
                                                          int32_t* __restrict__ counts) {
  __shared__ double csum[PK_NCHUNK];
  __shared__ int ccnt[PK_NCHUNK];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t base = (size_t)blockIdx.x * PK_BUCKET;
  for (int c = wave; c < PK_NCHUNK; c += 4) {
    double w[4];
    const unsigned mask = pk_load4(pred, weight, n, base + (size_t)c * PK_CHUNK + (size_t)lane * 4, mode, value, vec != 0, w);
    const double lane_sum = ((w[0] + w[1]) + w[2]) + w[3];
    const double incl = pk_wave_scan(lane_sum, lane);
    int cnt = __popc(mask);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, FSG_WAVE);
    if (lane == 63) { csum[c] = incl; ccnt[c] = cnt; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    int k = 0;
    for (int c = 0; c < PK_NCHUNK; ++c) { s += csum[c]; k += ccnt[c]; }
    sums[blockIdx.x] = s;   // sums = prefix + 1: (b) turns it into the prefix in place
    counts[blockIdx.x] = k;
  }
}

// ---- (b) ------------------------------------------------------------------------------------------------------------
// prefix[0] = 0, prefix[b + 1] = sum of buckets 0 .. b.  On entry prefix[b + 1] holds the sum of bucket b.
__global__ __launch_bounds__(PK_SCAN_THREADS) void pick_scan_kernel(PickWs W, int nb, const double* __restrict__ u, int m) {
  __shared__ double seg_sum[PK_SCAN_THREADS];
  __shared__ long long seg_cnt[PK_SCAN_THREADS];
  __shared__ int seg_last[PK_SCAN_THREADS];
  const int tid = threadIdx.x;
  const int L = (nb + PK_SCAN_THREADS - 1) / PK_SCAN_THREADS;  // buckets per segment
  const int b0 = tid * L, b1 = min(nb, b0 + L);
  double s = 0.0;
  long long c = 0;
  int last = -1;
  for (int b = b0; b < b1; ++b) {
    s += W.prefix[b + 1];
    const int k = W.counts[b];
    c += k;
    if (k > 0) last = b;
  }
  seg_sum[tid] = s; seg_cnt[tid] = c; seg_last[tid] = last;
  __syncthreads();
  if (tid == 0) {  // exclusive prefix of the segment totals, in turn
    double run = 0.0;
    long long crun = 0;
    int lrun = -1;
    for (int i = 0; i < PK_SCAN_THREADS; ++i) {
      const double v = seg_sum[i];
      seg_sum[i] = run;
      run += v;
      crun += seg_cnt[i];
      if (seg_last[i] >= 0) lrun = seg_last[i];
    }
    W.head->total = run;
    W.head->eligible = crun;
    W.head->last_bucket = lrun;
    W.prefix[0] = 0.0;
  }
  __syncthreads();
  const double start = seg_sum[tid];
  s = 0.0;
  for (int b = b0; b < b1; ++b) {  // same additions as above
    s += W.prefix[b + 1];
    W.prefix[b + 1] = start + s;
  }
  __threadfence_block();
  __syncthreads();
  const double total = W.head->total;
  const int lastb = W.head->last_bucket;
  for (int q = tid; q < m; q += PK_SCAN_THREADS) {
    const double t = u[q] * total;
    int lo = 0, hi = nb;  // first bucket whose inclusive prefix exceeds t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (W.prefix[mid + 1] > t) hi = mid; else lo = mid + 1;
    }
    W.target[q] = t;
    W.cbucket[q] = lo < nb ? lo : lastb;  // rounding left none: the last eligible voxel (lastb == -1: nothing is eligible)
  }
}

// ---- (c) ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void pick_locate_kernel(const T* __restrict__ pred, const float* __restrict__ weight, size_t n,
                                                         int mode, float value, int vec, PickWs W, int nb) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int b = W.cbucket[q];
  if (b < 0 || b >= nb) {
    if (lane == 0) W.cand[q] = -1;
    return;
  }
  const double t = W.target[q], start = W.prefix[b];
  const size_t base = (size_t)b * PK_BUCKET;
  double run = 0.0;      // sum of the chunks before this one, as (a) adds them
  long long mylast = -1; // last eligible voxel this lane has seen
  for (int c = 0; c < PK_NCHUNK; ++c) {
    const size_t e = base + (size_t)c * PK_CHUNK + (size_t)lane * 4;
    double w[4];
    const unsigned mask = pk_load4(pred, weight, n, e, mode, value, vec != 0, w);
    const double lane_sum = ((w[0] + w[1]) + w[2]) + w[3];
    const double incl = pk_wave_scan(lane_sum, lane);
    double excl = __shfl_up(incl, 1, FSG_WAVE);
    if (lane == 0) excl = 0.0;
    int hit = -1;
    double l = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      l += w[j];
      if ((mask >> j) & 1u) {
        mylast = (long long)(e + j);
        if (hit < 0 && start + (run + (excl + l)) > t) hit = j;
      }
    }
    const unsigned long long any = __ballot(hit >= 0);
    if (any) {
      if (lane == __ffsll((long long)any) - 1) W.cand[q] = (long long)(e + hit);
      return;
    }
    run += __shfl(incl, 63, FSG_WAVE);
  }
  // rounding left none in this bucket: its last eligible voxel
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long other = __shfl_xor(mylast, o, FSG_WAVE);
    mylast = other > mylast ? other : mylast;
  }
  if (lane == 0) W.cand[q] = mylast;
}

// ---- (d) ------------------------------------------------------------------------------------------------------------
// out[0] = eligible, out[1] = found, out[2 .. 2 + found) = the first k distinct candidates in candidate order, then -1
__global__ __launch_bounds__(1024) void pick_dedup_kernel(PickWs W, int m, int k, long long* __restrict__ out) {
  __shared__ long long cand[PK_MAX_M];
  __shared__ int wave_tot[16];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long eligible = W.head->eligible;
  for (int q = tid; q < m; q += 1024) cand[q] = eligible > 0 ? W.cand[q] : -1;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < m; base += 1024) {  // (uniform trip count: every thread reaches the barriers)
    const int q = base + tid;
    int keep = 0;
    long long v = -1;
    if (q < m) {
      v = cand[q];
      keep = v >= 0;
      for (int p = 0; keep && p < q; ++p) keep = cand[p] != v;
    }
    int x = keep;  // inclusive scan of the keep flags over the tile
#pragma unroll
    for (int o = 1; o < FSG_WAVE; o <<= 1) {
      const int y = __shfl_up(x, o, FSG_WAVE);
      if (lane >= o) x += y;
    }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    int before = carry;
    for (int w2 = 0; w2 < wave; ++w2) before += wave_tot[w2];
    const int pos = before + x - keep;
    if (keep && pos < k) out[2 + pos] = v;
    __syncthreads();
    if (tid == 1023) carry = before + x;
    __syncthreads();
  }
  const int found = carry < k ? carry : k;
  for (int i = found + tid; i < k; i += 1024) out[2 + i] = -1;
  if (tid == 0) { out[0] = eligible; out[1] = found; }
}

__global__ __launch_bounds__(256) void pick_empty_kernel(int k, long long* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k + 2) out[i] = i < 2 ? 0 : -1;
}

template <typename T>
int voxel_pick(const T* pred, size_t n, int mode, float value, const float* weight, const double* u, int m, int k,
               long long* out, void* ws, size_t ws_bytes, void* stream) {
  if (!u || !out || m <= 0 || k <= 0 || k > m || mode < 0 || mode > 2) return FSG_E_BADARG;
  if (m > PK_MAX_M || k > PK_MAX_K) return FSG_E_TOOBIG;
  if (n > ((size_t)1 << 36)) return FSG_E_TOOBIG;  // bucket numbers are int32
  hipStream_t st = fsg_stream(stream);
  if (n == 0) {
    hipLaunchKernelGGL(pick_empty_kernel, dim3((unsigned)((k + 2 + 255) / 256)), dim3(256), 0, st, k, out);
    FSG_RETURN_LAUNCH();
  }
  if (!pred || !ws || ((uintptr_t)ws & 15) || ws_bytes < pick_ws_layout(n, nullptr, nullptr)) return FSG_E_BADARG;
  PickWs W;
  pick_ws_layout(n, ws, &W);
  const int nb = (int)((n + PK_BUCKET - 1) / PK_BUCKET);
  const int vec = ((uintptr_t)pred % (sizeof(T) == 4 ? 16 : 4)) == 0 && (!weight || ((uintptr_t)weight % 16) == 0);
  hipLaunchKernelGGL(pick_bucket_kernel<T>, dim3((unsigned)nb), dim3(256), 0, st, pred, weight, n, mode, value, vec, W.prefix + 1,
                     W.counts);
  hipLaunchKernelGGL(pick_scan_kernel, dim3(1), dim3(PK_SCAN_THREADS), 0, st, W, nb, u, m);
  hipLaunchKernelGGL(pick_locate_kernel<T>, dim3((unsigned)m), dim3(64), 0, st, pred, weight, n, mode, value, vec, W, nb);
  hipLaunchKernelGGL(pick_dedup_kernel, dim3(1), dim3(1024), 0, st, W, m, k, out);
  FSG_RETURN_LAUNCH();
}

}  // namespace

extern "C" {

size_t fsg_voxel_pick_ws_bytes(size_t n) { return pick_ws_layout(n, nullptr, nullptr); }

int fsg_voxel_pick_f32(const float* pred, size_t n, int mode, float value, const float* weight, const double* u, int m, int k,
                       long long* out, void* ws, size_t ws_bytes, void* stream) {
  return voxel_pick<float>(pred, n, mode, value, weight, u, m, k, out, ws, ws_bytes, stream);
}
int fsg_voxel_pick_u8(const uint8_t* pred, size_t n, int mode, float value, const float* weight, const double* u, int m, int k,
                      long long* out, void* ws, size_t ws_bytes, void* stream) {
  return voxel_pick<uint8_t>(pred, n, mode, value, weight, u, m, k, out, ws, ws_bytes, stream);
}

}  // extern "C"
