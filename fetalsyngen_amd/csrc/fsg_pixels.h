// fsg_pixels.h -- what the streaming pixel passes of fsg_robust.hip and fsg_imatch.hip share (rb_estep_kernel,
// rb_weights_kernel, im_sums_kernel, im_apply_kernel) and the opening of their one-workgroup scalar passes (rb_update_kernel,
// im_scale_kernel).  A workgroup is PX_THREADS threads that each own FOUR consecutive pixels of one slice; it leaves one partial
// of PX_SLOTS floats (fsg_fold_sums_minmax of fsg_common.h: the sums, min y, max y, zeros), and the scalar pass adds a slice's
// partials in double in chunk order.  Every order of addition here is part of the units' contract.
#pragma once
#include <initializer_list>
#include <utility>
#include "fsg_common.h"

constexpr int PX_THREADS = 256;
constexpr int PX_CHUNK = 4 * PX_THREADS;  // pixels of one slice per workgroup
constexpr int PX_SLOTS = 8;               // floats of a partial
constexpr float PX_FLT_MAX = 3.402823466e+38f;

static inline int px_chunks(int h, int w) { return (int)(((size_t)h * (size_t)w + PX_CHUNK - 1) / PX_CHUNK); }

// the shapes the streaming passes take: slices on grid.y, pixel offsets in 32 bits
static inline int px_check_shape(int n, int h, int w) {
  if (n <= 0 || h <= 0 || w <= 0) return FSG_E_BADARG;
  if (n > 65535 || (size_t)n * (size_t)h * (size_t)w > (size_t)0x7FFFFFFF) return FSG_E_TOOBIG;
  // a thread's first pixel, (workgroup * PX_THREADS + thread) * 4, is an int: that of the last workgroup's last thread stays
  // representable
  if ((size_t)h * (size_t)w > (size_t)0x7FFFFFFF - PX_CHUNK) return FSG_E_TOOBIG;
  return 0;
}

// the 16-byte path: whole groups of four, every fp32 array present on 16 bytes, the mask on 4
static inline bool px_vec(int hw, std::initializer_list<const void*> f32, const uint8_t* mask) {
  uintptr_t bits = 0;
  for (const void* p : f32) bits |= (uintptr_t)p;
  return hw % 4 == 0 && !(bits & 15) && !((uintptr_t)mask & 3);
}

// [p, p + bytes) shares a byte with one of the arrays `in`, each (pointer, bytes)
static inline bool px_hits(const void* p, size_t bytes, std::initializer_list<std::pair<const void*, size_t>> in) {
  for (const auto& q : in)
    if (fsg_overlap(p, bytes, q.first, q.second)) return true;
  return false;
}

// The four pixels at p[a..a+3] of which `cnt` lie in the slice; VEC: cnt == 4 and p + a is on 16 bytes.  No address is formed
// past the end of the slice; a pixel there reads as 0.
template <bool VEC>
__device__ __forceinline__ void px_load4(const float* __restrict__ p, size_t a, int cnt, float (&v)[4]) {
  if (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(p + a);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[a + j] : 0.f;
  }
}

template <bool VEC>
__device__ __forceinline__ void px_store4(float* __restrict__ p, size_t a, int cnt, const float (&v)[4]) {
  if (VEC) {
    *reinterpret_cast<float4*>(p + a) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) p[a + j] = v[j];
  }
}

// the four mask bytes as one word, byte j non-zero iff pixel j is set; an absent mask sets all four
template <bool VEC>
__device__ __forceinline__ uint32_t px_mask4(const uint8_t* __restrict__ mask, size_t a, int cnt) {
  if (!mask) return 0x01010101u;
  if (VEC) return *reinterpret_cast<const uint32_t*>(mask + a);
  uint32_t mk = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < cnt && mask[a + j] != 0) mk |= 1u << (8 * j);
  return mk;
}
__device__ __forceinline__ bool px_mask_bit(uint32_t mk, int j) { return ((mk >> (8 * j)) & 255u) != 0; }

// the gate of a pixel before the unit's own finiteness rule: the mask, and where sim_weight is given weight > 0 and
// >= min_weight (a NaN weight takes no part)
__device__ __forceinline__ bool px_gate(bool mk, bool has_sw, float sw, float min_weight) {
  bool ok = mk;
  if (has_sw) ok = ok && sw > 0.f && sw >= min_weight;
  return ok;
}

// Phase A of the scalar passes, a thread per slice: the slice's NS sums, min y and max y from its `chunks` partials at p, in
// double, in chunk order.  -> the slice has a pixel; without one mn = mx = 0, so that no Inf is stored.
template <int NS>
__device__ __forceinline__ bool px_fold_slice(const float* __restrict__ p, int chunks, double (&r)[NS], double& mn, double& mx) {
#pragma unroll
  for (int j = 0; j < NS; ++j) r[j] = 0.0;
  mn = INFINITY;
  mx = -INFINITY;
  for (int b = 0; b < chunks; ++b) {
#pragma unroll
    for (int j = 0; j < NS; ++j) r[j] = r[j] + (double)p[(size_t)b * PX_SLOTS + j];
    mn = fmin(mn, (double)p[(size_t)b * PX_SLOTS + NS]);
    mx = fmax(mx, (double)p[(size_t)b * PX_SLOTS + NS + 1]);
  }
  const bool any = r[0] > 0.0;
  if (!any) mn = mx = 0.0;
  return any;
}

// Wave 0, all 64 lanes: min and max of y over the slices that have a pixel, from their rows of ROW doubles (count first, min
// and max last); every lane gets both.  Min and max do not depend on the order.
template <int ROW>
__device__ __forceinline__ void px_wave_range(const double* rows, int n, double& mn, double& mx) {
  mn = INFINITY;
  mx = -INFINITY;
  for (int k = threadIdx.x; k < n; k += FSG_WAVE) {
    const double* row = rows + (size_t)k * ROW;
    if (row[0] > 0.0) { mn = fmin(mn, row[ROW - 2]); mx = fmax(mx, row[ROW - 1]); }
  }
#pragma unroll
  for (int o = FSG_WAVE / 2; o > 0; o >>= 1) {
    mn = fmin(mn, __shfl_xor(mn, o, FSG_WAVE));
    mx = fmax(mx, __shfl_xor(mx, o, FSG_WAVE));
  }
}
