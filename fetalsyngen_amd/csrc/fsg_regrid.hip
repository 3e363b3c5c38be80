// fsg_regrid.hip -- resampling of real volumes through a 3x4 voxel-to-voxel affine, and the foreground box.
//
// What the reference does with monai transforms on the host (scripts/resample.py; transforms/inference.yaml as used by
// data/datasets.py:106-186 FetalTestDataset: Spacing, Orientation, CropForeground, SpatialPad / CenterSpatialCrop and
// their inverses): every one of those steps is an affine map between voxel grids, so the chain is ONE pass over the
// output with the composed map M and an "inside" box of the source.  Contract (tests/util_regrid64.py restates it in float64):
//   p = M (i,j,k,1);  inside iff lo_a - 0.5 <= p_a <= hi_a + 0.5 on every axis, else the fill values;
//   inside: p clamped to [lo_a, hi_a] (border replication within the box);
//   image: trilinear, f = floor(p), upper neighbour clamped to hi_a, weights 1-w and w, blended z, then y, then x;
//   label: the voxel at rint(p) (ties to even), copied.
// Coordinates are float32 in the order (m0 i + m1 j) + m2 k + m3 with separate multiplies and adds (contraction is off),
// from the INDEX of every voxel, never accumulated along a run: exact whenever the products and partial sums are
// representable (permutations, flips, integer shifts, factors on a 2^-8 grid), within 2^-13 of the float64 value for
// extents <= 512 otherwise.  No coordinate volume exists anywhere.
//
// Work shape: the output is z-fastest; a lane owns four consecutive elements of the FLAT output (16-byte image store,
// packed label store), so a quad that straddles the end of a row carries on in the next one when the z extent is no
// multiple of four (template WRAP) and only the last n % 4 elements of the volume are stored one by one.  All gathers of a lane's
// four voxels are issued before the first blend.  A gather kernel: bounded by the L1 / texture-address path as the warp.
#include "fsg_common.h"

namespace {

struct RegridK {
  float m[12];
  float lo[3], hi[3];      // the box as floats
  float lof[3], hif[3];    // lo - 0.5, hi + 0.5
  int hi_i[3];
  int s12, s2;             // source strides of axis 0 and 1 (elements)
  int d1, d2;              // output extents of axis 1 and 2
  float fill;
  int nan_zero;
};

template <typename LT> struct LabelPack;
template <> struct LabelPack<uint8_t> {
  typedef uint32_t type;
  static __device__ __forceinline__ type make(const uint8_t* l) {
    return (uint32_t)l[0] | ((uint32_t)l[1] << 8) | ((uint32_t)l[2] << 16) | ((uint32_t)l[3] << 24);
  }
};
template <> struct LabelPack<int16_t> {
  typedef uint2 type;
  static __device__ __forceinline__ type make(const int16_t* l) {
    return make_uint2((uint32_t)(uint16_t)l[0] | ((uint32_t)(uint16_t)l[1] << 16),
                      (uint32_t)(uint16_t)l[2] | ((uint32_t)(uint16_t)l[3] << 16));
  }
};
template <> struct LabelPack<float> {
  typedef float4 type;
  static __device__ __forceinline__ type make(const float* l) { return make_float4(l[0], l[1], l[2], l[3]); }
};

__device__ __forceinline__ float regrid_scrub(float v, int nan_zero) { return (nan_zero && v != v) ? 0.f : v; }

template <typename LT, bool HAS_IMG, bool HAS_LAB, bool WRAP>
__global__ __launch_bounds__(256) void regrid_kernel(RegridK P, const float* __restrict__ src, const LT* __restrict__ lab,
                                                     float* __restrict__ out, LT* __restrict__ out_lab, LT fill_lab,
                                                     unsigned n, int vec_img, int vec_lab) {
  const unsigned e = ((unsigned)xcd_tile((int)blockIdx.x, (int)gridDim.x) * 256u + threadIdx.x) << 2;
  if (e >= n) return;
  const unsigned row = e / (unsigned)P.d2;
  int k = (int)(e - row * (unsigned)P.d2);
  int i = (int)(row / (unsigned)P.d1);
  int j = (int)(row - (unsigned)i * (unsigned)P.d1);

  float p[4][3];
  bool in[4];
  bool any = false;
  float b[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) b[a] = P.m[4 * a] * (float)i + P.m[4 * a + 1] * (float)j;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (WRAP && q) {  // the quad may run over the end of a row (and of a plane): the voxel's own indices, every time
      if (++k == P.d2) {
        k = 0;
        if (++j == P.d1) { j = 0; ++i; }
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) b[a] = P.m[4 * a] * (float)i + P.m[4 * a + 1] * (float)j;
    }
    const float fk = (float)(WRAP ? k : k + q);
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float t = b[a] + P.m[4 * a + 2] * fk + P.m[4 * a + 3];
      ok = ok && (t >= P.lof[a]) && (t <= P.hif[a]);  // NaN / inf: outside
      p[q][a] = fminf(fmaxf(t, P.lo[a]), P.hi[a]);    // in the box whatever t is: every index below is in range
    }
    in[q] = ok;
    any = any || ok;
  }

  float v[4];
  LT l[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) { v[q] = P.fill; l[q] = fill_lab; }
  if (any) {
    float g[4][8];
    float w[4][3];
    LT t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (HAS_IMG) {
        int o0[3], o1[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const float f = floorf(p[q][a]);
          const int i0 = (int)f;
          const int i1 = min(i0 + 1, P.hi_i[a]);
          const int st = a == 0 ? P.s12 : a == 1 ? P.s2 : 1;
          w[q][a] = p[q][a] - f;
          o0[a] = i0 * st;
          o1[a] = i1 * st;
        }
        g[q][0] = src[(unsigned)(o0[0] + o0[1] + o0[2])];
        g[q][1] = src[(unsigned)(o0[0] + o0[1] + o1[2])];
        g[q][2] = src[(unsigned)(o0[0] + o1[1] + o0[2])];
        g[q][3] = src[(unsigned)(o0[0] + o1[1] + o1[2])];
        g[q][4] = src[(unsigned)(o1[0] + o0[1] + o0[2])];
        g[q][5] = src[(unsigned)(o1[0] + o0[1] + o1[2])];
        g[q][6] = src[(unsigned)(o1[0] + o1[1] + o0[2])];
        g[q][7] = src[(unsigned)(o1[0] + o1[1] + o1[2])];
      }
      if (HAS_LAB) {
        const int r0 = (int)rintf(p[q][0]), r1 = (int)rintf(p[q][1]), r2 = (int)rintf(p[q][2]);
        t[q] = lab[(unsigned)(r0 * P.s12 + r1 * P.s2 + r2)];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (HAS_IMG) {
#pragma unroll
        for (int c = 0; c < 8; ++c) g[q][c] = regrid_scrub(g[q][c], P.nan_zero);
        const float wx = w[q][0], wy = w[q][1], wz = w[q][2];
        const float ux = 1.f - wx, uy = 1.f - wy, uz = 1.f - wz;
        const float z00 = uz * g[q][0] + wz * g[q][1];
        const float z01 = uz * g[q][2] + wz * g[q][3];
        const float z10 = uz * g[q][4] + wz * g[q][5];
        const float z11 = uz * g[q][6] + wz * g[q][7];
        const float y0 = uy * z00 + wy * z01;
        const float y1 = uy * z10 + wy * z11;
        const float r = ux * y0 + wx * y1;
        if (in[q]) v[q] = r;
      }
      if (HAS_LAB) {
        if (in[q]) l[q] = t[q];
      }
    }
  }

  const bool full = e + 3 < n;
  if (HAS_IMG) {
    if (full && vec_img) {
      *reinterpret_cast<float4*>(out + e) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e + q < n) out[e + q] = v[q];
    }
  }
  if (HAS_LAB) {
    if (full && vec_lab) {
      *reinterpret_cast<typename LabelPack<LT>::type*>(out_lab + e) = LabelPack<LT>::make(l);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (e + q < n) out_lab[e + q] = l[q];
    }
  }
}

template <typename LT, bool HAS_IMG, bool HAS_LAB>
void regrid_launch(const RegridK& P, const float* src, const void* lab, float* out, void* out_lab, float fill_lab, unsigned n,
                   hipStream_t s) {
  const unsigned blocks = ((n + 3) / 4 + 255) / 256;
  const int vec_img = (((uintptr_t)out) & 15) == 0;
  const int vec_lab = (((uintptr_t)out_lab) & (4 * sizeof(LT) - 1)) == 0;
  const LT fl = (LT)fill_lab;
  if (P.d2 % 4 == 0)
    hipLaunchKernelGGL((regrid_kernel<LT, HAS_IMG, HAS_LAB, false>), dim3(blocks), dim3(256), 0, s, P, src, (const LT*)lab, out,
                       (LT*)out_lab, fl, n, vec_img, vec_lab);
  else
    hipLaunchKernelGGL((regrid_kernel<LT, HAS_IMG, HAS_LAB, true>), dim3(blocks), dim3(256), 0, s, P, src, (const LT*)lab, out,
                       (LT*)out_lab, fl, n, vec_img, vec_lab);
}

template <typename LT>
void regrid_dispatch(const RegridK& P, const float* src, const void* lab, float* out, void* out_lab, float fill_lab, unsigned n,
                     hipStream_t s) {
  if (src && lab) regrid_launch<LT, true, true>(P, src, lab, out, out_lab, fill_lab, n, s);
  else if (lab) regrid_launch<LT, false, true>(P, src, lab, out, out_lab, fill_lab, n, s);
  else regrid_launch<LT, true, false>(P, src, lab, out, out_lab, fill_lab, n, s);
}

// ---- foreground box ---------------------------------------------------------------------------------------------------
__global__ void bbox_init_kernel(int32_t* __restrict__ box, int n0, int n1, int n2) {
  if (threadIdx.x < 6) {
    const int a = threadIdx.x >> 1;
    box[threadIdx.x] = (threadIdx.x & 1) ? -1 : (a == 0 ? n0 : a == 1 ? n1 : n2);
  }
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, FSG_WAVE));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, FSG_WAVE));
  return v;
}

// a workgroup walks rows (i,j) of the volume, its lanes run along z; per-workgroup box, then at most six integer atomics
__global__ __launch_bounds__(256) void bbox_kernel(const float* __restrict__ v, int n0, int n1, int n2, float thr,
                                                   int32_t* __restrict__ box) {
  int lo0 = n0, lo1 = n1, lo2 = n2, hi0 = -1, hi1 = -1, hi2 = -1;
  const unsigned rows = (unsigned)n0 * (unsigned)n1;
  for (unsigned r = blockIdx.x; r < rows; r += gridDim.x) {
    const int i = (int)(r / (unsigned)n1), j = (int)(r - (unsigned)i * (unsigned)n1);
    const float* p = v + (size_t)r * n2;
    for (int k = threadIdx.x; k < n2; k += blockDim.x) {
      if (p[k] > thr) {  // NaN compares false
        lo0 = min(lo0, i); hi0 = max(hi0, i);
        lo1 = min(lo1, j); hi1 = max(hi1, j);
        lo2 = min(lo2, k); hi2 = max(hi2, k);
      }
    }
  }
  __shared__ int red[6][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  lo0 = wave_min_i(lo0); lo1 = wave_min_i(lo1); lo2 = wave_min_i(lo2);
  hi0 = wave_max_i(hi0); hi1 = wave_max_i(hi1); hi2 = wave_max_i(hi2);
  if (lane == 0) {
    red[0][wave] = lo0; red[1][wave] = hi0; red[2][wave] = lo1; red[3][wave] = hi1; red[4][wave] = lo2; red[5][wave] = hi2;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int c = threadIdx.x;
    int r = red[c][0];
    for (int w = 1; w < 4; ++w) r = (c & 1) ? max(r, red[c][w]) : min(r, red[c][w]);
    if (c & 1) {
      if (r >= 0) atomicMax(&box[c], r);
    } else {
      if (r < (c == 0 ? n0 : c == 2 ? n1 : n2)) atomicMin(&box[c], r);
    }
  }
}

}  // namespace

extern "C" {

int fsg_affine_resample(const float* src, const void* src_label, int label_dtype, int s0, int s1, int s2, const float* M_host,
                        const int32_t* box_host, int d0, int d1, int d2, float* out, void* out_label, float fill,
                        float fill_label, int nan_is_zero, void* stream) {
  if (!src && !src_label) return FSG_E_BADARG;
  if ((src != nullptr) != (out != nullptr) || (src_label != nullptr) != (out_label != nullptr)) return FSG_E_BADARG;
  if ((src && (const void*)src == (const void*)out) || (src_label && src_label == (const void*)out_label)) return FSG_E_BADARG;
  if (!M_host || !box_host) return FSG_E_BADARG;
  if (src_label && (label_dtype < FSG_LABEL_U8 || label_dtype > FSG_LABEL_F32)) return FSG_E_BADARG;
  if (s0 <= 0 || s1 <= 0 || s2 <= 0 || d0 <= 0 || d1 <= 0 || d2 <= 0) return FSG_E_BADARG;
  if (s0 > 1024 || s1 > 1024 || s2 > 1024 || d0 > 1024 || d1 > 1024 || d2 > 1024) return FSG_E_TOOBIG;
  const int sh[3] = {s0, s1, s2};
  RegridK P;
  for (int a = 0; a < 3; ++a) {
    const int lo = box_host[2 * a], hi = box_host[2 * a + 1];
    if (lo < 0 || hi >= sh[a] || lo > hi) return FSG_E_BADARG;  // an empty box, or one that leaves the volume
    P.lo[a] = (float)lo; P.hi[a] = (float)hi;
    P.lof[a] = (float)lo - 0.5f; P.hif[a] = (float)hi + 0.5f;
    P.hi_i[a] = hi;
  }
  for (int t = 0; t < 12; ++t) {
    if (!(M_host[t] - M_host[t] == 0.f)) return FSG_E_BADARG;  // NaN or infinite entry
    P.m[t] = M_host[t];
  }
  P.s12 = s1 * s2; P.s2 = s2; P.d1 = d1; P.d2 = d2;
  P.fill = fill; P.nan_zero = nan_is_zero ? 1 : 0;
  const unsigned n = (unsigned)d0 * (unsigned)d1 * (unsigned)d2;  // <= 2^30
  hipStream_t s = fsg_stream(stream);
  if (!src_label) regrid_dispatch<uint8_t>(P, src, nullptr, out, nullptr, 0.f, n, s);
  else if (label_dtype == FSG_LABEL_U8) regrid_dispatch<uint8_t>(P, src, src_label, out, out_label, fill_label, n, s);
  else if (label_dtype == FSG_LABEL_I16) regrid_dispatch<int16_t>(P, src, src_label, out, out_label, fill_label, n, s);
  else regrid_dispatch<float>(P, src, src_label, out, out_label, fill_label, n, s);
  FSG_RETURN_LAUNCH();
}

int fsg_bbox_gt_f32(const float* v, int n0, int n1, int n2, float thr, int32_t* box6_dev, void* stream) {
  if (!v || !box6_dev || n0 <= 0 || n1 <= 0 || n2 <= 0) return FSG_E_BADARG;
  if ((size_t)n0 * n1 * n2 > (size_t)0x7FFFFFFF) return FSG_E_TOOBIG;
  hipStream_t s = fsg_stream(stream);
  hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, s, box6_dev, n0, n1, n2);
  unsigned blocks = (unsigned)n0 * (unsigned)n1;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(bbox_kernel, dim3(blocks), dim3(256), 0, s, v, n0, n1, n2, thr, box6_dev);
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
