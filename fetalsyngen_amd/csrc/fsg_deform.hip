// fsg_deform.hip -- K2/K3/K4(/K5): deformation coordinates and the fused warp.
//
// Replaces, for one volume: `SpatialDeformation.generate_deformation_and_flip` +
// `apply_deformation_and_flip` (generator/deformation/affine_nonrigid.py:122-193, :299-366) and the
// `fast_3D_interp_torch` gathers (utils/generation.py:204-288) of the reference, plus optionally the
// RandGamma / RandBiasField pointwise stages (generator/augmentation/synthseg.py:274, :178-182).
//
// HBM layout: source and destination volumes (n0,n1,n2) fp32 (labels optionally uint8), z fastest.
// The 192 MiB coordinate volumes and the 192 MiB up-sampled field of the reference are never
// materialised: each thread re-evaluates the coarse field (<= 40 KB, L1/L2 resident) at its voxel.
#include "fsg_common.h"
#include "fsg_ride.h"

int g_tuning_flags = 0;  // FSG_TUNE_* bits, see fsg_set_tuning

namespace {

// ---- min/max of the clamped coordinates (affine_nonrigid.py:350-355) -------------------------
__global__ __launch_bounds__(256) void coords_minmax_kernel(FsgDeformK D, int32_t* __restrict__ mm6) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int rows = D.n0 * D.n1;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const int i = r / D.n1, j = r - i * D.n1;
    for (int k = threadIdx.x; k < D.n2; k += blockDim.x) {
      float x, y, z;
      fsg_position(D, i, j, k, x, y, z);
      lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
      lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
      lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
    }
  }
  __shared__ float red[6][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float l = fsg_wave_min(lo[a]), h = fsg_wave_max(hi[a]);
    if (lane == 0) { red[a][wave] = l; red[3 + a][wave] = h; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float v = red[a][0];
    for (int w = 1; w < 4; ++w) v = a < 3 ? fminf(v, red[a][w]) : fmaxf(v, red[a][w]);
    // -0.0 must order below +0.0 like torch.min would see it only by sign; keys keep the sign bit
    if (a < 3) fsg_atomic_min_key(&mm6[a], v);
    else fsg_atomic_max_key(&mm6[a], v);
  }
}

// ---- materialised coordinates (public API of SpatialDeformation) ------------------------------
__global__ __launch_bounds__(256) void coords_kernel(FsgDeformK D, const int32_t* __restrict__ mm6,
                                                     float* __restrict__ xx, float* __restrict__ yy,
                                                     float* __restrict__ zz) {
  const int k = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, i = blockIdx.z;
  if (k >= D.n2 || j >= D.n1) return;
  const Margins m = load_margins(mm6);
  float x, y, z;
  fsg_position(D, i, j, k, x, y, z);
  const size_t o = ((size_t)i * D.n1 + j) * D.n2 + k;
  xx[o] = x - m.mx;
  yy[o] = y - m.my;
  zz[o] = z - m.mz;
}

// ---- samplers ---------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T fetch(const T* __restrict__ s, const FsgDeformK& D, int x, int y, int z) {
  const int xs = D.flip ? (D.n0 - 1 - x) : x;  // torch.flip(.., [0]) folded into the index
  return s[((size_t)xs * D.n1 + y) * D.n2 + z];
}

__device__ __forceinline__ float sample_linear(const float* __restrict__ s, const FsgDeformK& D, float x,
                                               float y, float z) {
  const float hx = (float)(D.n0 - 1), hy = (float)(D.n1 - 1), hz = (float)(D.n2 - 1);
  const bool ok = (x > 0.f) && (y > 0.f) && (z > 0.f) && (x <= hx) && (y <= hy) && (z <= hz);
  if (!ok) return 0.f;
  const float fx = floorf(x), fy = floorf(y), fz = floorf(z);
  const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
  const int x1 = min(x0 + 1, D.n0 - 1), y1 = min(y0 + 1, D.n1 - 1), z1 = min(z0 + 1, D.n2 - 1);
  const float bx = x - fx, by = y - fy, bz = z - fz;
  const float ax = 1.f - bx, ay = 1.f - by, az = 1.f - bz;
  const float c000 = fetch(s, D, x0, y0, z0), c100 = fetch(s, D, x1, y0, z0);
  const float c010 = fetch(s, D, x0, y1, z0), c110 = fetch(s, D, x1, y1, z0);
  const float c001 = fetch(s, D, x0, y0, z1), c101 = fetch(s, D, x1, y0, z1);
  const float c011 = fetch(s, D, x0, y1, z1), c111 = fetch(s, D, x1, y1, z1);
  const float c00 = c000 * ax + c100 * bx;
  const float c01 = c001 * ax + c101 * bx;
  const float c10 = c010 * ax + c110 * bx;
  const float c11 = c011 * ax + c111 * bx;
  const float c0 = c00 * ay + c10 * by;
  const float c1 = c01 * ay + c11 * by;
  return c0 * az + c1 * bz;
}

template <typename T>
__device__ __forceinline__ T sample_nearest(const T* __restrict__ s, const FsgDeformK& D, float x, float y,
                                            float z) {
  int xi = (int)rintf(x), yi = (int)rintf(y), zi = (int)rintf(z);  // round half to even
  xi = min(max(xi, 0), D.n0 - 1);
  yi = min(max(yi, 0), D.n1 - 1);
  zi = min(max(zi, 0), D.n2 - 1);
  return fetch(s, D, xi, yi, zi);
}

// =================================================================================================
// Row-wise kernels (the tuned path).  One wave owns one output row (i, j, all k) at a time:
//   1. the 64 lanes evaluate the x- and y-interpolation of the coarse displacement grid (and of the
//      coarse bias grid) ONCE per row -- 3*f2 + b2 values -- into a wave-private LDS slot;
//   2. every voxel of the row then needs only the z-interpolation: two LDS reads + one lerp per
//      channel, instead of 8 global loads + 7 lerps per channel.
// The arithmetic per voxel is the same sequence of fp32 operations as fsg_tab_interp (x, then y, then
// z; products then sum, no FMA), so positions are bit-identical to the per-voxel kernels.
// =================================================================================================
constexpr int ROWCAP = 512;  // floats of LDS per wave (3*f2 + b2 must fit; else per-voxel fallback)

// x/y part of the separable interpolation for one row: dst[c*s2 + zs], c < NCH
template <int NCH>
__device__ __forceinline__ void fill_row_xy(const float* __restrict__ grid, int s1, int s2, const fsg_tap a,
                                            const fsg_tap b, float* dst, int lane) {
  const float* p00 = grid + (((size_t)a.lo * s1 + b.lo) * s2) * NCH;
  const float* p10 = grid + (((size_t)a.hi * s1 + b.lo) * s2) * NCH;
  const float* p01 = grid + (((size_t)a.lo * s1 + b.hi) * s2) * NCH;
  const float* p11 = grid + (((size_t)a.hi * s1 + b.hi) * s2) * NCH;
  for (int e = lane; e < NCH * s2; e += FSG_WAVE) {
    const int c = e / s2, zs = e - c * s2;
    const int o = zs * NCH + c;
    const float t0 = fsg_mix(a.w_lo, p00[o], a.w_hi, p10[o]);  // y = b.lo
    const float t1 = fsg_mix(a.w_lo, p01[o], a.w_hi, p11[o]);  // y = b.hi
    dst[e] = fsg_mix(b.w_lo, t0, b.w_hi, t1);
  }
}

// position of voxel (i,j,k) from the row's LDS slot (same op order as fsg_position)
__device__ __forceinline__ void row_position(const FsgDeformK& D, const float* sm, int i, int j, int k,
                                             const fsg_tap& c, float& x, float& y, float& z) {
  float px = (float)i - D.cen[0], py = (float)j - D.cen[1], pz = (float)k - D.cen[2];
  if (D.field) {
    px = px + fsg_mix(c.w_lo, sm[c.lo], c.w_hi, sm[c.hi]);
    py = py + fsg_mix(c.w_lo, sm[D.f2 + c.lo], c.w_hi, sm[D.f2 + c.hi]);
    pz = pz + fsg_mix(c.w_lo, sm[2 * D.f2 + c.lo], c.w_hi, sm[2 * D.f2 + c.hi]);
  }
  x = D.A[0] * px + D.A[1] * py + D.A[2] * pz + D.c2[0];
  y = D.A[3] * px + D.A[4] * py + D.A[5] * pz + D.c2[1];
  z = D.A[6] * px + D.A[7] * py + D.A[8] * pz + D.c2[2];
  const float hx = (float)(D.n0 - 1), hy = (float)(D.n1 - 1), hz = (float)(D.n2 - 1);
  if (x < 0.f) x = 0.f;
  if (y < 0.f) y = 0.f;
  if (z < 0.f) z = 0.f;
  if (x > hx) x = hx;
  if (y > hy) y = hy;
  if (z > hz) z = hz;
}

typedef float float2_u __attribute__((ext_vector_type(2), aligned(4)));

// ---- per-row coarse values, precomputed once per deformation ------------------------------------------
// rows[(i*n1 + j)*stride + e]: e < 3*f2 -> x/y-interpolated displacement (channel-major, then z index of
// the coarse grid); 3*f2 <= e < 3*f2 + b2 -> x/y-interpolated bias grid.  One thread per entry.  With this
// buffer the warp / min-max kernels start a row with ONE coalesced load instead of a dependent chain
// (table entry -> four coarse-grid loads -> LDS).
__device__ __forceinline__ void deform_rows_body(const FsgDeformK& D, const EpiK& E, float* __restrict__ rows, int stride,
                                                 int i, int t) {  // t = (j, e) of x plane i
  const int nf = D.field ? 3 * D.f2 : 0;
  const int need = nf + (E.bias ? E.b2 : 0);
  if (t >= D.n1 * need) return;
  const int j = t / need, e = t - j * need;
  float v;
  if (e < nf) {
    const fsg_tap a = D.tx[i], b = D.ty[j];
    const int c = e / D.f2, zs = e - c * D.f2;
    const int o = zs * 3 + c;
    const float* g = D.field;
    const float f00 = g[((a.lo * D.f1 + b.lo) * D.f2) * 3 + o];
    const float f10 = g[((a.hi * D.f1 + b.lo) * D.f2) * 3 + o];
    const float f01 = g[((a.lo * D.f1 + b.hi) * D.f2) * 3 + o];
    const float f11 = g[((a.hi * D.f1 + b.hi) * D.f2) * 3 + o];
    v = fsg_mix(b.w_lo, fsg_mix(a.w_lo, f00, a.w_hi, f10), b.w_hi, fsg_mix(a.w_lo, f01, a.w_hi, f11));
  } else {
    const fsg_tap a = E.bx[i], b = E.by[j];
    const int zs = e - nf;
    const float* g = E.bias;
    const float f00 = g[(a.lo * E.b1 + b.lo) * E.b2 + zs];
    const float f10 = g[(a.hi * E.b1 + b.lo) * E.b2 + zs];
    const float f01 = g[(a.lo * E.b1 + b.hi) * E.b2 + zs];
    const float f11 = g[(a.hi * E.b1 + b.hi) * E.b2 + zs];
    v = fsg_mix(b.w_lo, fsg_mix(a.w_lo, f00, a.w_hi, f10), b.w_hi, fsg_mix(a.w_lo, f01, a.w_hi, f11));
  }
  rows[((size_t)i * D.n1 + j) * stride + e] = v;
}

// Workgroup form of the same values.  The per-entry kernel is bound by dependent round trips, not by bytes: 11 000 workgroups
// each live for a tap load -> four gathers -> one store, and only 2 048 of them are resident at a time.  Here a workgroup
// owns one x plane and RB_J consecutive y rows: ONE phase of global loads (the x taps, the two coarse planes they select,
// the y taps of its rows), then every entry is a y-blend of two LDS values.  Blend order x then y as above: bit-identical.
constexpr int RB_J = 64;        // y rows per workgroup
constexpr int RB_SLAB_F = 2048; // floats: f1 * f2 * 3 of the coarse displacement grid
constexpr int RB_SLAB_B = 256;  // floats: b1 * b2 of the coarse bias grid
constexpr int RB_NEED = 512;    // entries per row

struct RowsSmem {
  float sf[RB_SLAB_F];
  float sb[RB_SLAB_B];
  int tab[RB_NEED];
  int4 ty[RB_J];
  int4 by[RB_J];
};

__host__ __device__ inline bool rows_block_fits(const FsgDeformK& D, const EpiK& E) {
  const int nf = D.field ? 3 * D.f2 : 0, nb = E.bias ? E.b2 : 0;
  return (D.field ? D.f1 * D.f2 * 3 : 0) <= RB_SLAB_F && (E.bias ? E.b1 * E.b2 : 0) <= RB_SLAB_B && nf + nb <= RB_NEED;
}

__device__ __forceinline__ void deform_rows_block(const FsgDeformK& D, const EpiK& E, float* __restrict__ rows, int stride,
                                                  int i, int j0, RowsSmem& S) {
  const int tid = threadIdx.x;
  const int nf = D.field ? 3 * D.f2 : 0, nb = E.bias ? E.b2 : 0, need = nf + nb;
  const int slab_f = D.field ? D.f1 * D.f2 * 3 : 0, slab_b = E.bias ? E.b1 * E.b2 : 0;
  const int jn = min(RB_J, D.n1 - j0);
  if (tid < jn) {
    if (D.field) S.ty[tid] = *reinterpret_cast<const int4*>(D.ty + j0 + tid);
    if (E.bias) S.by[tid] = *reinterpret_cast<const int4*>(E.by + j0 + tid);
  }
  if (D.field) {
    const fsg_tap a = fsg_uniform_tap(D.tx, i);
    const float* g0 = D.field + (size_t)a.lo * slab_f;
    const float* g1 = D.field + (size_t)a.hi * slab_f;
    for (int t = tid; t < slab_f; t += 256) S.sf[t] = fsg_mix(a.w_lo, g0[t], a.w_hi, g1[t]);
  }
  if (E.bias) {
    const fsg_tap a = fsg_uniform_tap(E.bx, i);
    const float* g0 = E.bias + (size_t)a.lo * slab_b;
    const float* g1 = E.bias + (size_t)a.hi * slab_b;
    for (int t = tid; t < slab_b; t += 256) S.sb[t] = fsg_mix(a.w_lo, g0[t], a.w_hi, g1[t]);
  }
  for (int e = tid; e < need; e += 256) {
    if (e < nf) {
      const int c = e / D.f2, zs = e - c * D.f2;
      S.tab[e] = zs * 3 + c;
    } else {
      S.tab[e] = e - nf;
    }
  }
  __syncthreads();
  const int rf = D.f2 * 3;
  for (int jj = tid >> 6; jj < jn; jj += 4) {
    float* dst = rows + ((size_t)i * D.n1 + j0 + jj) * stride;
    for (int e = tid & 63; e < need; e += 64) {
      const int o = S.tab[e];
      float v;
      if (e < nf) {
        const int4 b = S.ty[jj];
        v = fsg_mix(__builtin_bit_cast(float, b.z), S.sf[b.x * rf + o], __builtin_bit_cast(float, b.w), S.sf[b.y * rf + o]);
      } else {
        const int4 b = S.by[jj];
        v = fsg_mix(__builtin_bit_cast(float, b.z), S.sb[b.x * E.b2 + o], __builtin_bit_cast(float, b.w),
                    S.sb[b.y * E.b2 + o]);
      }
      dst[e] = v;
    }
  }
}

__global__ __launch_bounds__(256) void deform_rows_block_kernel(FsgDeformK D, EpiK E, float* __restrict__ rows, int stride) {
  __shared__ RowsSmem S;
  deform_rows_block(D, E, rows, stride, blockIdx.y, blockIdx.x * RB_J, S);
}

__global__ __launch_bounds__(256) void deform_rows_kernel(FsgDeformK D, EpiK E, float* __restrict__ rows, int stride) {
  deform_rows_body(D, E, rows, stride, blockIdx.y, blockIdx.x * blockDim.x + threadIdx.x);
}

// ---- floor(min) of the clamped coordinates with a boundary shortcut --------------------------------------
// Only floor(min) per axis is consumed downstream (margin subtraction, affine_nonrigid.py:350-358).  The
// coordinates are clamped to [0, n-1], so as soon as ONE voxel has a coordinate < 1 on an axis, that axis'
// floor(min) is 0 whatever the other voxels do.  In practice such voxels sit on the faces of the grid: pass 1
// evaluates the six faces only (2.3 % of a 256^3 grid); pass 2 (all voxels) runs only for the rare
// deformations where some axis is still unresolved -- every block of it first checks the three keys and
// exits when all are below key(1.0).  The result has the same floor as the exact minimum.
constexpr int FACE_STEP = 4;
__host__ __device__ inline int faces_samples(int n) { return (n - 1 + FACE_STEP - 1) / FACE_STEP + 1; }  // 0, 4, .., n-1
__host__ __device__ inline int faces_total(int n0, int n1, int n2) {
  const int m0 = faces_samples(n0), m1 = faces_samples(n1), m2 = faces_samples(n2);
  return 2 * (m1 * m2 + m0 * m2 + m0 * m1);
}

__device__ __forceinline__ void coords_faces_min_body(const FsgDeformK& D, int32_t* __restrict__ mm3, float (*red)[4],
                                                      int blk, int nblk) {
  // every FACE_STEP-th voxel of each face in both directions, the last index always included (corners and edges are in):
  // ANY subset of voxels is a valid first pass -- a coordinate < 1 found settles its axis, an axis left open sends the
  // sample through the exact full pass
  const int n0 = D.n0, n1 = D.n1, n2 = D.n2;
  const int m0 = faces_samples(n0), m1 = faces_samples(n1), m2 = faces_samples(n2);
  const int fa = m1 * m2, fb = m0 * m2, fc = m0 * m1;
  const int total = 2 * (fa + fb + fc);
  float lo[3] = {INFINITY, INFINITY, INFINITY};
  for (int t = blk * blockDim.x + threadIdx.x; t < total; t += nblk * blockDim.x) {
    int i, j, k, u = t;
    if (u < 2 * fa) {
      i = (u >= fa) ? n0 - 1 : 0; u %= fa; j = u / m2; k = u - j * m2;
      j = min(j * FACE_STEP, n1 - 1); k = min(k * FACE_STEP, n2 - 1);
    } else if ((u -= 2 * fa) < 2 * fb) {
      j = (u >= fb) ? n1 - 1 : 0; u %= fb; i = u / m2; k = u - i * m2;
      i = min(i * FACE_STEP, n0 - 1); k = min(k * FACE_STEP, n2 - 1);
    } else {
      u -= 2 * fb; k = (u >= fc) ? n2 - 1 : 0; u %= fc; i = u / m1; j = u - i * m1;
      i = min(i * FACE_STEP, n0 - 1); j = min(j * FACE_STEP, n1 - 1);
    }
    float x, y, z;
    fsg_position(D, i, j, k, x, y, z);
    lo[0] = fminf(lo[0], x);
    lo[1] = fminf(lo[1], y);
    lo[2] = fminf(lo[2], z);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float l = fsg_wave_min(lo[a]);
    if (lane == 0) red[a][wave] = l;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    float v = red[a][0];
    for (int w = 1; w < 4; ++w) v = fminf(v, red[a][w]);
    fsg_atomic_min_key(&mm3[a], v);
  }
}

__global__ __launch_bounds__(256) void coords_faces_min_kernel(FsgDeformK D, int32_t* __restrict__ mm3) {
  __shared__ float red[3][4];
  coords_faces_min_body(D, mm3, red, blockIdx.x, gridDim.x);
}

// ---- head of a sample as ONE launch ----------------------------------------------------------------------------
// The GMM draw (K1), the per-row coarse values and the six-face minimum do not depend on one another, and the two small ones
// cost a launch each mostly for the launch itself (~6 us of dispatch + end-of-kernel write-back against 2-4 us of work).
// Workgroups [0, nfaces) reduce the faces, [nfaces, nfaces + nrows) fill the rows, the rest draw the intensities (VALU-bound,
// so the small latency-bound work hides beside it).  The min/max keys must already be initialised (they arrive with the
// parameter arena): no workgroup of this launch may reset what another one reduces into.
struct HeadGmm {
  const uint8_t* l0; const uint8_t* l1; const uint8_t* l2; const uint8_t* l3;
  size_t n;
  const float* mus; const float* sigmas; int ntab;
  const float* noise; uint64_t seed, stream_id;
  float* out;
  // codes mode (ntuples > 0): l0 = the uint16 code volume, l1 = the tuples, sel = the four selected bytes of a row (8 bits each)
  int ntuples, stride;
  uint32_t sel;
};

// 8 waves/SIMD (<= 64 VGPRs) as the stand-alone GMM kernel has: the face job alone would take 73 and cap the launch at 6
// HAS_DRAW: the NEXT sample's keyed draw job (fsg_ride.h; fsg_sample_plan::ride_draw) in workgroups [nfaces, nfaces + ndraw).
// It touches nothing of this sample, borrows the GMM job's s_mu table (a workgroup does one job) and, like the faces, is a
// dependent chain that should start before the bandwidth-bound jobs fill the machine.  ndraw == 0: no job, P is not read.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void sample_head_kernel(HeadGmm G, FsgDeformK D, EpiK E, float* __restrict__ rows,
                                                          int stride, int rows_gx, int nrows, int nfaces,
                                                          int32_t* __restrict__ mm3, int ndraw, const fsg_ride::DrawK P) {
  __shared__ float s_mu[256], s_sg[256];
  __shared__ float red[3][4];
  union HeadSmem {  // a workgroup does one job: the rows job's block and the codes mode's (mu, sigma) table share the space
    RowsSmem rows;
    float2 code_ms[FSG_CODES_MAX];
  };
  __shared__ HeadSmem U;
  RowsSmem& S = U.rows;
  int b = blockIdx.x;  // workgroup-uniform branches: a workgroup does exactly one of the jobs
  if (b < nfaces) {  // the longest dependent chain first
    coords_faces_min_body(D, mm3, red, b, nfaces);
    return;
  }
  b -= nfaces;
  if (b < ndraw) {
    fsg_ride::keyed_draw_body(P, b, s_mu);
    return;
  }
  b -= ndraw;
  if (b < nrows) {
    deform_rows_block(D, E, rows, stride, b / rows_gx, (b % rows_gx) * RB_J, S);
    return;
  }
  b -= nrows;
  if (G.ntuples > 0) {  // codes mode (fsg_ride.h)
    const fsg_ride::GmmCodesK C{G.l0, G.l1, G.ntuples, G.stride, G.sel, G.n, G.mus, G.sigmas, G.ntab, G.seed, G.stream_id, G.out};
    fsg_ride::gmm_codes_job(C, U.code_ms, (unsigned)b, gridDim.x - (unsigned)(nrows + nfaces + ndraw));
    return;
  }
  for (int t = threadIdx.x; t < 256; t += blockDim.x) {
    s_mu[t] = t < G.ntab ? G.mus[t] : 0.f;
    s_sg[t] = t < G.ntab ? G.sigmas[t] : 0.f;
  }
  __syncthreads();
  fsg_gmm_x4_loop(G.l0, G.l1, G.l2, G.l3, G.n, s_mu, s_sg, G.noise, G.seed, G.stream_id, G.out, (unsigned)b,
                  gridDim.x - (unsigned)(nrows + nfaces + ndraw));
}

constexpr int WARP_ROWS_PER_WAVE = 4;

// Tuning knobs measured on MI355X (tools/kernel_bench.py, 256^3, rot 12 deg): batch 2 + skipping the gathers
// of voxels that sample outside the volume is the fastest of {1,2,4} x {skip, no skip} for the full kernel.
#ifndef FSG_WARP_BATCH
#define FSG_WARP_BATCH 2
#endif
#ifndef FSG_WARP_NO_SKIP_OUTSIDE
#define FSG_WARP_SKIP_OUTSIDE 1
#endif

template <typename LT, bool HAS_LIN, bool HAS_NN, bool FAST, int Q0, int NQ>
__device__ __forceinline__ void warp_emitN(const FsgDeformK& D, const EpiK& E, const Margins& m, const float* sm,
                                           int nf, int i, int j, int kbase, const fsg_tap (&ck)[4],
                                           const fsg_tap (&cbk)[4], size_t row, const float* __restrict__ src_lin,
                                           float* __restrict__ out_lin, const LT* __restrict__ src_nn,
                                           LT* __restrict__ out_nn) {
  const float hx = (float)(D.n0 - 1), hy = (float)(D.n1 - 1), hz = (float)(D.n2 - 1);
  const unsigned sx = (unsigned)D.n1 * (unsigned)D.n2, sy = (unsigned)D.n2;
  float x[NQ], y[NQ], z[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int k = min(kbase + 64 * (Q0 + q), D.n2 - 1);
    row_position(D, sm, i, j, k, ck[Q0 + q], x[q], y[q], z[q]);
    x[q] = x[q] - m.mx;
    y[q] = y[q] - m.my;
    z[q] = z[q] - m.mz;
  }
  LT nn[NQ];
  if (HAS_NN) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int xi = (int)rintf(x[q]), yi = (int)rintf(y[q]), zi = (int)rintf(z[q]);
      xi = min(max(xi, 0), D.n0 - 1);
      yi = min(max(yi, 0), D.n1 - 1);
      zi = min(max(zi, 0), D.n2 - 1);
      if (D.flip) xi = D.n0 - 1 - xi;
      nn[q] = src_nn[(unsigned)xi * sx + (unsigned)yi * sy + (unsigned)zi];
    }
  }
  float2_u p00[NQ], p10[NQ], p01[NQ], p11[NQ];
  float bx[NQ], by[NQ], bz[NQ];
  bool ok[NQ], hi0[NQ];
  if (HAS_LIN) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      ok[q] = (x[q] > 0.f) && (y[q] > 0.f) && (z[q] > 0.f) && (x[q] <= hx) && (y[q] <= hy) && (z[q] <= hz);
      const float fx = floorf(x[q]), fy = floorf(y[q]), fz = floorf(z[q]);
      bx[q] = x[q] - fx;
      by[q] = y[q] - fy;
      bz[q] = z[q] - fz;
      int x0 = min(max((int)fx, 0), D.n0 - 1), y0 = min(max((int)fy, 0), D.n1 - 1), z0 = min(max((int)fz, 0), D.n2 - 1);
      int x1 = min(x0 + 1, D.n0 - 1);
      const int y1 = min(y0 + 1, D.n1 - 1);
      if (D.flip) { x0 = D.n0 - 1 - x0; x1 = D.n0 - 1 - x1; }
      const int zb = min(z0, D.n2 - 2);
      hi0[q] = z0 != zb;
      const unsigned o00 = (unsigned)x0 * sx + (unsigned)y0 * sy + (unsigned)zb;
      const unsigned o10 = (unsigned)x1 * sx + (unsigned)y0 * sy + (unsigned)zb;
      const unsigned o01 = (unsigned)x0 * sx + (unsigned)y1 * sy + (unsigned)zb;
      const unsigned o11 = (unsigned)x1 * sx + (unsigned)y1 * sy + (unsigned)zb;
#ifdef FSG_WARP_SKIP_OUTSIDE
      p00[q] = p10[q] = p01[q] = p11[q] = float2_u{0.f, 0.f};
      if (ok[q])  // voxels that sample outside the volume (clamped onto a 0-face) need no data
#endif
      {
        p00[q] = *reinterpret_cast<const float2_u*>(src_lin + o00);
        p10[q] = *reinterpret_cast<const float2_u*>(src_lin + o10);
        p01[q] = *reinterpret_cast<const float2_u*>(src_lin + o01);
        p11[q] = *reinterpret_cast<const float2_u*>(src_lin + o11);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int k = kbase + 64 * (Q0 + q);
    const bool live = k < D.n2;
    if (HAS_NN && live) out_nn[row + k] = nn[q];
    if (HAS_LIN) {
      const float ax = 1.f - bx[q], ay = 1.f - by[q], az = 1.f - bz[q];
      const float c000 = hi0[q] ? p00[q].y : p00[q].x, c001 = p00[q].y;
      const float c100 = hi0[q] ? p10[q].y : p10[q].x, c101 = p10[q].y;
      const float c010 = hi0[q] ? p01[q].y : p01[q].x, c011 = p01[q].y;
      const float c110 = hi0[q] ? p11[q].y : p11[q].x, c111 = p11[q].y;
      const float c00 = c000 * ax + c100 * bx[q];
      const float c01 = c001 * ax + c101 * bx[q];
      const float c10 = c010 * ax + c110 * bx[q];
      const float c11 = c011 * ax + c111 * bx[q];
      const float c0 = c00 * ay + c10 * by[q];
      const float c1 = c01 * ay + c11 * by[q];
      float v = ok[q] ? (c0 * az + c1 * bz[q]) : 0.f;
      if (E.gamma > 0.f) {
        // 300*(v/300)^g.  FAST: 300 * 2^(g*(log2 v - log2 300)) on v_log_f32 / v_exp_f32; else OCML powf and
        // an IEEE division like ATen.  (|FAST - precise| < 1e-4 on the 0..255 scale, tests/test_hip_parity.py)
        if (FAST) v = 300.0f * __builtin_amdgcn_exp2f(E.gamma * (__builtin_amdgcn_logf(v) - 8.2288186904958804f));
        else v = 300.0f * powf(v / 300.0f, E.gamma);
      }
      if (E.bias) {
        const fsg_tap cb = cbk[Q0 + q];
        const float bval = fsg_mix(cb.w_lo, sm[nf + cb.lo], cb.w_hi, sm[nf + cb.hi]);
        v = v * (FAST ? __builtin_amdgcn_exp2f(bval * 1.4426950408889634f) : expf(bval));
      }
      if (live) out_lin[row + k] = v;
    }
  }
}

template <typename LT, bool HAS_LIN, bool HAS_NN, bool FAST>
__device__ __forceinline__ void warp_emit4(const FsgDeformK& D, const EpiK& E, const Margins& m, const float* sm,
                                           int nf, int i, int j, int kbase, const fsg_tap (&ck)[4],
                                           const fsg_tap (&cbk)[4], size_t row, const float* __restrict__ src_lin,
                                           float* __restrict__ out_lin, const LT* __restrict__ src_nn,
                                           LT* __restrict__ out_nn) {
#define FSG_EMIT(Q0, NQ) \
  warp_emitN<LT, HAS_LIN, HAS_NN, FAST, Q0, NQ>(D, E, m, sm, nf, i, j, kbase, ck, cbk, row, src_lin, out_lin, src_nn, out_nn)
#if FSG_WARP_BATCH == 4
  FSG_EMIT(0, 4);
#elif FSG_WARP_BATCH == 2
  FSG_EMIT(0, 2);
  FSG_EMIT(2, 2);
#else
  FSG_EMIT(0, 1);
  FSG_EMIT(1, 1);
  FSG_EMIT(2, 1);
  FSG_EMIT(3, 1);
#endif
#undef FSG_EMIT
}

// stage one row's coarse values into the wave's LDS slot
__device__ __forceinline__ void stage_row(const FsgDeformK& D, const EpiK& E, int i, int j, int nf, int need,
                                          const fsg_tap& ax, const fsg_tap& abx, float* sm, int lane) {
  if (D.rows) {
    const float* r = D.rows + ((size_t)i * D.n1 + j) * D.row_stride;
    for (int e = lane; e < need; e += FSG_WAVE) sm[e] = r[e];
  } else {
    if (D.field) fill_row_xy<3>(D.field, D.f1, D.f2, ax, fsg_uniform_tap(D.ty, j), sm, lane);
    if (E.bias) fill_row_xy<1>(E.bias, E.b1, E.b2, abx, fsg_uniform_tap(E.by, j), sm + nf, lane);
  }
}

template <typename LT, bool HAS_LIN, bool HAS_NN, bool FAST>
__global__ __launch_bounds__(256) void warp_rows_kernel(FsgDeformK D, const int32_t* __restrict__ mm6,
                                                        const float* __restrict__ src_lin,
                                                        float* __restrict__ out_lin, const LT* __restrict__ src_nn,
                                                        LT* __restrict__ out_nn, EpiK E) {
  __shared__ float sm_all[4][2][ROWCAP];  // per wave, double buffered
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // Row -> wave mapping (FSG_WARP_MAP).  An L1-missing cache line costs ~10.7 cycles of the CU's fill path
  // (profiles/r01_gather_cost_ubench.txt), so the four waves of a block should gather from ADJACENT source
  // rows at the same time: 0 = wave w owns rows 4w..4w+3 (no sharing), 1 = wave w owns rows w, w+4, w+8,
  // w+12 (the block sweeps 4 adjacent rows per step), 2 = 2x2 patches of (x,y) rows.
#ifndef FSG_WARP_MAP
#define FSG_WARP_MAP 1
#endif
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
#if FSG_WARP_MAP == 2
  const int tiles_j = (D.n1 + 2 * WARP_ROWS_PER_WAVE - 1) / (2 * WARP_ROWS_PER_WAVE);
  const int i = min(2 * (tile / tiles_j) + (wave >> 1), D.n0 - 1);
  const bool dead_i = 2 * (tile / tiles_j) + (wave >> 1) >= D.n0;
  const int jbase = (tile % tiles_j) * (2 * WARP_ROWS_PER_WAVE) + (wave & 1);
  const int jstep = 2;
#else
  const int tiles_j = (D.n1 + 4 * WARP_ROWS_PER_WAVE - 1) / (4 * WARP_ROWS_PER_WAVE);
  const int i = tile / tiles_j;
  const bool dead_i = false;
#if FSG_WARP_MAP == 1
  const int jbase = (tile - i * tiles_j) * (4 * WARP_ROWS_PER_WAVE) + wave;
  const int jstep = 4;
#else
  const int jbase = (tile - i * tiles_j) * (4 * WARP_ROWS_PER_WAVE) + wave * WARP_ROWS_PER_WAVE;
  const int jstep = 1;
#endif
#endif
  const Margins m = load_margins(mm6);
  const int nf = D.field ? 3 * D.f2 : 0;
  const int need = nf + (E.bias ? E.b2 : 0);
  const fsg_tap none = fsg_tap{0, 0, 0.f, 0.f};
  const bool onfly = D.rows == nullptr;
  const fsg_tap ax = (onfly && D.field) ? fsg_uniform_tap(D.tx, i) : none;
  const fsg_tap abx = (onfly && E.bias) ? fsg_uniform_tap(E.bx, i) : none;
  // the z tables are the same for every row: keep this lane's entries in registers (n2 <= 256)
  const bool cached = D.n2 <= 256;
  fsg_tap ck[4], cbk[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = min(lane + 64 * q, D.n2 - 1);
    ck[q] = D.field ? D.tz[k] : none;
    cbk[q] = E.bias ? E.bz[k] : none;
  }
  if (dead_i) return;
  if (jbase < D.n1 && need) stage_row(D, E, i, jbase, nf, need, ax, abx, sm_all[wave][0], lane);
  for (int r = 0; r < WARP_ROWS_PER_WAVE; ++r) {
    const int j = jbase + r * jstep;
    if (j >= D.n1) break;
    const float* sm = sm_all[wave][r & 1];
    fsg_wave_lds_sync();
    // prefetch the next row's coarse values into the other buffer while this row's gathers are in flight
    if (r + 1 < WARP_ROWS_PER_WAVE && j + jstep < D.n1 && need)
      stage_row(D, E, i, j + jstep, nf, need, ax, abx, sm_all[wave][(r + 1) & 1], lane);
    const size_t row = ((size_t)i * D.n1 + j) * D.n2;
    if (cached) {
      warp_emit4<LT, HAS_LIN, HAS_NN, FAST>(D, E, m, sm, nf, i, j, lane, ck, cbk, row, src_lin, out_lin, src_nn,
                                            out_nn);
    } else {
      for (int kb = 0; kb < D.n2; kb += 256) {
        fsg_tap c4[4], b4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = min(kb + lane + 64 * q, D.n2 - 1);
          c4[q] = D.field ? D.tz[k] : none;
          b4[q] = E.bias ? E.bz[k] : none;
        }
        warp_emit4<LT, HAS_LIN, HAS_NN, FAST>(D, E, m, sm, nf, i, j, kb + lane, c4, b4, row, src_lin, out_lin,
                                              src_nn, out_nn);
      }
    }
  }
}

// ---- patch variant: 16 waves sweep a 4 x 4 patch of adjacent rows in lockstep ----------------------------
// Cost model (profiles/r01_gather_cost_ubench.txt): a gather costs ~10.7 cycles of the CU's fill path per
// 128-B line that misses L1, whatever its width.  Output rows (i..i+3, j..j+3) read source rows that
// overlap almost entirely (their 2x2 neighbourhoods interleave), so when the 16 waves of ONE workgroup
// advance through z together -- one 64-voxel chunk per wave per step, a barrier per step -- a line missed
// by one wave is an L1 hit for the others.  Same per-voxel arithmetic as the row kernel (warp_emitN).
constexpr int PATCH = 4;
constexpr int PATCH_ROWCAP = 128;
#ifndef FSG_PATCH_NQ
#define FSG_PATCH_NQ 1
#endif
constexpr int PATCH_NQ = FSG_PATCH_NQ;  // 64-voxel chunks per lane and lockstep step (2: 174 us against 135 us -- the L1 working set doubles)
constexpr int PATCH_TZCAP = 512;  // z extent whose taps are staged in LDS (2 x 8 KB)

template <typename LT, bool HAS_LIN, bool HAS_NN, bool FAST>
__global__ __launch_bounds__(1024, 8) void warp_patch_kernel(FsgDeformK D, const int32_t* __restrict__ mm6,
                                                          const float* __restrict__ src_lin,
                                                          float* __restrict__ out_lin,
                                                          const LT* __restrict__ src_nn, LT* __restrict__ out_nn,
                                                          EpiK E) {
  __shared__ float sm_all[PATCH * PATCH][PATCH_ROWCAP];
  // the z taps of the whole row (displacement and bias grids), staged once per workgroup: read from the tables inside
  // the chunk loop they put a dependent global round trip in front of every chunk's gathers
  __shared__ int4 s_tz[PATCH_TZCAP], s_bz[PATCH_TZCAP];
  const bool taps_lds = D.n2 <= PATCH_TZCAP;
  if (taps_lds) {
    for (int t = threadIdx.x; t < D.n2; t += 1024) {
      if (D.field) s_tz[t] = *reinterpret_cast<const int4*>(D.tz + t);
      if (E.bias) s_bz[t] = *reinterpret_cast<const int4*>(E.bz + t);
    }
  }
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int tiles_j = (D.n1 + PATCH - 1) / PATCH;
  const int tile = xcd_tile(blockIdx.x, gridDim.x);
  const int i_raw = (tile / tiles_j) * PATCH + (wave >> 2), j_raw = (tile % tiles_j) * PATCH + (wave & 3);
  const bool live_row = i_raw < D.n0 && j_raw < D.n1;
  const int i = min(i_raw, D.n0 - 1), j = min(j_raw, D.n1 - 1);
  const Margins m = load_margins(mm6);
  const int nf = D.field ? 3 * D.f2 : 0;
  const int need = nf + (E.bias ? E.b2 : 0);
  const fsg_tap none = fsg_tap{0, 0, 0.f, 0.f};
  float* sm = sm_all[wave];
  if (need) {
    const bool onfly = D.rows == nullptr;
    const fsg_tap ax = (onfly && D.field) ? fsg_uniform_tap(D.tx, i) : none;
    const fsg_tap abx = (onfly && E.bias) ? fsg_uniform_tap(E.bx, i) : none;
    stage_row(D, E, i, j, nf, need, ax, abx, sm, lane);
  }
  __syncthreads();  // rows are wave-private, the z taps were written by every wave
  const size_t row = ((size_t)i * D.n1 + j) * D.n2;
  auto tap_at = [&](const int4* lds, const fsg_tap* tab, bool on, int k) {
    // NB: written as `if`, not `cond ? table[k] : none`: the ternary makes hipcc scalarise the 16-byte entry
    // into eight branchy dword loads (+35 % kernel time, measured)
    fsg_tap c = none;
    if (on) {
      if (taps_lds) { const int4 v = lds[k]; c = fsg_tap{v.x, v.y, __builtin_bit_cast(float, v.z), __builtin_bit_cast(float, v.w)}; }
      else c = tab[k];
    }
    return c;
  };
  // PATCH_NQ chunks of 64 voxels per step and lane: all their gathers are in flight before the first blend
  for (int kb = 0; kb < D.n2; kb += PATCH_NQ * FSG_WAVE) {
    const int kk = kb + lane;
    fsg_tap ck[4] = {none, none, none, none}, cbk[4] = {none, none, none, none};
#pragma unroll
    for (int q = 0; q < PATCH_NQ; ++q) {
      const int k = min(kk + 64 * q, D.n2 - 1);
      ck[q] = tap_at(s_tz, D.tz, D.field != nullptr, k);
      cbk[q] = tap_at(s_bz, E.bz, E.bias != nullptr, k);
    }
    if (live_row)
      warp_emitN<LT, HAS_LIN, HAS_NN, FAST, 0, PATCH_NQ>(D, E, m, sm, nf, i, j, kk, ck, cbk, row, src_lin, out_lin, src_nn,
                                                         out_nn);
    __syncthreads();  // keep the 16 waves on the same z chunks: bounded L1 working set, shared misses
  }
}

template <bool MIN_ONLY>
__device__ __forceinline__ void coords_minmax_rows_body(const FsgDeformK& D, int32_t* __restrict__ mm6, int rows_per_block, int blk);

template <bool MIN_ONLY>
__global__ __launch_bounds__(256) void coords_minmax_rows_kernel(FsgDeformK D, int32_t* __restrict__ mm6,
                                                                 int rows_per_block) {
  coords_minmax_rows_body<MIN_ONLY>(D, mm6, rows_per_block, (int)blockIdx.x);
}

template <bool MIN_ONLY>
__device__ __forceinline__ void coords_minmax_rows_body(const FsgDeformK& D, int32_t* __restrict__ mm6, int rows_per_block, int blk) {
  if (MIN_ONLY) {  // floor(min) already known to be 0 on every axis: nothing to add (block-uniform exit)
    const int32_t one = fsg_f2key(1.0f);
    const int32_t k0 = __hip_atomic_load(&mm6[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t k1 = __hip_atomic_load(&mm6[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t k2 = __hip_atomic_load(&mm6[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k0 < one && k1 < one && k2 < one) return;
  }
  __shared__ float sm_all[4][ROWCAP];
  __shared__ float red[6][4];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  float* sm = sm_all[wave];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int rows = D.n0 * D.n1;
  const int r_begin = blk * rows_per_block;
  const int r_end = min(rows, r_begin + rows_per_block);
  const fsg_tap none = fsg_tap{0, 0, 0.f, 0.f};
  const bool cached = D.n2 <= 256;
  fsg_tap ck[4];
  if (cached) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = lane + 64 * q;
      ck[q] = (D.field && k < D.n2) ? D.tz[k] : none;
    }
  }
  for (int r = r_begin + wave; r < r_end; r += 4) {
    const int i = r / D.n1, j = r - i * D.n1;
    if (D.rows) {
      const float* rr = D.rows + (size_t)r * D.row_stride;
      for (int e = lane; e < 3 * D.f2; e += FSG_WAVE) sm[e] = rr[e];
    } else if (D.field) {
      fill_row_xy<3>(D.field, D.f1, D.f2, fsg_uniform_tap(D.tx, i), fsg_uniform_tap(D.ty, j), sm, lane);
    }
    fsg_wave_lds_sync();
    if (cached) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = lane + 64 * q;
        if (k < D.n2) {
          float x, y, z;
          row_position(D, sm, i, j, k, ck[q], x, y, z);
          lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
          lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
          lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
        }
      }
    } else {
      for (int k = lane; k < D.n2; k += FSG_WAVE) {
        float x, y, z;
        row_position(D, sm, i, j, k, D.field ? D.tz[k] : none, x, y, z);
        lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
        lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
        lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
      }
    }
    fsg_wave_lds_sync();
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float l = fsg_wave_min(lo[a]), h = fsg_wave_max(hi[a]);
    if (lane == 0) { red[a][wave] = l; red[3 + a][wave] = h; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float v = red[a][0];
    for (int w = 1; w < 4; ++w) v = a < 3 ? fminf(v, red[a][w]) : fmaxf(v, red[a][w]);
    if (a < 3) fsg_atomic_min_key(&mm6[a], v);
    else if (!MIN_ONLY) fsg_atomic_max_key(&mm6[a], v);
  }
}

// ---- fused warp -------------------------------------------------------------------------------
template <typename LT>
__global__ __launch_bounds__(256) void warp_kernel(FsgDeformK D, const int32_t* __restrict__ mm6,
                                                   const float* __restrict__ src_lin, float* __restrict__ out_lin,
                                                   const LT* __restrict__ src_nn, LT* __restrict__ out_nn, EpiK E) {
  const int k = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, i = blockIdx.z;
  if (k >= D.n2 || j >= D.n1) return;
  const Margins m = load_margins(mm6);
  float x, y, z;
  fsg_position(D, i, j, k, x, y, z);
  x = x - m.mx;
  y = y - m.my;
  z = z - m.mz;
  const size_t o = ((size_t)i * D.n1 + j) * D.n2 + k;
  if (src_nn) out_nn[o] = sample_nearest<LT>(src_nn, D, x, y, z);
  if (src_lin) {
    float v = sample_linear(src_lin, D, x, y, z);
    if (E.gamma > 0.f) v = 300.0f * powf(v / 300.0f, E.gamma);
    if (E.bias) {
      const float b = fsg_tab_interp<1>(E.bias, E.b1, E.b2, 0, E.bx[i], E.by[j], E.bz[k]);
      v = v * expf(b);
    }
    out_lin[o] = v;
  }
}

// ---- operand checks of the fused-warp entry points ----------------------------------------------------------------------------
// What fsg_warp_f32 / _u8 (launch_warp), fsg_warp_f32_u8_to_f32 and fsg_warp_dual_f32 all refuse, before any launch: a bad
// deformation (fsg_fill_deform's own code, FSG_E_TOOBIG included, first in all three), then with FSG_E_BADARG a null mm6, one of
// a source / destination pair without the other, no source at all (the dual entry point needs src_lin, so it refuses that too)
// and a bad epilogue.  Every refusal after the deformation's is FSG_E_BADARG, so their order among themselves shows nowhere.
static int warp_operands(const fsg_deform* d, const fsg_epilogue* epi, const int32_t* mm6, const void* src_lin,
                         const void* out_lin, const void* src_nn, const void* out_nn, FsgDeformK& D, EpiK& E) {
  const int rc = fsg_fill_deform(d, D);
  if (rc) return rc;
  if (!mm6) return FSG_E_BADARG;
  if ((src_lin == nullptr) != (out_lin == nullptr)) return FSG_E_BADARG;
  if ((src_nn == nullptr) != (out_nn == nullptr)) return FSG_E_BADARG;
  if (!src_lin && !src_nn) return FSG_E_BADARG;
  return fill_epilogue(epi, E);
}

// Two more that launch_warp and fsg_warp_dual_f32 make and fsg_warp_f32_u8_to_f32 does NOT: the trilinear source warped onto
// itself, and precomputed rows narrower than the coarse values of a row.  (_u8_to_f32 launches the first as it is, and for the
// second gets FSG_E_ALIGN from the lean launcher where the other two answer FSG_E_BADARG.  Not unified here.)
static int warp_alias_rows(const FsgDeformK& D, const EpiK& E, const void* src_lin, const void* out_lin) {
  if (src_lin && src_lin == out_lin) return FSG_E_BADARG;
  const int need = (D.field ? 3 * D.f2 : 0) + (E.bias ? E.b2 : 0);
  if (D.rows && D.row_stride < need) return FSG_E_BADARG;
  return 0;
}

template <typename LT>
int launch_warp(const fsg_deform* d, const int32_t* mm6, const float* src_lin, float* out_lin, const LT* src_nn,
                LT* out_nn, const fsg_epilogue* epi, void* stream) {
  FsgDeformK D;
  EpiK E;
  int rc = warp_operands(d, epi, mm6, src_lin, out_lin, src_nn, out_nn, D, E);
  if (!rc) rc = warp_alias_rows(D, E, src_lin, out_lin);
  if (rc) return rc;
  const int need = (D.field ? 3 * D.f2 : 0) + (E.bias ? E.b2 : 0);
  if (!(g_tuning_flags & (FSG_TUNE_GENERIC_WARP | FSG_TUNE_NO_PATCH | FSG_TUNE_NO_LEAN))) {
    // default: the lean body (fsg_warp_lean.hip); FSG_E_ALIGN = configuration outside its domain
    rc = fsg_launch_warp_lean(D, E, mm6, src_lin, out_lin, src_nn, out_nn, (int)sizeof(LT), (int)sizeof(LT),
                              !(g_tuning_flags & FSG_TUNE_PRECISE_MATH), stream);
    if (rc != FSG_E_ALIGN) return rc;
  }
  if (need <= PATCH_ROWCAP && D.n2 >= 2 && !(g_tuning_flags & (FSG_TUNE_GENERIC_WARP | FSG_TUNE_NO_PATCH))) {
    const int ntiles = ((D.n0 + PATCH - 1) / PATCH) * ((D.n1 + PATCH - 1) / PATCH);
    const bool fast = !(g_tuning_flags & FSG_TUNE_PRECISE_MATH);
    const dim3 grid((unsigned)ntiles), block(1024);
    hipStream_t st = fsg_stream(stream);
#define FSG_LAUNCH_PATCH(L, N, F) \
  hipLaunchKernelGGL((warp_patch_kernel<LT, L, N, F>), grid, block, 0, st, D, mm6, src_lin, out_lin, src_nn, out_nn, E)
    FSG_WARP_LADDER(FSG_LAUNCH_PATCH, src_lin, src_nn, fast);
#undef FSG_LAUNCH_PATCH
    FSG_RETURN_LAUNCH();
  }
  if (need <= ROWCAP && D.n2 >= 2 && !(g_tuning_flags & FSG_TUNE_GENERIC_WARP)) {
#if FSG_WARP_MAP == 2
    const int tiles_j = (D.n1 + 2 * WARP_ROWS_PER_WAVE - 1) / (2 * WARP_ROWS_PER_WAVE);
    const int ntiles = ((D.n0 + 1) / 2) * tiles_j;
#else
    const int tiles_j = (D.n1 + 4 * WARP_ROWS_PER_WAVE - 1) / (4 * WARP_ROWS_PER_WAVE);
    const int ntiles = D.n0 * tiles_j;
#endif
    const bool fast = !(g_tuning_flags & FSG_TUNE_PRECISE_MATH);
    const dim3 grid((unsigned)ntiles), block(256);
    hipStream_t st = fsg_stream(stream);
#define FSG_LAUNCH_WARP(L, N, F) \
  hipLaunchKernelGGL((warp_rows_kernel<LT, L, N, F>), grid, block, 0, st, D, mm6, src_lin, out_lin, src_nn, out_nn, E)
    FSG_WARP_LADDER(FSG_LAUNCH_WARP, src_lin, src_nn, fast);
#undef FSG_LAUNCH_WARP
    FSG_RETURN_LAUNCH();
  }
  hipLaunchKernelGGL(warp_kernel<LT>, fsg_grid3(D.n0, D.n1, D.n2), fsg_block3(), 0, fsg_stream(stream), D, mm6,
                     src_lin, out_lin, src_nn, out_nn, E);
  FSG_RETURN_LAUNCH();
}

// ---- generic gather with explicit coordinates ---------------------------------------------------
__global__ __launch_bounds__(256) void interp_kernel(const float* __restrict__ src, int sx, int sy, int sz,
                                                     const float* __restrict__ ii, const float* __restrict__ jj,
                                                     const float* __restrict__ kk, size_t npts, int mode,
                                                     float defval, float* __restrict__ dst) {
  FsgDeformK D;
  D.n0 = sx; D.n1 = sy; D.n2 = sz; D.flip = 0;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < npts; p += (size_t)gridDim.x * blockDim.x) {
    const float x = ii[p], y = jj[p], z = kk[p];
    if (mode == 1) {
      dst[p] = sample_nearest<float>(src, D, x, y, z);
    } else {
      const float hx = (float)(sx - 1), hy = (float)(sy - 1), hz = (float)(sz - 1);
      const bool ok = (x > 0.f) && (y > 0.f) && (z > 0.f) && (x <= hx) && (y <= hy) && (z <= hz);
      dst[p] = ok ? sample_linear(src, D, x, y, z) : defval;
    }
  }
}

__global__ void mm_init_kernel(int32_t* mm, int nmin, int nmax) {
  const int t = threadIdx.x;
  if (t < nmin) mm[t] = fsg_f2key(INFINITY);
  else if (t < nmin + nmax) mm[t] = fsg_f2key(-INFINITY);
}

}  // namespace

extern "C" {

int fsg_set_tuning(int flags) {
  const int prev = g_tuning_flags;
  g_tuning_flags = flags;
  return prev;
}

extern int g_lean_pace, g_lean_ablate;
int fsg_warp_set_variant(int variant) {
  const int prev = g_lean_pace < 0 ? 0 : (g_lean_pace == 0 ? 5 : (g_lean_pace == 2 ? 6 : 7));
#ifdef FSG_DIAG  // the ablation kernels (wrong results by construction) exist in a -DFSG_DIAG build only
  if (variant == 8 || variant == 9) { g_lean_pace = 1; g_lean_ablate = variant - 7; return prev; }
#endif
  if (variant != 0 && (variant < 5 || variant > 7)) return FSG_E_BADARG;
  g_lean_ablate = 0;
  g_lean_pace = variant == 0 ? -1 : (variant == 5 ? 0 : (variant == 6 ? 2 : 1));
  return prev;
}

int fsg_minmax_init(int32_t* mm, int nmin, int nmax, void* stream) {
  if (!mm || nmin < 0 || nmax < 0 || nmin + nmax <= 0 || nmin + nmax > 64) return FSG_E_BADARG;
  hipLaunchKernelGGL(mm_init_kernel, dim3(1), dim3(64), 0, fsg_stream(stream), mm, nmin, nmax);
  FSG_RETURN_LAUNCH();
}

int fsg_deform_rows_f32(const fsg_deform* d, const fsg_epilogue* epi, float* rows, int row_stride, void* stream) {
  FsgDeformK D;
  int rc = fsg_fill_deform(d, D);
  if (rc) return rc;
  EpiK E;
  rc = fill_epilogue(epi, E);
  if (rc) return rc;
  const int need = (D.field ? 3 * D.f2 : 0) + (E.bias ? E.b2 : 0);
  if (!rows || row_stride < need) return FSG_E_BADARG;
  if (need == 0) return 0;
  if (D.n0 > 65535) return FSG_E_TOOBIG;
  if (rows_block_fits(D, E) && !(g_tuning_flags & FSG_TUNE_SPLIT_HEAD)) {
    const dim3 grid((unsigned)((D.n1 + RB_J - 1) / RB_J), (unsigned)D.n0);
    hipLaunchKernelGGL(deform_rows_block_kernel, grid, dim3(256), 0, fsg_stream(stream), D, E, rows, row_stride);
    FSG_RETURN_LAUNCH();
  }
  const dim3 grid((unsigned)((D.n1 * need + 255) / 256), (unsigned)D.n0);
  hipLaunchKernelGGL(deform_rows_kernel, grid, dim3(256), 0, fsg_stream(stream), D, E, rows, row_stride);
  FSG_RETURN_LAUNCH();
}

int fsg_coords_minmax_f32(const fsg_deform* d, int32_t* mm6, void* stream) {
  FsgDeformK D;
  int rc = fsg_fill_deform(d, D);
  if (rc) return rc;
  if (!mm6) return FSG_E_BADARG;
  const int rows = D.n0 * D.n1;
  if ((D.field ? 3 * D.f2 : 0) <= ROWCAP && !(g_tuning_flags & FSG_TUNE_GENERIC_WARP)) {
    int grid = (int)fsg_blocks((size_t)rows, 8, 2048);
    const int rpb = (rows + grid - 1) / grid;
    grid = (rows + rpb - 1) / rpb;
    hipLaunchKernelGGL(coords_minmax_rows_kernel<false>, dim3(grid), dim3(256), 0, fsg_stream(stream), D, mm6, rpb);
    FSG_RETURN_LAUNCH();
  }
  const int grid = rows < 2048 ? rows : 2048;
  hipLaunchKernelGGL(coords_minmax_kernel, dim3(grid), dim3(256), 0, fsg_stream(stream), D, mm6);
  FSG_RETURN_LAUNCH();
}

int fsg_coords_floormin_f32(const fsg_deform* d, int32_t* mm3, void* stream) {
  FsgDeformK D;
  int rc = fsg_fill_deform(d, D);
  if (rc) return rc;
  if (!mm3) return FSG_E_BADARG;
  hipStream_t st = fsg_stream(stream);
  const int faces = faces_total(D.n0, D.n1, D.n2);
  hipLaunchKernelGGL(coords_faces_min_kernel, dim3(fsg_blocks((size_t)faces, 256, 1024)), dim3(256), 0, st, D, mm3);
  const int rows = D.n0 * D.n1;
  if ((D.field ? 3 * D.f2 : 0) <= ROWCAP) {
    // 512 workgroups: in the usual case every one of them exits on its first instruction, and fewer of them
    // exit sooner; the rare full pass runs at a quarter of the parallelism, which is fine
    int grid = (int)fsg_blocks((size_t)rows, 8, 512);
    const int rpb = (rows + grid - 1) / grid;
    grid = (rows + rpb - 1) / rpb;
    hipLaunchKernelGGL(coords_minmax_rows_kernel<true>, dim3(grid), dim3(256), 0, st, D, mm3, rpb);
  } else {
    // very large coarse grids: exact per-voxel pass (writes the maxima after the three minima too)
    return FSG_E_TOOBIG;
  }
  FSG_RETURN_LAUNCH();
}

int fsg_coords_floormin_rest_f32(const fsg_deform* d, int32_t* mm3, void* stream) {
  FsgDeformK D;
  int rc = fsg_fill_deform(d, D);
  if (rc) return rc;
  if (!mm3) return FSG_E_BADARG;
  if ((D.field ? 3 * D.f2 : 0) > ROWCAP) return FSG_E_TOOBIG;
  const int rows = D.n0 * D.n1;
  int grid = (int)fsg_blocks((size_t)rows, 8, 512);
  const int rpb = (rows + grid - 1) / grid;
  grid = (rows + rpb - 1) / rpb;
  hipLaunchKernelGGL(coords_minmax_rows_kernel<true>, dim3(grid), dim3(256), 0, fsg_stream(stream), D, mm3, rpb);
  FSG_RETURN_LAUNCH();
}

static int launch_sample_head(const HeadGmm& G, size_t n, const fsg_deform* d, const fsg_epilogue* epi, float* rows,
                              int row_stride, int32_t* mm3, const void* drawk, unsigned draw_blocks, void* stream);

// ---- internal entry points of fsg_pipeline.cpp (not part of include/fsg_hip.h) ------------------------------------------------
// The one-launch head with the look-ahead's job beside it: drawk (a fsg_ride::DrawK on the host, NULL = none) is the NEXT
// sample's keyed draw job of draw_blocks workgroups, 1 .. FSG_HEAD_DRAW_MAX (the caller launches a larger job on its own).
// fsg_internal_head_no_gmm: a sample whose intensities are given (fsg_sample_image::prior_in) -- rows and faces jobs, no GMM job.
extern "C" int fsg_internal_head_no_gmm(size_t n, const fsg_deform* d, const fsg_epilogue* epi, float* rows, int row_stride,
                                        int32_t* mm3, const void* drawk, unsigned draw_blocks, void* stream) {
  if (n == 0 || !mm3) return FSG_E_BADARG;
  HeadGmm G{};  // G.out == nullptr: no workgroup is launched for the GMM job
  G.n = n;
  return launch_sample_head(G, n, d, epi, rows, row_stride, mm3, drawk, draw_blocks, stream);
}

extern "C" int fsg_internal_head_f32(const uint8_t* l0, const uint8_t* l1, const uint8_t* l2, const uint8_t* l3, size_t n,
                                     const float* mus, const float* sigmas, int ntab, const float* noise, uint64_t seed,
                                     uint64_t stream_id, float* out, const fsg_deform* d, const fsg_epilogue* epi, float* rows,
                                     int row_stride, int32_t* mm3, const void* drawk, unsigned draw_blocks, void* stream) {
  if (n == 0 || !l0 || !mus || !sigmas || !out || ntab <= 0 || ntab > 256 || !mm3) return FSG_E_BADARG;
  const uintptr_t al = (uintptr_t)l0 | (uintptr_t)l1 | (uintptr_t)l2 | (uintptr_t)l3;
  if ((al & 3) || ((uintptr_t)out & 15)) return FSG_E_ALIGN;
  HeadGmm G{l0, l1, l2, l3, n, mus, sigmas, ntab, noise, seed, stream_id, out, 0, 0, 0u};
  return launch_sample_head(G, n, d, epi, rows, row_stride, mm3, drawk, draw_blocks, stream);
}

extern "C" int fsg_internal_head_codes_f32(const uint16_t* codes, const uint8_t* tuples, int ntuples, int stride,
                                           const int32_t sel[4], size_t n, const float* mus, const float* sigmas, int ntab,
                                           uint64_t seed, uint64_t stream_id, float* out, const fsg_deform* d,
                                           const fsg_epilogue* epi, float* rows, int row_stride, int32_t* mm3, const void* drawk,
                                           unsigned draw_blocks, void* stream) {
  if (n == 0 || !codes || !tuples || !sel || !mus || !sigmas || !out || ntab <= 0 || ntab > 256 || !mm3) return FSG_E_BADARG;
  if (ntuples <= 0 || stride <= 0 || stride > 256) return FSG_E_BADARG;
  for (int m = 0; m < 4; ++m)
    if (sel[m] < 0 || sel[m] >= stride) return FSG_E_BADARG;
  if (ntuples > FSG_CODES_MAX || n > ((size_t)1 << 30)) return FSG_E_TOOBIG;
  if ((n & 7) || ((uintptr_t)codes & 15) || ((uintptr_t)out & 15)) return FSG_E_ALIGN;
  HeadGmm G{reinterpret_cast<const uint8_t*>(codes), tuples, nullptr, nullptr, n, mus, sigmas, ntab, nullptr, seed, stream_id, out,
            ntuples, stride, (uint32_t)sel[0] | ((uint32_t)sel[1] << 8) | ((uint32_t)sel[2] << 16) | ((uint32_t)sel[3] << 24)};
  return launch_sample_head(G, n, d, epi, rows, row_stride, mm3, drawk, draw_blocks, stream);
}

int fsg_sample_head_f32(const uint8_t* l0, const uint8_t* l1, const uint8_t* l2, const uint8_t* l3, size_t n,
                        const float* mus, const float* sigmas, int ntab, const float* noise, uint64_t seed,
                        uint64_t stream_id, float* out, const fsg_deform* d, const fsg_epilogue* epi, float* rows,
                        int row_stride, int32_t* mm3, void* stream) {
  return fsg_internal_head_f32(l0, l1, l2, l3, n, mus, sigmas, ntab, noise, seed, stream_id, out, d, epi, rows, row_stride, mm3,
                               nullptr, 0u, stream);
}

int fsg_sample_head_codes_f32(const uint16_t* codes, const uint8_t* tuples, int ntuples, int stride, const int32_t sel[4],
                              size_t n, const float* mus, const float* sigmas, int ntab, uint64_t seed, uint64_t stream_id,
                              float* out, const fsg_deform* d, const fsg_epilogue* epi, float* rows, int row_stride,
                              int32_t* mm3, void* stream) {
  return fsg_internal_head_codes_f32(codes, tuples, ntuples, stride, sel, n, mus, sigmas, ntab, seed, stream_id, out, d, epi, rows,
                                     row_stride, mm3, nullptr, 0u, stream);
}

static int launch_sample_head(const HeadGmm& G, size_t n, const fsg_deform* d, const fsg_epilogue* epi, float* rows,
                              int row_stride, int32_t* mm3, const void* drawk, unsigned draw_blocks, void* stream) {
  FsgDeformK D;
  int rc = fsg_fill_deform(d, D);
  if (rc) return rc;
  EpiK E;
  rc = fill_epilogue(epi, E);
  if (rc) return rc;
  if (drawk ? (draw_blocks == 0 || draw_blocks > FSG_HEAD_DRAW_MAX) : draw_blocks != 0) return FSG_E_BADARG;
  const int need = (D.field ? 3 * D.f2 : 0) + (E.bias ? E.b2 : 0);
  if (need > 0 && (!rows || row_stride < need)) return FSG_E_BADARG;
  if ((size_t)D.n0 * D.n1 * D.n2 != n) return FSG_E_BADARG;
  if ((D.field ? 3 * D.f2 : 0) > ROWCAP) return FSG_E_TOOBIG;
  if (!rows_block_fits(D, E)) return FSG_E_TOOBIG;
  const int rows_gx = need > 0 ? (D.n1 + RB_J - 1) / RB_J : 0;
  const long long nrows = (long long)rows_gx * D.n0;
  const int faces = faces_total(D.n0, D.n1, D.n2);
  const int nfaces = (int)fsg_blocks((size_t)faces, 256, 1024);
  // No GMM job without an output (fsg_internal_head_no_gmm).  Cap 4 096, 4 groups per thread: 33.8 us (8 192: 34.8,
  // 16 384: 39.0); codes mode, 2 x 8 voxels per thread: 30.5 us (1 024: 34.7, 2 048: 37.0, 8 192: 33.6)
  const unsigned ngmm = G.out ? fsg_blocks((n + 3) / 4, 256, 4096) : 0u;
  if (nrows > 1000000) return FSG_E_TOOBIG;
  static const fsg_ride::DrawK no_draw = {};
  hipLaunchKernelGGL(sample_head_kernel, dim3((unsigned)(nrows + nfaces + ngmm) + draw_blocks), dim3(256), 0, fsg_stream(stream), G,
                     D, E, rows, row_stride, rows_gx > 0 ? rows_gx : 1, (int)nrows, nfaces, mm3, (int)draw_blocks,
                     drawk ? *reinterpret_cast<const fsg_ride::DrawK*>(drawk) : no_draw);
  FSG_RETURN_LAUNCH();
}

int fsg_coords_f32(const fsg_deform* d, const int32_t* mm6, float* xx, float* yy, float* zz, void* stream) {
  FsgDeformK D;
  int rc = fsg_fill_deform(d, D);
  if (rc) return rc;
  if (!mm6 || !xx || !yy || !zz) return FSG_E_BADARG;
  hipLaunchKernelGGL(coords_kernel, fsg_grid3(D.n0, D.n1, D.n2), fsg_block3(), 0, fsg_stream(stream), D, mm6, xx,
                     yy, zz);
  FSG_RETURN_LAUNCH();
}

int fsg_warp_f32(const fsg_deform* d, const int32_t* mm6, const float* src_lin, float* out_lin,
                 const float* src_nn, float* out_nn, const fsg_epilogue* epi, void* stream) {
  return launch_warp<float>(d, mm6, src_lin, out_lin, src_nn, out_nn, epi, stream);
}

int fsg_warp_f32_u8(const fsg_deform* d, const int32_t* mm6, const float* src_lin, float* out_lin,
                    const uint8_t* src_nn, uint8_t* out_nn, const fsg_epilogue* epi, void* stream) {
  return launch_warp<uint8_t>(d, mm6, src_lin, out_lin, src_nn, out_nn, epi, stream);
}

int fsg_warp_f32_u8_to_f32(const fsg_deform* d, const int32_t* mm6, const float* src_lin, float* out_lin,
                           const uint8_t* src_nn, float* out_nn, const fsg_epilogue* epi, void* stream) {
  FsgDeformK D;
  EpiK E;
  const int rc = warp_operands(d, epi, mm6, src_lin, out_lin, src_nn, out_nn, D, E);
  if (rc) return rc;
  // (no warp_alias_rows here: see there)
  if (g_tuning_flags & (FSG_TUNE_GENERIC_WARP | FSG_TUNE_NO_PATCH | FSG_TUNE_NO_LEAN)) return FSG_E_ALIGN;
  // served by the lean kernel alone (the uint8 -> uint8 case reaches it through launch_warp)
  return fsg_launch_warp_lean(D, E, mm6, src_lin, out_lin, src_nn, out_nn, 1, 4, !(g_tuning_flags & FSG_TUNE_PRECISE_MATH),
                              stream);
}

int fsg_warp_dual_f32(const fsg_deform* d, const int32_t* mm6, const float* src_lin, float* out_lin, const float* src_img,
                      float* out_img, size_t img_voxels, const void* src_nn, void* out_nn, int label_dtype_in, int label_dtype_out,
                      const fsg_epilogue* epi, void* stream) {
  FsgDeformK D;
  EpiK E;
  int rc = warp_operands(d, epi, mm6, src_lin, out_lin, src_nn, out_nn, D, E);
  if (!rc) rc = warp_alias_rows(D, E, src_lin, out_lin);
  if (rc) return rc;
  if (!src_lin) return FSG_E_BADARG;  // the labels alone are fsg_warp_f32 / _u8's
  if ((src_img == nullptr) != (out_img == nullptr)) return FSG_E_BADARG;
  if (src_img && (img_voxels != (size_t)D.n0 * D.n1 * D.n2 || out_img == src_img || out_img == src_lin || out_img == out_lin ||
                  out_lin == src_img))  // an output over a source other lanes still gather from
    return FSG_E_BADARG;
  const int lin = label_dtype_in == FSG_LABEL_F32 ? 4 : label_dtype_in == FSG_LABEL_U8 ? 1 : 0;
  const int lout = label_dtype_out == FSG_LABEL_F32 ? 4 : label_dtype_out == FSG_LABEL_U8 ? 1 : 0;
  if (src_nn && (!lin || !lout || (lin == 4 && lout == 1))) return FSG_E_BADARG;
  if (g_tuning_flags & (FSG_TUNE_GENERIC_WARP | FSG_TUNE_NO_PATCH | FSG_TUNE_NO_LEAN)) return FSG_E_ALIGN;
  return fsg_launch_warp_lean(D, E, mm6, src_lin, out_lin, src_nn, out_nn, src_nn ? lin : 4, src_nn ? lout : 4,
                              !(g_tuning_flags & FSG_TUNE_PRECISE_MATH), stream, src_img, out_img);
}

int fsg_interp3d_f32(const float* src, int sx, int sy, int sz, const float* ii, const float* jj, const float* kk,
                     size_t npts, int mode, float defval, float* dst, void* stream) {
  if (!src || !ii || !jj || !kk || !dst || sx <= 0 || sy <= 0 || sz <= 0) return FSG_E_BADARG;
  if (mode != 0 && mode != 1) return FSG_E_BADARG;
  if ((size_t)sx * sy * sz > (size_t)0x7FFFFFFF) return FSG_E_TOOBIG;
  if (npts == 0) return 0;
  hipLaunchKernelGGL(interp_kernel, dim3(fsg_blocks(npts, 256, 8192)), dim3(256), 0, fsg_stream(stream), src, sx, sy, sz, ii,
                     jj, kk, npts, mode, defval, dst);
  FSG_RETURN_LAUNCH();
}

}  // extern "C"
