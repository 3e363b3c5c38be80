// fsg_tk1.hip -- out = t + lam * L p, the first-order (TK1 / Huber-reweighted) regulariser of the srr solve.
//
// L is the weighted graph Laplacian of the 6-neighbour grid restricted to the voxels of the mask; include/fsg_hip.h states which
// edges take part, the edge weight and the order of the fp32 operations.  A gather: every thread reads p (and the guide, the
// mask) around its four voxels and writes those four alone, so there are no atomics, no LDS, no allocation and no host
// synchronisation, and the result is the same bits whichever of the load paths ran.  The overlap test is fsg_common.h's.
#include "fsg_common.h"
#include <cmath>

namespace {

constexpr int TK_THREADS = 256;

// One thread owns the four consecutive elements e .. e + 3 of the flat volume (x fastest).  Its x neighbours are its own registers
// plus the two elements p[e - 1], p[e + 4]; its y and z neighbours come from cached loads of the rows W and H * W away.
//   VEC   every float pointer is 16-byte aligned, mask 4-byte aligned: the thread's own group moves as one 16-byte word.
//   ROW4  VEC and W % 4 == 0: a group never crosses a row end, so y and z are the group's and the four neighbour rows are 16-byte
//         words too.  Otherwise each element has its own (x, y, z) and its neighbours are scalar loads.
template <bool VEC, bool ROW4>
__global__ __launch_bounds__(TK_THREADS) void tk1_apply_kernel(const float* __restrict__ p, const float* t,
                                                               const uint8_t* __restrict__ mask, const float* __restrict__ g,
                                                               float delta, float lam, uint32_t H, uint32_t W, uint32_t n,
                                                               float* out) {
  const uint32_t grp = (uint32_t)xcd_tile((int)blockIdx.x, (int)gridDim.x) * TK_THREADS + threadIdx.x;
  if (grp >= ((n + 3) >> 2)) return;
  const uint32_t e = grp << 2, HW = H * W;
  const int cnt = n - e < 4 ? (int)(n - e) : 4;
  const bool full = VEC && cnt == 4;

  float vp[4], vt[4], vg[4] = {0.f, 0.f, 0.f, 0.f}, np[6][4], ngd[6][4];
  bool keep[4], on[6][4];
  if (full) {
    const float4 a = *reinterpret_cast<const float4*>(p + e), b = *reinterpret_cast<const float4*>(t + e);
    vp[0] = a.x; vp[1] = a.y; vp[2] = a.z; vp[3] = a.w;
    vt[0] = b.x; vt[1] = b.y; vt[2] = b.z; vt[3] = b.w;
    if (g) {
      const float4 c = *reinterpret_cast<const float4*>(g + e);
      vg[0] = c.x; vg[1] = c.y; vg[2] = c.z; vg[3] = c.w;
    }
    const uint32_t m = mask ? *reinterpret_cast<const uint32_t*>(mask + e) : 0x01010101u;
#pragma unroll
    for (int j = 0; j < 4; ++j) keep[j] = ((m >> (8 * j)) & 255u) != 0;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = j < cnt;
      vp[j] = in ? p[e + j] : 0.f;
      vt[j] = in ? t[e + j] : 0.f;
      if (g) vg[j] = in ? g[e + j] : 0.f;
      keep[j] = in && (!mask || mask[e + j] != 0);
    }
  }

  // (x, y, z) of the four elements
  uint32_t x[4], y[4], z[4];
  {
    const uint32_t row = e / W;
    x[0] = e - row * W; y[0] = row % H; z[0] = row / H;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      if (ROW4) {
        x[j] = x[0] + j; y[j] = y[0]; z[j] = z[0];
      } else {
        const uint32_t r = (e + j) / W;
        x[j] = (e + j) - r * W; y[j] = r % H; z[j] = r / H;
      }
    }
  }

  // x-, x+: the group's own registers and one element on either side
  {
    const bool lo = x[0] > 0, hi = cnt == 4 && x[3] + 1 < W;  // then e - 1 >= 0 and e + 4 < n
    const float pl = lo ? p[e - 1] : 0.f, ph = hi ? p[e + 4] : 0.f;
    const float gl = (g && lo) ? g[e - 1] : 0.f, gh = (g && hi) ? g[e + 4] : 0.f;
    const bool kl = lo && (!mask || mask[e - 1] != 0), kh = hi && (!mask || mask[e + 4] != 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      np[0][j] = j > 0 ? vp[j - 1] : pl;
      ngd[0][j] = j > 0 ? vg[j - 1] : gl;
      on[0][j] = x[j] > 0 && (j > 0 ? keep[j - 1] : kl);
      np[1][j] = j < 3 ? vp[j + 1] : ph;
      ngd[1][j] = j < 3 ? vg[j + 1] : gh;
      on[1][j] = x[j] + 1 < W && (j < 3 ? keep[j + 1] : kh);  // x + 1 < W puts element e + j + 1 inside the volume, so j + 1 < cnt
    }
  }

  // y-, y+, z-, z+
  if (ROW4) {
    const bool has[4] = {y[0] > 0, y[0] + 1 < H, z[0] > 0, e + HW < n};
    const uint32_t at[4] = {e - W, e + W, e - HW, e + HW};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
      uint32_t m = 0;
      if (has[d]) {
        a = *reinterpret_cast<const float4*>(p + at[d]);
        if (g) c = *reinterpret_cast<const float4*>(g + at[d]);
        m = mask ? *reinterpret_cast<const uint32_t*>(mask + at[d]) : 0x01010101u;
      }
      np[2 + d][0] = a.x; np[2 + d][1] = a.y; np[2 + d][2] = a.z; np[2 + d][3] = a.w;
      ngd[2 + d][0] = c.x; ngd[2 + d][1] = c.y; ngd[2 + d][2] = c.z; ngd[2 + d][3] = c.w;
#pragma unroll
      for (int j = 0; j < 4; ++j) on[2 + d][j] = ((m >> (8 * j)) & 255u) != 0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t i = e + j;
      const bool in = j < cnt;
      const bool has[4] = {in && y[j] > 0, in && y[j] + 1 < H, in && z[j] > 0, in && i + HW < n};
      const uint32_t at[4] = {i - W, i + W, i - HW, i + HW};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        np[2 + d][j] = has[d] ? p[at[d]] : 0.f;
        ngd[2 + d][j] = (g && has[d]) ? g[at[d]] : 0.f;
        on[2 + d][j] = has[d] && (!mask || mask[at[d]] != 0);
      }
    }
  }

  float vo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
      if (on[d][j]) {
        float df = vp[j] - np[d][j];
        if (g) {
          const float a = fabsf(vg[j] - ngd[d][j]);
          const float c = a <= delta ? 1.f : delta / a;
          df = c * df;
        }
        acc = acc + df;
      }
    }
    const float s = lam * acc;
    vo[j] = keep[j] ? vt[j] + s : vt[j];
  }
  if (full) {
    *reinterpret_cast<float4*>(out + e) = make_float4(vo[0], vo[1], vo[2], vo[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < cnt) out[e + j] = vo[j];
  }
}

}  // namespace

extern "C" int fsg_tk1_apply_f32(const float* p, const float* t, const uint8_t* mask, const float* guide, float delta, float lam,
                                 int D, int H, int W, float* out, void* stream) {
  if (!p || !t || !out || D < 1 || H < 1 || W < 1) return FSG_E_BADARG;
  if (!std::isfinite(lam) || lam < 0.f) return FSG_E_BADARG;
  if (guide && (!std::isfinite(delta) || !(delta > 0.f))) return FSG_E_BADARG;
  const size_t n = (size_t)D * H * W;
  if (n > (size_t)0x7FFFFFFF) return FSG_E_TOOBIG;
  const size_t nb = n * sizeof(float);
  if (fsg_overlap(out, nb, p, nb) || fsg_overlap(out, nb, guide, nb) || fsg_overlap(out, nb, mask, n)) return FSG_E_BADARG;
  if (out != t && fsg_overlap(out, nb, t, nb)) return FSG_E_BADARG;
  const dim3 grid((unsigned)((((n + 3) >> 2) + TK_THREADS - 1) / TK_THREADS)), block(TK_THREADS);
  const bool vec = ((((uintptr_t)p | (uintptr_t)t | (uintptr_t)guide | (uintptr_t)out) & 15) == 0) && ((uintptr_t)mask & 3) == 0;
  const uint32_t h = (uint32_t)H, w = (uint32_t)W, nn = (uint32_t)n;
  if (vec && (W & 3) == 0)
    hipLaunchKernelGGL((tk1_apply_kernel<true, true>), grid, block, 0, fsg_stream(stream), p, t, mask, guide, delta, lam, h, w, nn, out);
  else if (vec)
    hipLaunchKernelGGL((tk1_apply_kernel<true, false>), grid, block, 0, fsg_stream(stream), p, t, mask, guide, delta, lam, h, w, nn, out);
  else
    hipLaunchKernelGGL((tk1_apply_kernel<false, false>), grid, block, 0, fsg_stream(stream), p, t, mask, guide, delta, lam, h, w, nn, out);
  FSG_RETURN_LAUNCH();
}
