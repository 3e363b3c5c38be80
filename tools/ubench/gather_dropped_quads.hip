// Microbenchmark: what a raw-buffer gather costs the TA/TCP path when some of its lanes are sent OUT OF RANGE of the buffer
// descriptor (the range check drops them: they read 0 without an access).  The instruction is issued by every lane on every
// trip, as in the fused warp; only the offsets differ.  Lane shape as in gather_slope_cost.hip: 2 rows x 32 lanes on a
// slanted line, data L1/L2 resident (16 KB window per workgroup, read-only), 32 waves per CU.
//   byte gather:   lanes 1 byte apart, rows 256 bytes apart (the uint8 label twin of a 256^3 volume)
//   8-byte gather: lanes 4 bytes apart, rows 1 KB apart     (the image corners)
// Two ways of dropping a share p of the 64 lanes (a quad = 4 consecutive lanes, 8 quads per row):
//   quads: whole quads, in one contiguous run from the start of each row (ceil(n/2) quads of row 0, floor(n/2) of row 1,
//          n = round(16 p))
//   lanes: the first floor(4 p) lanes of EVERY quad, so that every quad stays live up to 75 %; what is left of round(64 p)
//          after that fills up quads from the start (at 90 %: 10 quads dropped whole, 6 with one live lane; 100 % = quads)
//   hipcc --offload-arch=gfx950 -O3 gather_dropped_quads.hip -o gather_dropped_quads && ./gather_dropped_quads
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cmath>
typedef float f2v __attribute__((ext_vector_type(2)));

constexpr unsigned WINDOW = 16384;  // bytes per workgroup

template <int BYTES>
__global__ __launch_bounds__(1024) void k(const float* __restrict__ buf, unsigned total_bytes, int iters, float slope,
                                          unsigned long long dropped, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)buf, 0, total_bytes, 0x00020000);
  const unsigned w = blockIdx.x * WINDOW;
  const int l = lane & 31, rj = lane >> 5;
  const int drow = (int)floorf((float)l * slope);
  const bool drop = (dropped >> lane) & 1ull;
  float acc = 0.f;
  int sel = 0;
  for (int it = 0; it < iters; ++it) {
    unsigned off;
    if (BYTES == 1) {  // 64 rows x 256 bytes; col + 31 <= 127 + 31 < 256
      const int r0 = (it * 3 + wave + sel) & 63, c0 = (it * 7 + wave * 5) & 127;
      off = w + (unsigned)(((r0 + rj + drow) & 63) * 256 + c0 + l);
    } else {  // 16 rows x 256 floats; col + 1 <= 63 + 31 + 1 < 256
      const int r0 = (it * 3 + wave + sel) & 15, c0 = (it * 7 + wave * 5) & 63;
      off = w + (unsigned)(((r0 + rj + drow) & 15) * 256 + c0 + l) * 4u;
    }
    off = drop ? 0x80000000u : off;  // >= total_bytes: dropped by the range check
    if (BYTES == 1) acc += (float)__builtin_amdgcn_raw_buffer_load_b8(r, off, 0, 0);
    if (BYTES == 8) { f2v v = __builtin_bit_cast(f2v, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0)); acc += v.x + v.y; }
    sel = (acc == 1234.5f) ? 1 : 0;
  }
  out[(size_t)blockIdx.x * 1024 + threadIdx.x] = acc;
}

static unsigned long long mask_quads(int pct) {
  const int n = (int)lround(16.0 * pct / 100.0), n0 = (n + 1) / 2, n1 = n / 2;
  unsigned long long m = 0;
  for (int q = 0; q < n0; ++q) m |= 0xFull << (4 * q);
  for (int q = 0; q < n1; ++q) m |= 0xFull << (32 + 4 * q);
  return m;
}
static unsigned long long mask_lanes(int pct) {
  const int total = (int)lround(64.0 * pct / 100.0), per = pct >= 100 ? 4 : (4 * pct) / 100;
  unsigned long long m = 0;
  for (int q = 0; q < 16; ++q) m |= ((1ull << per) - 1ull) << (4 * q);
  int left = total - 16 * per;
  for (int q = 0; q < 16 && left > 0; ++q) {  // fill up quads from the start, alternating rows as above
    const int qq = (q & 1) ? 8 + q / 2 : q / 2;
    for (int j = per; j < 4 && left > 0; ++j, --left) m |= 1ull << (4 * qq + j);
  }
  return m;
}

int main() {
  const int blocks = 512;
  const unsigned total_bytes = (unsigned)blocks * WINDOW;  // 8 MB < 2^31
  float *buf, *out;
  hipMalloc(&buf, total_bytes);
  hipMalloc(&out, (size_t)blocks * 1024 * 4);
  hipMemset(buf, 0, total_bytes);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  const int iters = 2048;
  const float slopes[] = {0.f, 0.2f, 0.34f};
  const int pcts[] = {0, 25, 50, 75, 90, 100};
  printf("cycles per wave-instruction per CU (2400 MHz, 256 CUs); columns: share of the 64 lanes sent out of range\n");
  printf("%-36s", "");
  for (int p : pcts) printf(" %6d%%", p);
  printf("\n");
  for (float slope : slopes)
    for (int bytes : {1, 8})
      for (int pattern = 0; pattern < 2; ++pattern) {
        printf("slope %.2f  %d B  %-18s", slope, bytes, pattern == 0 ? "whole quads" : "lanes in live quads");
        for (int p : pcts) {
          const unsigned long long m = pattern == 0 ? mask_quads(p) : mask_lanes(p);
          auto run = [&]() {
            if (bytes == 1) hipLaunchKernelGGL((k<1>), dim3(blocks), dim3(1024), 0, 0, buf, total_bytes, iters, slope, m, out);
            else hipLaunchKernelGGL((k<8>), dim3(blocks), dim3(1024), 0, 0, buf, total_bytes, iters, slope, m, out);
          };
          run();
          hipDeviceSynchronize();
          hipEventRecord(e0);
          for (int r = 0; r < 5; ++r) run();
          hipEventRecord(e1);
          hipEventSynchronize(e1);
          float ms;
          hipEventElapsedTime(&ms, e0, e1);
          const double us = ms * 1e3 / 5;
          const double winstr_per_cu = (double)blocks * 16 * iters / 256.0;
          printf(" %7.1f", us * 2400.0 / winstr_per_cu);
        }
        printf("\n");
      }
  if (hipDeviceSynchronize() != hipSuccess) { printf("FAILED\n"); return 1; }
  return 0;
}
