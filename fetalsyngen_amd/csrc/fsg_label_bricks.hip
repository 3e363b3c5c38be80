// fsg_label_bricks.hip -- the brick table of a uint8 label volume and the registry the fused warp finds it in.
//
// Label volumes are piecewise constant: most 8x8x8 bricks of a segmentation hold ONE label (89.9 % of the phantom's at 256^3),
// and a subject's segmentation does not change from sample to sample.  The table says, per brick, that label -- or 255 for
// "mixed: gather" -- so that warp_lean_kernel<.., HAS_MAP> (fsg_warp_lean.hip) can send the label gathers of uniform bricks
// outside its descriptor's range.  Built once per subject (not a timed kernel); the warp takes it from the registry below by
// the label volume's address, so the plan layout carries nothing new.
#include "fsg_common.h"

#include <mutex>

namespace {

// One wave per brick: lane = (x, y) of the brick's 8 x 8 columns, 8 voxels along z each; voxels past an upper face do not count.
__global__ __launch_bounds__(256) void label_bricks_kernel(const uint8_t* __restrict__ labels, int n0, int n1, int n2, int b1,
                                                           int b2, int nb, uint8_t* __restrict__ map) {
  const int lane = threadIdx.x & 63;
  const int brick = blockIdx.x * 4 + (threadIdx.x >> 6);  // uniform per wave
  if (brick >= nb) return;
  const int bz = brick % b2, by = (brick / b2) % b1, bx = brick / (b2 * b1);
  const int x = bx * 8 + (lane >> 3), y = by * 8 + (lane & 7), z0 = bz * 8;
  const uint8_t first = labels[((size_t)(bx * 8) * n1 + by * 8) * n2 + z0];  // a brick's first corner is always inside
  bool same = true;
  if (x < n0 && y < n1) {
    const uint8_t* __restrict__ row = labels + ((size_t)x * n1 + y) * n2;
    const int kn = min(8, n2 - z0);
    for (int k = 0; k < kn; ++k) same = same && row[z0 + k] == first;
  }
  const bool uniform = __all(same);
  if (lane == 0) map[brick] = (uniform && first != 255) ? first : (uint8_t)255;
}

struct BrickEntry {
  const void* vol;
  const void* map;
  int n0, n1, n2;
};
constexpr int BRICKS_ENTRIES = 64;  // tables attached at a time; a volume beyond that is simply gathered
BrickEntry g_bricks[BRICKS_ENTRIES];
int g_bricks_count = 0;
int g_bricks_cap = FSG_LABEL_BRICKS_CAP;
std::mutex g_bricks_mutex;

long long bricks_of(int n0, int n1, int n2) {
  return (long long)((n0 + 7) / 8) * ((n1 + 7) / 8) * ((n2 + 7) / 8);
}

}  // namespace

const uint8_t* fsg_label_bricks_find(const void* labels_u8, int n0, int n1, int n2) {
  std::lock_guard<std::mutex> lock(g_bricks_mutex);
  if (g_bricks_count == 0 || bricks_of(n0, n1, n2) > g_bricks_cap) return nullptr;
  for (int i = 0; i < g_bricks_count; ++i) {
    const BrickEntry& e = g_bricks[i];
    if (e.vol == labels_u8) return (e.n0 == n0 && e.n1 == n1 && e.n2 == n2) ? (const uint8_t*)e.map : nullptr;
  }
  return nullptr;
}

extern "C" {

int fsg_label_bricks_u8(const uint8_t* labels_u8, int n0, int n1, int n2, uint8_t* map_out, void* stream) {
  if (!labels_u8 || !map_out || n0 <= 0 || n1 <= 0 || n2 <= 0) return FSG_E_BADARG;
  const long long nb = bricks_of(n0, n1, n2);
  if ((long long)n0 * n1 * n2 >= (1ll << 31) || nb >= (1ll << 31)) return FSG_E_TOOBIG;
  const int b1 = (n1 + 7) / 8, b2 = (n2 + 7) / 8;
  hipLaunchKernelGGL(label_bricks_kernel, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, fsg_stream(stream), labels_u8, n0, n1, n2,
                     b1, b2, (int)nb, map_out);
  FSG_RETURN_LAUNCH();
}

int fsg_label_bricks_attach(const void* labels_u8, int n0, int n1, int n2, const void* map) {
  if (!labels_u8 || !map || n0 <= 0 || n1 <= 0 || n2 <= 0) return FSG_E_BADARG;
  if ((uintptr_t)map & 15u) return FSG_E_ALIGN;
  std::lock_guard<std::mutex> lock(g_bricks_mutex);
  int at = g_bricks_count;
  for (int i = 0; i < g_bricks_count; ++i)
    if (g_bricks[i].vol == labels_u8) at = i;
  if (at == BRICKS_ENTRIES) return FSG_E_TOOBIG;
  g_bricks[at] = BrickEntry{labels_u8, map, n0, n1, n2};
  if (at == g_bricks_count) ++g_bricks_count;
  return 0;
}

int fsg_label_bricks_detach(const void* labels_u8) {
  std::lock_guard<std::mutex> lock(g_bricks_mutex);
  for (int i = 0; i < g_bricks_count; ++i)
    if (g_bricks[i].vol == labels_u8) {
      g_bricks[i] = g_bricks[--g_bricks_count];
      return 1;
    }
  return 0;
}

int fsg_label_bricks_count(void) {
  std::lock_guard<std::mutex> lock(g_bricks_mutex);
  return g_bricks_count;
}

int fsg_label_bricks_usable(int n0, int n1, int n2) {
  if (n0 <= 0 || n1 <= 0 || n2 <= 0) return 0;
  std::lock_guard<std::mutex> lock(g_bricks_mutex);
  return bricks_of(n0, n1, n2) <= g_bricks_cap ? 1 : 0;
}

int fsg_label_bricks_set_cap(int cap) {
  if (cap < 0 || cap > FSG_LABEL_BRICKS_CAP) return FSG_E_BADARG;
  std::lock_guard<std::mutex> lock(g_bricks_mutex);
  const int prev = g_bricks_cap;
  g_bricks_cap = cap == 0 ? FSG_LABEL_BRICKS_CAP : cap;
  return prev;
}

}  // extern "C"
