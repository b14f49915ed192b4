// What the head of a rollout writes, element by element: the packed parameter vector out of its source tensors and the
// cached step's weight image (gcm_dense_rows_cached_weight_image: [4][64][64] floats per layout, m = W_rel1, W_root1,
// W_rel2, W_root2, value W_m[lane][k] or 0 outside the matrix) in its three layouts.  One place for k_head_fused
// (head_fused.hip), which makes them as a launch, and for the merged step kernel's fresh-state form
// (rows_cached_run.hip), which makes them beside its steps and fills its LDS copy of the third layout from the same
// sources: the two cannot drift.
#pragma once
#include <cstddef>

namespace gcm_rows {

constexpr int HEAD_MAX_SRCS = 16;

struct HeadSrcs {
  const float* p[HEAD_MAX_SRCS];
  unsigned off[HEAD_MAX_SRCS + 1];   // off[i]: the first float of source i in `packed`; off[n] = the total (repeated to the end)
};

const void* head_fused_kernel();   // k_head_fused (head_fused.hip): what a captured head launch's node must run

// (host) n source tensors as kernel arguments; false: invalid (a null source with a length, 2^31 floats or more, none)
inline bool head_make_srcs(const float* const* srcs_host, const size_t* lens_host, int n, HeadSrcs& hs, size_t& total) {
  hs = HeadSrcs{};
  total = 0;
  if (!srcs_host || !lens_host || n <= 0 || n > HEAD_MAX_SRCS) return false;
  for (int i = 0; i < n; ++i) {
    if (!srcs_host[i] && lens_host[i] != 0) return false;
    hs.p[i] = srcs_host[i];
    hs.off[i] = (unsigned)total;
    total += lens_host[i];
    if (total >= ((size_t)1 << 31)) return false;
  }
  for (int i = n; i <= HEAD_MAX_SRCS; ++i) hs.off[i] = (unsigned)total;
  return total > 0;
}

// float e < hs.off[HEAD_MAX_SRCS] of the packed vector: from the last source that starts at or before it (empty
// sources share their successor's start)
__device__ inline float head_packed_value(const HeadSrcs& hs, unsigned e) {
  const float* src = hs.p[0];
  unsigned base = 0;
#pragma unroll
  for (int i = 1; i < HEAD_MAX_SRCS; ++i) {
    const bool in = e >= hs.off[i] && hs.off[i] < hs.off[HEAD_MAX_SRCS];
    src = in ? hs.p[i] : src;
    base = in ? hs.off[i] : base;
  }
  return src[e - base];
}

constexpr int IMG_LAYOUT_FLOATS = 4 * 64 * 64;

// element e of [4][64][64] is (m, k, lane); layout 1 holds it at e itself
// layout 2: [layer][k][lane][rel | root]
__host__ __device__ inline int image2_index(int m, int k, int lane) {
  return IMG_LAYOUT_FLOATS + ((((m >> 1) * 64 + k) * 64 + lane) << 1) + (m & 1);
}
// layout 3 (lane, k < 32 only): [layer][k % 16][(k / 16) * 32 + lane][rel | root]
__host__ __device__ inline int image3_index(int m, int k, int lane) {
  return 2 * IMG_LAYOUT_FLOATS + ((((m >> 1) * 16 + (k & 15)) * 64 + (k >> 4) * 32 + lane) << 1) + (m & 1);
}
// the run kernel's LDS copy of layout 3, [layer][k % 16][lane][k / 16][rel | root]: pair e of layout 3 (its float
// index / 2) sits at pair image3_lds_pair(e)
__host__ __device__ inline int image3_lds_pair(int e) { return ((e >> 6) * 32 + (e & 31)) * 2 + ((e >> 5) & 1); }
__host__ __device__ inline int image3_lds_index(int m, int k, int lane) {
  return (image3_lds_pair((image3_index(m, k, lane) - 2 * IMG_LAYOUT_FLOATS) >> 1) << 1) + (m & 1);
}
// the value of image element (m, k, lane): the six GNN tensors lead the sources (W_rel1, W_root1, b1, W_rel2, W_root2, b2)
__device__ inline float head_image_value(const HeadSrcs& hs, int m, int k, int lane, int F, int H1, int H2) {
  float v = 0.f;
  if (m < 2) { if (lane < H1 && k < F) v = (m == 0 ? hs.p[0] : hs.p[1])[(size_t)lane * F + k]; }
  else { if (lane < H2 && k < H1) v = (m == 2 ? hs.p[3] : hs.p[4])[(size_t)lane * H1 + k]; }
  return v;
}
// ... and its stores into the three layouts
__device__ inline void head_image_store(float* image, int e, float v) {
  const int m = e >> 12, k = (e >> 6) & 63, lane = e & 63;
  image[e] = v;
  image[image2_index(m, k, lane)] = v;
  if (lane < 32 && k < 32) image[image3_index(m, k, lane)] = v;
}

}  // namespace gcm_rows
