// What the time-parallel rollout kernels share (rollout_tp.hip; rollout_reset.hip: the same forward with per-graph
// episode resets): the hop list of the forward temporal selectors, the 32-graph row loads, the host's hop collection.
#pragma once
#include "fused_common.h"
#include "gcm_common.h"
#include "rows_common.h"

namespace gcm_rtp {

using gcm_fused::acc_row;
using gcm_fused::mma32;

struct Hops {
  int n;          // distinct hops >= 1, DESCENDING (sources in ascending node order)
  int h[16];
  int self;       // a hop of 0: self loop
};

// rows b0 .. b0 + 31 of a [*, B, W] tensor at step s (W = 4 * W4 floats): lane loads W4 / 2 float4 (32 rows x W4 = 16 W4
// float4 per wave instruction group); piece i of lane: e4 = lane + 64 i, row = e4 / W4, col4 = e4 % W4
template <int W4>
__device__ __forceinline__ void load_rows(const float* __restrict__ base, size_t row_stride, int b0, int B, int lane,
                                          float4 (&v)[W4 / 2]) {
#pragma unroll
  for (int i = 0; i < W4 / 2; ++i) {
    const int e4 = lane + 64 * i, r = e4 / W4, c4 = e4 % W4;
    const int b = b0 + r < B ? b0 + r : B - 1;   // (clamped: an unconditional load)
    v[i] = *reinterpret_cast<const float4*>(base + (size_t)b * row_stride + 4 * c4);
  }
}
__device__ __forceinline__ void add4(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

static inline int collect_hops(const gcm_selector_desc* selectors, int n_selectors, int N, int T, Hops* out) {
  Hops hp{};
  int mx = 0;
  for (int i = 0; i < n_selectors; ++i) {
    const gcm_selector_desc& d = selectors[i];
    if (d.kind != GCM_SEL_TEMPORAL || d.direction != GCM_DIR_FORWARD) return 0;
    for (int k = 0; k < d.n_hops; ++k) {
      const int h = d.hops[k];
      if (h < 0 || h > N - 1) continue;       // (temporal.py:74: never valid in a graph of N nodes)
      if (h == 0) { hp.self = 1; continue; }
      bool seen = false;
      for (int q = 0; q < hp.n; ++q) seen = seen || hp.h[q] == h;
      if (seen) continue;
      if (hp.n == 16) return 0;
      hp.h[hp.n++] = h;
      mx = h > mx ? h : mx;
    }
  }
  if (T > N && N <= 2 * mx) return 0;         // a live row would have lost a source to the overflow roll
  for (int a = 0; a < hp.n; ++a)              // descending
    for (int b = a + 1; b < hp.n; ++b)
      if (hp.h[b] > hp.h[a]) { const int t = hp.h[a]; hp.h[a] = hp.h[b]; hp.h[b] = t; }
  *out = hp;
  return 1;
}

}  // namespace gcm_rtp
