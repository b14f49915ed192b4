// What the lean cached step (rows_cached_lean.hip) and its multi-step form (rows_cached_run.hip) share: the half-wave
// product chain - ONE definition, so that both kernels make the same operations in the same order - and the lean
// kernel's host entry.
#pragma once
#include "gcm_common.h"
#include "rows_common.h"

namespace gcm_rows {

// a half-wave's sixteen k of a layer's two products (image3 pairs, sv = (agg, x)[k] pairs), two chains of eight
__device__ __forceinline__ float lean_half_matvec(const f32x2 (&w)[16], const float* sv, int kh) {
  f32x2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(sv + 32 * kh + 4 * j);
    acc0 = w[2 * j] * f32x2{u[0], u[1]} + acc0;
    acc1 = w[2 * j + 1] * f32x2{u[2], u[3]} + acc1;
  }
  const f32x2 acc = acc0 + acc1;
  return gcm_xor32_add(acc[0] + acc[1]);
}

// The same chain for a lane that makes BOTH K halves of its column itself (the multi-step kernel: a step per half-wave)
// and adds them in lean_half_matvec's order, half 0's sum + half 1's: lean_half_chain(.., 0) + lean_half_chain(.., 1).
// It repeats the loop above word for word - keep the two alike - instead of sharing a helper with it: with a shared
// helper the compiler swaps the operands of two packed adds in the lean kernel, whose code is to stay what it is.
__device__ __forceinline__ float lean_half_chain(const f32x2 (&w)[16], const float* sv, int kh) {
  f32x2 acc0 = {0.f, 0.f}, acc1 = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(sv + 32 * kh + 4 * j);
    acc0 = w[2 * j] * f32x2{u[0], u[1]} + acc0;
    acc1 = w[2 * j + 1] * f32x2{u[2], u[3]} + acc1;
  }
  const f32x2 acc = acc0 + acc1;
  return acc[0] + acc[1];
}

// Is this cached step the lean case - and if so, which step?  The ONE decision both gcm_dense_rows_step_cached_ws and
// the run entry (rows_cached_run.hip) take: a weight image in its interleaved form, no distance selector, neither
// GCM_STEP_ONE_WAVE nor GCM_STEP_NOT_LEAN, F = H1 = 32, 0 < H2 <= 32, tanh / tanh, the row known on the host
// (0 <= cur_host < N <= 128), at most four distinct hops 0 < h < 128.  (The caller has checked
// gcm_dense_rows_cached_supported_ws and the 32-bit offsets.)  hops: those hops ASCENDING; self: a hop of 0;
// m0, m1: the source rows cur_host - h >= 0 as a mask.
struct LeanCase {
  int hops[4], nh, self;
  unsigned long long m0, m1;
};
inline bool lean_step_case(const gcm_selector_desc* selectors, int n_selectors, const float* weight_image, int has_bias,
                           int act1, int act2, int N, int F, int H1, int H2, int cur_host, LeanCase& c) {
  if (!weight_image || !(has_bias & GCM_STEP_IMG_V4) || (has_bias & (GCM_STEP_ONE_WAVE | GCM_STEP_NOT_LEAN)) || F != 32 ||
      H1 != 32 || H2 <= 0 || H2 > 32 || act1 != GCM_ACT_TANH || act2 != GCM_ACT_TANH || cur_host < 0 || cur_host >= N ||
      N > 128)
    return false;
  c.nh = c.self = 0;
  c.m0 = c.m1 = 0ull;
  for (int i = 0; i < n_selectors; ++i) {
    const gcm_selector_desc& d = selectors[i];
    if (d.kind == GCM_SEL_DISTANCE) return false;
    for (int k = 0; k < d.n_hops; ++k) {
      const int h = d.hops[k];
      if (h == 0) c.self = 1;
      if (h <= 0 || h >= 128) continue;
      int at = 0;
      while (at < c.nh && c.hops[at] < h) ++at;
      if (at < c.nh && c.hops[at] == h) continue;
      if (c.nh == 4) return false;
      for (int j = c.nh; j > at; --j) c.hops[j] = c.hops[j - 1];
      c.hops[at] = h;
      ++c.nh;
    }
  }
  for (int a = 0; a < c.nh; ++a) {
    const int j = cur_host - c.hops[a];
    if (j < 0) continue;
    if (j < 64) c.m0 |= 1ull << j;
    else c.m1 |= 1ull << (j - 64);
  }
  return true;
}

// the lean kernel's host handle (what a captured launch's graph node carries as its function)
const void* lean_step_kernel();
int launch_step_cached_lean(const float* obs, float* nodes, float* adj, int64_t* count, unsigned long long m0,
                            unsigned long long m1, int self, const float* params, const float* image, float* cH,
                            float* cA, float* cX, float* saved, const CachedLayout& lay, uint32_t* flags, int B, int N,
                            int H2, int cur, hipStream_t stream);

}  // namespace gcm_rows
