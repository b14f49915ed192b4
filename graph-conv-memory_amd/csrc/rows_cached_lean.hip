// The lean cached step (cfg2's timed kernel): k_step_rows_cached_img4b (rows_cached.hip) for the one case the benchmark
// runs - F = H1 = 32, H2 <= 32, tanh / tanh, at most four distinct forward hops, the row known on the host
// (0 <= cur_host < N <= 128) - with the path from launch to the last load issue cut down to what the computing wave needs.
//
// What img4b's computing wave waited for (its gfx950 ISA): three dependent scalar loads of a 192-byte kernarg segment
// (HopMask and CachedLayout by value), each behind an lgkmcnt wait, then ~60 scalar instructions that decode the hops,
// and only then the loads of the source rows; the activations were selected at run time.  Here
//   * the host resolves the step: row cur, the source rows cur - hop (ascending, compacted: the order img4b's mask walk
//     adds them in), the source masks the bookkeeping wave writes from;
//   * the first 13 dwords of the arguments are all the computing wave needs before its last load (obs, image, nodes, cH,
//     params, cur, the packed sources, N | H2 | self) - and this translation unit is compiled with
//     -amdgpu-kernarg-preload-count (Makefile), so that they arrive in SGPRs with the wave: no scalar load and no scalar
//     wait in front of the loads;
//   * the loads are issued in the order they are consumed (rows and obs, layer 1's weights and bias, layer 2's), so that
//     layer 1 starts on a counted vmcnt while layer 2's weights are still in flight;
//   * tanh is compile-time, and each half-wave's product chain is two independent packed accumulators of eight instead of
//     one of sixteen (re-associated: DESIGN §4).
// The second wave (the state's entries, the count, the record's live list / coefficients / header) is img4b's; the record
// is the same layout, so gcm_dense_rows_bptt_cached reads it unchanged.
#include "fused_common.h"
#include "gcm_common.h"
#include "rows_common.h"
#include "rows_lean.h"

namespace gcm_rows {

// src4: the source rows of row cur, ascending, one byte each, 0xff for an empty slot.  nhs: N | H2 << 8 | self << 16.
// m0, m1: the source rows as a mask (without the self loop); o_*: the record's float offsets (CachedLayout), rec = 0:
// the record is mx alone.
__global__ __launch_bounds__(128) void k_step_rows_cached_img4_lean(
    const float* __restrict__ obs, const float* __restrict__ image, float* __restrict__ nodes, float* __restrict__ cH,
    const float* __restrict__ params, int cur, unsigned src4, unsigned nhs,
    float* __restrict__ adj, int64_t* __restrict__ count, float* __restrict__ cA, float* __restrict__ cX,
    float* __restrict__ saved, uint32_t* __restrict__ flags, unsigned long long m0, unsigned long long m1,
    unsigned o_v, unsigned o_hdr, unsigned o_coef, unsigned o_live, int rec) {
  constexpr int F = 32, H1 = 32;
  __shared__ __attribute__((aligned(16))) float sv[128];
  const int lane = threadIdx.x & 63;
  const unsigned gb = blockIdx.x;
  const unsigned N = nhs & 0xffu;
  const int H2 = (int)((nhs >> 8) & 0xffu);
  const bool self = (nhs >> 16) & 1u;
  const unsigned rc = gb * N + (unsigned)cur;
  STAMP(0);
  if (threadIdx.x >= 64) {
    // ---- the bookkeeping wave: what follows from cur and the masks alone ----------------------------------------
    const float xo = obs[gb * F + (lane & 31)];
    if (lane < F) {
      nodes[rc * F + lane] = xo;
      cX[rc * F + lane] = xo;
    }
    float* arow = adj + (size_t)rc * N;
    const unsigned long long s0 = m0 | ((self && cur < 64) ? 1ull << cur : 0ull);
    const unsigned long long s1 = m1 | ((self && cur >= 64) ? 1ull << (cur - 64) : 0ull);
    if (lane < (int)N && ((s0 >> lane) & 1ull)) arow[lane] = 1.f;
    if (lane + 64 < (int)N && ((s1 >> lane) & 1ull)) arow[lane + 64] = 1.f;
    if (lane == 0) count[gb] = cur + 1;
    if (rec) {
      const unsigned long long l0 = m0 | (cur < 64 ? 1ull << cur : 0ull), l1 = m1 | (cur >= 64 ? 1ull << (cur - 64) : 0ull);
      int* live = reinterpret_cast<int*>(saved + o_live) + gb * N;
      float* coef = saved + o_coef + gb * N;
      const int j0 = lane, j1 = lane + 64;
      const bool in0 = (l0 >> lane) & 1ull, in1 = (l1 >> lane) & 1ull;
      const int pos0 = __popcll(l0 & ((1ull << lane) - 1ull));
      const int pos1 = __popcll(l0) + __popcll(l1 & ((1ull << lane) - 1ull));
      if (in0) { live[pos0] = j0; coef[pos0] = (j0 == cur && !self) ? 0.f : 1.f; }
      if (in1) { live[pos1] = j1; coef[pos1] = (j1 == cur && !self) ? 0.f : 1.f; }
      if (lane == 0) {
        int* hdr = reinterpret_cast<int*>(saved + o_hdr) + 4 * gb;
        const int L = __popcll(l0) + __popcll(l1);
        const int l_cur = cur < 64 ? __popcll(l0 & ((1ull << cur) - 1ull)) : __popcll(l0) + __popcll(l1 & ((1ull << (cur - 64)) - 1ull));
        hdr[0] = L; hdr[1] = l_cur; hdr[2] = cur; hdr[3] = 0;
      }
    }
    return;
  }
  // ---- the computing wave: every load from the preloaded arguments, in the order of use --------------------------
  const int fl = lane & 31, ol = lane < H2 ? lane : H2 - 1, kh = lane >> 5;
  float xa[4], ha[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {   // the source rows (an empty slot reads row 0 and adds nothing)
    const unsigned s = (src4 >> (8 * q)) & 0xffu;
    const unsigned rj = gb * N + (s == 0xffu ? 0u : s);
    xa[q] = nodes[rj * F + fl];
    ha[q] = cH[rj * H1 + fl];
  }
  const float xc = obs[gb * F + fl];
  asm volatile("" ::: "memory");
  const f32x2* i3 = reinterpret_cast<const f32x2*>(image + 2 * 4 * 64 * 64);   // image3 (k_cached_weight_image)
  f32x2 w1[16], w2[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) w1[k] = i3[k * 64 + lane];
  const float* b1 = params + 2 * H1 * F;
  const float bias1 = b1[fl];
  asm volatile("" ::: "memory");
#pragma unroll
  for (int k = 0; k < 16; ++k) w2[k] = i3[(16 + k) * 64 + lane];
  const float bias2 = b1[H1 + 2 * H2 * H1 + ol];
  STAMP(1);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool any = ((src4 >> (8 * q)) & 0xffu) != 0xffu;
    xa[q] = any ? xa[q] : 0.f;
    ha[q] = any ? ha[q] : 0.f;
  }
  // (the sums img4b's mask walk makes: sources ascending, (v0 + v1) + (v2 + v3))
  float agg1 = (xa[0] + xa[1]) + (xa[2] + xa[3]), agg2 = (ha[0] + ha[1]) + (ha[2] + ha[3]);
  agg1 = lane < F ? agg1 + (self ? xc : 0.f) : 0.f;
  if (lane < F) *reinterpret_cast<f32x2*>(sv + 2 * lane) = f32x2{agg1, xc};
  asm volatile("" ::: "memory");   // (lanes exchange through LDS; one wave: its LDS operations execute in order)
  STAMP(2);
  const float p1 = bias1 + lean_half_matvec(w1, sv, kh);   // (all 64 lanes: the halves meet across lanes 0 - 63)
  const float h1c = lane < H1 ? gcm_tanh(p1) : 0.f;
  STAMP(3);
  agg2 = lane < H1 ? agg2 + (self ? h1c : 0.f) : 0.f;
  if (lane < H1) *reinterpret_cast<f32x2*>(sv + 2 * lane) = f32x2{agg2, h1c};
  asm volatile("" ::: "memory");
  const float p2 = bias2 + lean_half_matvec(w2, sv, kh);
  const float v = gcm_tanh(p2);
  STAMP(4);
  if (lane < F) cA[rc * F + lane] = agg1;
  if (lane < H1) cH[rc * H1 + lane] = h1c;
  if (lane < H2) saved[gb * H2 + lane] = v;
  if (rec && lane < H1) {
    saved[o_v + gb * 2 * H1 + lane] = agg2;
    saved[o_v + gb * 2 * H1 + H1 + lane] = h1c;
  }
  STAMP(5);
  const bool nonfinite = __any(lane < H2 && !isfinite(v));
  if (nonfinite && lane == 0) atomicOr(flags, GCM_FLAG_NONFINITE);
}

// the host side: the step resolved from cur and the hop mask (gcm_dense_rows_step_cached_ws decides the case)
int launch_step_cached_lean(const float* obs, float* nodes, float* adj, int64_t* count, unsigned long long m0,
                            unsigned long long m1, int self, const float* params, const float* image, float* cH,
                            float* cA, float* cX, float* saved, const CachedLayout& lay, uint32_t* flags, int B, int N,
                            int H2, int cur, hipStream_t stream) {
  if (N > 128 || H2 <= 0 || H2 > 32 || cur < 0 || cur >= N || lay.total >= ((size_t)1 << 31)) return GCM_EUNSUPPORTED;
  unsigned src4 = 0xffffffffu;
  int n = 0;
  for (int j = 0; j < N; ++j) {
    const bool on = j < 64 ? ((m0 >> j) & 1ull) != 0 : ((m1 >> (j - 64)) & 1ull) != 0;
    if (!on) continue;
    if (n == 4) return GCM_EUNSUPPORTED;
    src4 &= ~(0xffu << (8 * n));
    src4 |= (unsigned)j << (8 * n);
    ++n;
  }
  const unsigned nhs = (unsigned)N | (unsigned)H2 << 8 | (self ? 1u << 16 : 0u);
  hipLaunchKernelGGL(k_step_rows_cached_img4_lean, dim3(B), dim3(128), 0, stream, obs, image, nodes, cH, params, cur,
                     src4, nhs, adj, count, cA, cX, saved, flags, m0, m1, (unsigned)lay.o_v, (unsigned)lay.o_hdr,
                     (unsigned)lay.o_coef, (unsigned)lay.o_live, lay.total ? 1 : 0);
  return gcm_launch_status();
}

const void* lean_step_kernel() { return (const void*)k_step_rows_cached_img4_lean; }

}  // namespace gcm_rows
