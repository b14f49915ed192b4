// LearnedEdge(deterministic=True) (edge_selectors/learned.py:78-111 with the `deterministic` branch
// taken): the hard sparsemax (util.Spardmax, util.py:29-42; sparsemax of Martins & Astudillo 2016 made
// binary with a straight-through estimator) over the candidate logits of every graph, and the
// adjacency-row write.  Same form as k_select_fwd / k_select_bwd of learned.hip: one wave per graph,
// four graphs per 256-thread block, lane l owns columns l, l+64, ..., the row kept in registers.
//
// The threshold tau (sum_j max(z_j - tau, 0) = 1) comes from Michelot's iteration instead of a sort:
// start with every live entry in the set, tau = (sum_set z - 1) / |set|, drop the entries with
// z <= tau, repeat until the set no longer shrinks.  tau only grows, so a dropped entry stays out and
// the loop ends after at most n passes with the exact support; a pass is one fused pair of wave
// reductions in a fixed (butterfly) order, so the result is bitwise reproducible.  Membership is a
// comparison of values: equal logits are all in or all out, whichever lane or column holds them.
#include "gcm_common.h"

namespace {

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// two sums at once: the shuffles of one hide behind the other's
__device__ __forceinline__ void wave_sum2(float& a, float& b) {
  for (int o = 32; o > 0; o >>= 1) {
    const float ta = __shfl_xor(a, o), tb = __shfl_xor(b, o);
    a += ta;
    b += tb;
  }
}

// C = columns per lane (N <= 64 * C)
template <int C>
__global__ __launch_bounds__(256) void k_sparsemax_fwd(const float* __restrict__ logits,
                                                       const int64_t* __restrict__ cur_idx,
                                                       float* __restrict__ adj,
                                                       float* __restrict__ soft, int B, int N) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  int64_t cur64 = cur_idx[b];
  const int cur = (int)(cur64 < 0 ? 0 : (cur64 > N - 1 ? N - 1 : cur64));
  float z[C];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = lane + 64 * c;
    z[c] = (j < cur) ? logits[(size_t)b * N + j] : -INFINITY;
    m = fmaxf(m, z[c]);
  }
  m = wave_max(m);
  // sparsemax is shift invariant: with the row maximum at 0 every z <= 0, so sum_set z - 1 <= -1 stays
  // accurate for large logits, tau <= -1/|set| < 0 and the maximum never leaves the set.  A dead
  // column (j >= cur) is -inf - m = -inf: never in the set.
  unsigned in = 0;                       // bit c: column lane + 64 c is in the set
#pragma unroll
  for (int c = 0; c < C; ++c) {
    z[c] -= m;
    if (lane + 64 * c < cur) in |= 1u << c;
  }
  float tau = 0.f;
  float prev = -1.f;                     // |set| of the previous pass (counts <= 1023 are exact in fp32)
  for (int pass = 0; pass < cur; ++pass) {   // at most cur - 1 passes drop something: the last tau stands
    float s = 0.f, k = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (in >> c & 1u) {
        s += z[c];
        k += 1.f;
      }
    wave_sum2(s, k);
    if (k == prev) break;                // nothing was dropped: tau is the threshold of this set
    prev = k;
    tau = (s - 1.f) / k;
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (!(z[c] > tau)) in &= ~(1u << c);
  }
  float* row = adj + ((size_t)b * N + cur) * N;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = lane + 64 * c;
    if (j >= N) break;
    const bool sel = in >> c & 1u;
    // z > tau with |tau| >= 1/1023: the difference is a normal, positive float, so the backward can
    // read the support back as soft > 0
    soft[(size_t)b * N + j] = sel ? z[c] - tau : 0.f;
    if (j < cur) {
      const float edge = sel ? 1.f : 0.f;                    // Spardmax forward, cutoff 0 (util.py:38-42)
      row[j] = (edge + row[j] > 0.f) ? 1.f : 0.f;            // learned.py:108-110
    }
  }
}

// sparsemax Jacobian on row cur of g_adj: g_z[j] = g_j - mean_{k in S} g_k for j in S, else 0
template <int C>
__global__ __launch_bounds__(256) void k_sparsemax_bwd(const float* __restrict__ g_adj,
                                                       const float* __restrict__ soft,
                                                       const int64_t* __restrict__ cur_idx,
                                                       float* __restrict__ g_logits, int B, int N) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (b >= B) return;
  int64_t cur64 = cur_idx[b];
  const int cur = (int)(cur64 < 0 ? 0 : (cur64 > N - 1 ? N - 1 : cur64));
  const float* grow = g_adj + ((size_t)b * N + cur) * N;
  float g[C];
  unsigned in = 0;
  float s = 0.f, k = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = lane + 64 * c;
    const bool sel = j < cur && soft[(size_t)b * N + j] > 0.f;
    g[c] = sel ? grow[j] : 0.f;
    if (sel) {
      in |= 1u << c;
      s += g[c];
      k += 1.f;
    }
  }
  wave_sum2(s, k);
  const float mean = k > 0.f ? s / k : 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int j = lane + 64 * c;
    if (j < N) g_logits[(size_t)b * N + j] = (in >> c & 1u) ? g[c] - mean : 0.f;
  }
}

constexpr int MAXC = 16;   // N <= 1024, as gcm_learned_select_*

// launch(grid, block, c): a kernel's <c> instantiation, c = the columns of 64 candidates a lane holds
template <typename Launch>
int sparsemax_launch(int B, int N, Launch launch) {
  const int cols = (N + 63) / 64;
  return gcm_pick(
      [&](auto c) {
        launch(dim3((B + 3) / 4), dim3(256), c);
        return gcm_launch_status();
      },
      OneOf<1, 2, 4, 8, MAXC>{cols <= 1 ? 1 : cols <= 2 ? 2 : cols <= 4 ? 4 : cols <= 8 ? 8 : MAXC});
}

}  // namespace

extern "C" int gcm_learned_sparsemax_fwd(const float* logits, const int64_t* cur_idx, float* adj,
                                         float* soft, int B, int N, gcm_stream_t stream) {
  GCM_REQUIRE(logits && cur_idx && adj && soft && B > 0 && N > 0);
  if (N > 64 * MAXC) return GCM_EUNSUPPORTED;
  return sparsemax_launch(B, N, [&](dim3 grid, dim3 block, auto c) {
    hipLaunchKernelGGL(k_sparsemax_fwd<c()>, grid, block, 0, (hipStream_t)stream, logits, cur_idx, adj, soft, B, N);
  });
}

extern "C" int gcm_learned_sparsemax_bwd(const float* g_adj, const float* soft,
                                         const int64_t* cur_idx, float* g_logits, int B, int N,
                                         gcm_stream_t stream) {
  GCM_REQUIRE(g_adj && soft && cur_idx && g_logits && B > 0 && N > 0);
  if (N > 64 * MAXC) return GCM_EUNSUPPORTED;
  return sparsemax_launch(B, N, [&](dim3 grid, dim3 block, auto c) {
    hipLaunchKernelGGL(k_sparsemax_bwd<c()>, grid, block, 0, (hipStream_t)stream, g_adj, soft, cur_idx, g_logits, B, N);
  });
}
