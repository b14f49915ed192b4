// Time-parallel DenseGCM rollout with per-graph episode resets: DenseGCM.rollout(obs[T,B,F], reset=[T,B]) from EMPTY
// graphs with forward temporal hops as the only selectors and observations that carry no gradient.
//
// reset[t, b] empties graph b BEFORE obs[t, b] is inserted.  Nothing of the time-parallel form of rollout_tp.hip is lost:
// node t of graph b is still observation t, the caches [B, Tc, .] are still indexed by the step.  What changes is which
// hops are valid: with age[t, b] = t - start[t, b], start[t, b] = the latest s <= t with reset[s, b] (else 0), the node
// of step t sits in row min(age, N - 1) of its graph and hop h reaches a source iff h <= min(age, N - 1) - per GRAPH
// where rollout_tp.hip decides per step.  So the kernels below are k_rollout_tp_l1 / _l2 with the validity of a source
// row decided per row of the 32-graph tile: every lane knows the graphs its pieces belong to, loads their start[t, .]
// once, and a source row that is not valid is read from step t instead (an unconditional load) and replaced by zeros.
//
//   k_episode_start         start [T, B] from reset [T, B]: one thread per graph walking t (loads coalesced over b)
//   k_rollout_tp_reset_l1   layer 1 of every (step, 32 graphs) tile into the caches; the final state per graph:
//                           t0_b = max(start[T-1, b], T - N), rows t - t0_b for t >= t0_b, count_b = T - t0_b (nodes
//                           and adj are ZERO on entry: rows at or beyond count_b stay zero)
//   k_rollout_tp_reset_l2   layer 2, beliefs, and the step records with a live list / header per graph
//                           (gcm_dense_rows_bptt_cached walks them per (step, graph)); raises GCM_FLAG_WRAPPED when some
//                           graph receives a node at age >= N (the overflow roll of gcm.py:263-271)
#include "rollout_tp_common.h"

namespace gcm_rtp {

// rows b0 .. b0 + 31 of a tensor addressed as base + step * step_stride + b * row_stride (W = 4 * W4 floats a row) at
// step t - h where the row's graph holds that node (h <= age), zeros elsewhere: the address of a row that is not
// valid is redirected to step t (in bounds, no branch) and its value dropped.  Pieces as in load_rows.
template <int W4>
__device__ __forceinline__ void load_rows_valid(const float* __restrict__ base, size_t step_stride, size_t row_stride,
                                                int t, int h, const int (&age)[W4 / 2], int b0, int B, int lane,
                                                float4 (&v)[W4 / 2]) {
#pragma unroll
  for (int i = 0; i < W4 / 2; ++i) {
    const int e4 = lane + 64 * i, r = e4 / W4, c4 = e4 % W4;
    const int b = b0 + r < B ? b0 + r : B - 1;
    const bool ok = h <= age[i];
    const int s = ok ? t - h : t;
    const float4 x = *reinterpret_cast<const float4*>(base + (size_t)s * step_stride + (size_t)b * row_stride + 4 * c4);
    v[i] = make_float4(ok ? x.x : 0.f, ok ? x.y : 0.f, ok ? x.z : 0.f, ok ? x.w : 0.f);
  }
}

__global__ __launch_bounds__(256) void k_episode_start(const uint8_t* __restrict__ reset, int32_t* __restrict__ start,
                                                       int T, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int s = 0;
  int t = 0;
  for (; t + 8 <= T; t += 8) {              // eight independent loads in flight
    uint8_t m[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = reset[(size_t)(t + k) * B + b];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      s = m[k] ? t + k : s;
      start[(size_t)(t + k) * B + b] = s;
    }
  }
  for (; t < T; ++t) {
    s = reset[(size_t)t * B + b] ? t : s;
    start[(size_t)t * B + b] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------
template <int FP, int HP>
__global__ __launch_bounds__(256) void k_rollout_tp_reset_l1(
    const float* __restrict__ obs, const int32_t* __restrict__ start, Hops hp, const float* __restrict__ params, int act1,
    float* __restrict__ cH, float* __restrict__ cA, float* __restrict__ cX, float* __restrict__ nodes_out,
    float* __restrict__ adj_out, int64_t* __restrict__ count_out, int B, int T, int N, int Tc, int n_tiles) {
  constexpr int F = FP, H1 = HP, F4 = FP / 4;
  constexpr int AS = 2 * FP + 1;          // A tile row stride (odd: conflict-free fragment reads)
  constexpr int WS = HP + 1;              // B operand [k][n] row stride
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  extern __shared__ float smem[];
  float* sW = smem;                                      // [2 FP][WS]: k < FP: W_rel1[n][k], else W_root1[n][k - FP]
  float* sA = sW + 2 * FP * WS + (size_t)wave * 32 * AS;   // this wave's [32][AS] tile: agg1 | x
  for (int e = tid; e < 2 * FP * HP; e += 256) {
    const int m = e / (FP * HP), rem = e - m * FP * HP, n = rem / FP, k = rem % FP;
    sW[(m * FP + k) * WS + n] = params[(size_t)m * H1 * F + (size_t)n * F + k];
  }
  float bias[HP / 32];
#pragma unroll
  for (int nt = 0; nt < HP / 32; ++nt) bias[nt] = params[2 * (size_t)H1 * F + nt * 32 + li];
  const int act_v = gcm_vgpr(act1);
  __syncthreads();
  const int nbt = (B + 31) / 32;
  const int t_floor = T > N ? T - N : 0;    // no graph's final state reaches further back
  const int32_t* start_last = start + (size_t)(T - 1) * B;
#pragma unroll 1
  for (int tile = blockIdx.x * 4 + wave; tile < n_tiles; tile += gridDim.x * 4) {
    const int t = tile / nbt, b0 = (tile - t * nbt) * 32;
    int age[F4 / 2], t0[F4 / 2];            // of the graph each piece belongs to
#pragma unroll
    for (int i = 0; i < F4 / 2; ++i) {
      const int r = (lane + 64 * i) / F4;
      const int b = b0 + r < B ? b0 + r : B - 1;
      age[i] = t - start[(size_t)t * B + b];
      const int sl = start_last[b];
      t0[i] = sl > t_floor ? sl : t_floor;  // the final state holds the nodes of steps t0 .. T - 1
    }
    float4 xv[F4 / 2], ag[F4 / 2];
    load_rows<F4>(obs + (size_t)t * B * F, F, b0, B, lane, xv);
#pragma unroll
    for (int i = 0; i < F4 / 2; ++i) ag[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = 0; q < hp.n; ++q) {        // hops descending: sources in ascending node order
      int h = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) h = q == i ? hp.h[i] : h;
      if (h > t) continue;                  // (uniform: valid in no graph, and t - h stays a step)
      float4 sv[F4 / 2];
      load_rows_valid<F4>(obs, (size_t)B * F, F, t, h, age, b0, B, lane, sv);
#pragma unroll
      for (int i = 0; i < F4 / 2; ++i) add4(ag[i], sv[i]);
    }
    if (hp.self) {
#pragma unroll
      for (int i = 0; i < F4 / 2; ++i) add4(ag[i], xv[i]);
    }
#pragma unroll
    for (int i = 0; i < F4 / 2; ++i) {
      const int e4 = lane + 64 * i, r = e4 / F4, c = (e4 % F4) * 4;
      float* a = sA + r * AS + c;
      a[0] = ag[i].x; a[1] = ag[i].y; a[2] = ag[i].z; a[3] = ag[i].w;
      a[FP] = xv[i].x; a[FP + 1] = xv[i].y; a[FP + 2] = xv[i].z; a[FP + 3] = xv[i].w;
      const int b = b0 + r;
      if (b < B) {
        const size_t rc = ((size_t)b * Tc + t) * F + c;
        *reinterpret_cast<float4*>(cA + rc) = ag[i];
        *reinterpret_cast<float4*>(cX + rc) = xv[i];
        if (t >= t0[i]) *reinterpret_cast<float4*>(nodes_out + ((size_t)b * N + (t - t0[i])) * F + c) = xv[i];
      }
    }
    if (li + b0 < B) {                      // the band row of the final adjacency, and the count behind the last step
      const int sl = start_last[b0 + li];
      const int t0g = sl > t_floor ? sl : t_floor;
      const int r_state = t - t0g;          // < N: t0g >= T - N
      if (r_state >= 0) {
        float* arow = adj_out + ((size_t)(b0 + li) * N + r_state) * N;
        for (int q = lh; q < hp.n; q += 2) {
          int h = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) h = q == i ? hp.h[i] : h;
          if (h <= r_state) arow[r_state - h] = 1.f;
        }
        if (hp.self && lh == 0) arow[r_state] = 1.f;
        if (t == T - 1 && lh == 0) count_out[b0 + li] = T - t0g;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int nt = 0; nt < HP / 32; ++nt) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      mma32(acc, sA, AS, 1, sW + nt * 32, WS, 1, 2 * FP, li, lh);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int b = b0 + acc_row(r, lh);
        if (b < B) cH[((size_t)b * Tc + t) * H1 + nt * 32 + li] = gcm_act_sel(acc[r] + bias[nt], act_v);
      }
    }
    __builtin_amdgcn_wave_barrier();        // the tile is rewritten by the next trip
  }
}

// ---------------------------------------------------------------------------------------------------------
template <int HP>
__global__ __launch_bounds__(256) void k_rollout_tp_reset_l2(
    const int32_t* __restrict__ start, Hops hp, const float* __restrict__ params, int F, int act2,
    const float* __restrict__ cH, float* __restrict__ mx_all, float* __restrict__ rec0, size_t rec_stride,
    gcm_rows::CachedLayout lay, int record, uint32_t* __restrict__ flags, int B, int T, int N, int Tc, int H2,
    int n_tiles) {
  constexpr int H1 = HP, H4 = HP / 4;
  constexpr int AS = 2 * HP + 1, WS = 65;   // H2 <= 64
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 31, lh = lane >> 5;
  extern __shared__ float smem[];
  float* sW = smem;                                      // [2 HP][WS]: k < HP: W_rel2[n][k], else W_root2[n][k - HP]
  float* sA = sW + 2 * HP * WS + (size_t)wave * 32 * AS;   // [32][AS]: agg2 | h1[t]
  const float* w2 = params + 2 * (size_t)H1 * F + H1;
  for (int e = tid; e < 2 * HP * 64; e += 256) {
    const int m = e / (HP * 64), rem = e - m * HP * 64, n = rem / HP, k = rem % HP;
    sW[(m * HP + k) * WS + n] = n < H2 ? w2[(size_t)m * H2 * H1 + (size_t)n * H1 + k] : 0.f;
  }
  const float* b2 = w2 + 2 * (size_t)H2 * H1;
  float bias[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) bias[nt] = nt * 32 + li < H2 ? b2[nt * 32 + li] : 0.f;
  const int act_v = gcm_vgpr(act2);
  __syncthreads();
  const int nbt = (B + 31) / 32;
  const int n_out = (H2 + 31) / 32;
  bool bad = false, wrapped = false;
#pragma unroll 1
  for (int tile = blockIdx.x * 4 + wave; tile < n_tiles; tile += gridDim.x * 4) {
    const int t = tile / nbt, b0 = (tile - t * nbt) * 32;
    int age[H4 / 2];                        // of the graph each piece belongs to
#pragma unroll
    for (int i = 0; i < H4 / 2; ++i) {
      const int r = (lane + 64 * i) / H4;
      const int b = b0 + r < B ? b0 + r : B - 1;
      age[i] = t - start[(size_t)t * B + b];
    }
    float4 hv[H4 / 2], ag[H4 / 2];
    load_rows<H4>(cH + (size_t)t * H1, (size_t)Tc * H1, b0, B, lane, hv);
#pragma unroll
    for (int i = 0; i < H4 / 2; ++i) ag[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q = 0; q < hp.n; ++q) {
      int h = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) h = q == i ? hp.h[i] : h;
      if (h > t) continue;                  // (uniform)
      float4 sv[H4 / 2];
      load_rows_valid<H4>(cH, H1, (size_t)Tc * H1, t, h, age, b0, B, lane, sv);
#pragma unroll
      for (int i = 0; i < H4 / 2; ++i) add4(ag[i], sv[i]);
    }
    if (hp.self) {
#pragma unroll
      for (int i = 0; i < H4 / 2; ++i) add4(ag[i], hv[i]);
    }
    float* rec = rec0 + (size_t)t * rec_stride;
#pragma unroll
    for (int i = 0; i < H4 / 2; ++i) {
      const int e4 = lane + 64 * i, r = e4 / H4, c = (e4 % H4) * 4;
      float* a = sA + r * AS + c;
      a[0] = ag[i].x; a[1] = ag[i].y; a[2] = ag[i].z; a[3] = ag[i].w;
      a[HP] = hv[i].x; a[HP + 1] = hv[i].y; a[HP + 2] = hv[i].z; a[HP + 3] = hv[i].w;
      const int b = b0 + r;
      if (record && b < B) {                // v = agg2 | h1[cur]
        float* v = rec + lay.o_v + (size_t)b * 2 * H1 + c;
        *reinterpret_cast<float4*>(v) = ag[i];
        *reinterpret_cast<float4*>(v + H1) = hv[i];
      }
    }
    if (b0 + li < B && lh == 0) {           // per graph: the live list (the selected rows ascending, row t behind them)
      const int b = b0 + li;
      const int ageg = t - start[(size_t)t * B + b];
      wrapped = wrapped || ageg >= N;
      if (record) {
        int* live = reinterpret_cast<int*>(rec + lay.o_live) + (size_t)b * Tc;
        float* coef = rec + lay.o_coef + (size_t)b * Tc;
        int l = 0;
        for (int q = 0; q < hp.n; ++q) {
          int h = 0;
#pragma unroll
          for (int i = 0; i < 16; ++i) h = q == i ? hp.h[i] : h;
          if (h > ageg || h > t) continue;
          live[l] = t - h;
          coef[l] = 1.f;
          ++l;
        }
        live[l] = t;
        coef[l] = hp.self ? 1.f : 0.f;
        int* hdr = reinterpret_cast<int*>(rec + lay.o_hdr) + 4 * b;
        hdr[0] = l + 1; hdr[1] = l; hdr[2] = ageg < N ? ageg : N - 1; hdr[3] = ageg >= N ? 1 : 0;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int nt = 0; nt < n_out; ++nt) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      mma32(acc, sA, AS, 1, sW + nt * 32, WS, 1, 2 * HP, li, lh);
      const int col = nt * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int b = b0 + acc_row(r, lh);
        const float v = gcm_act_sel(acc[r] + bias[nt & 1], act_v);
        if (b < B && col < H2) {
          mx_all[((size_t)t * B + b) * H2 + col] = v;
          rec[(size_t)b * H2 + col] = v;      // mx: the head of the record
          bad = bad || !isfinite(v);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  const uint32_t f = (__any(bad) ? GCM_FLAG_NONFINITE : 0u) | (__any(wrapped) ? GCM_FLAG_WRAPPED : 0u);
  if (f && lane == 0) atomicOr(flags, f);
}

}  // namespace gcm_rtp

extern "C" int gcm_episode_start(const uint8_t* reset, int32_t* start, int T, int B, gcm_stream_t stream) {
  GCM_REQUIRE(reset && start && T > 0 && B > 0);
  if (T > 65535) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(gcm_rtp::k_episode_start, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, reset, start, T,
                     B);
  return gcm_launch_status();
}

extern "C" int gcm_dense_rollout_tp_reset_fwd(const float* obs, const int32_t* start, const gcm_selector_desc* selectors,
                                              int n_selectors, const float* params, int has_bias, int act1, int act2,
                                              float* nodes, float* adj, int64_t* count, float* cache_h1,
                                              float* cache_agg1, float* cache_nodes, float* records, size_t rec_stride,
                                              int record, float* mx_all, uint32_t* flags, int T, int B, int N, int Tc,
                                              int F, int H1, int H2, gcm_stream_t stream) {
  GCM_REQUIRE(obs && start && params && nodes && adj && count && cache_h1 && cache_agg1 && cache_nodes && records &&
              mx_all && flags && B > 0 && Tc >= T && (selectors || n_selectors == 0));
  if (!gcm_dense_rollout_tp_supported(selectors, n_selectors, has_bias, T, N, F, H1, H2)) return GCM_EUNSUPPORTED;
  if (T > 65535 || (size_t)B * Tc * 64 >= ((size_t)1 << 40)) return GCM_EUNSUPPORTED;
  gcm_rtp::Hops hp;
  gcm_rtp::collect_hops(selectors, n_selectors, N, T, &hp);
  const gcm_rows::CachedLayout lay = gcm_rows::make_cached_layout(B, Tc, H1, H2);
  GCM_REQUIRE(rec_stride >= (record ? lay.total : gcm_rows::pad64((size_t)B * H2)));
  const int nbt = (B + 31) / 32;
  const long tiles_l = (long)T * nbt;
  if (tiles_l > 2147483647L) return GCM_EUNSUPPORTED;
  const int n_tiles = (int)tiles_l;
  const int cap = 2 * gcm_cu_count();
  const int grid = (n_tiles + 3) / 4 < cap ? (n_tiles + 3) / 4 : cap;
  hipStream_t s = (hipStream_t)stream;
  const OneOf<32, 64> h1_{H1};
  const int rc = gcm_pick(
      [&](auto a, auto b) {
        auto k1 = gcm_rtp::k_rollout_tp_reset_l1<a(), b()>;
        const size_t lds1 = sizeof(float) * ((size_t)2 * a() * (b() + 1) + (size_t)4 * 32 * (2 * a() + 1));
        gcm_allow_dynamic_lds((const void*)k1, lds1);
        hipLaunchKernelGGL(k1, dim3(grid), dim3(256), lds1, s, obs, start, hp, params, act1, cache_h1, cache_agg1,
                           cache_nodes, nodes, adj, count, B, T, N, Tc, n_tiles);
        return gcm_launch_status();
      },
      OneOf<32, 64>{F}, h1_);
  if (rc) return rc;
  return gcm_pick(
      [&](auto b) {
        auto k2 = gcm_rtp::k_rollout_tp_reset_l2<b()>;
        const size_t lds2 = sizeof(float) * ((size_t)2 * b() * 65 + (size_t)4 * 32 * (2 * b() + 1));
        gcm_allow_dynamic_lds((const void*)k2, lds2);
        hipLaunchKernelGGL(k2, dim3(grid), dim3(256), lds2, s, start, hp, params, F, act2, cache_h1, mx_all, records,
                           rec_stride, lay, record, flags, B, T, N, Tc, H2, n_tiles);
        return gcm_launch_status();
      },
      h1_);
}
