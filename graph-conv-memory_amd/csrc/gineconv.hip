// GINEConv / DenseGINEConv (PyG's GINEConv and a dense twin) and the RelativeEdgeAttr transform on gfx950.  The
// layer's `nn` is an arbitrary module and stays in torch; what is here is
//
//   e_k     = W_e a_k + b_e  (the layer's `lin`; a_k [D] the edge's features), or a_k itself without it (D == F)
//   sparse:  h_i   = (1 + eps) x_i + sum over the edges k = (j -> i) of relu(x_j + e_k)
//   dense :  h_bi  = s x_bi + sum over j with adj_bij != 0 of adj_bij relu(x_bj + e_bij),  s = add_loop ? 1 + eps : 0
//
// The ReLU is per edge AND per channel, between the gather and the sum: there is no contraction for the matrix cores
// and no library GEMM covers it.  The point of the kernels is that neither e [E,F] nor the messages [E,F] ever reach
// memory: an edge costs its D features, not 3 F floats, and the backward recomputes x_j + W_e a_k + b_e and its sign.
//
// Lanes and channels, as resgatedconv.hip.  A group of G lanes owns a row; lane gl of the group holds channel gl (and
// gl + 64 when F > 64).  G is the power of two >= F from 8 to 64.  A lane keeps ITS channels' rows of W_e (D <= 32
// registers per channel; the template's DB is 4 or 32, the loops are unrolled over it) and b_e.  The D features of an
// edge are one address across the group: a broadcast read.  eps is read from its device pointer.
//
// sparse: k_gine_csr_fwd  a group per destination walks its CSR row.
//         k_gine_csr_dcol a group per source walks its CSC column: g_x[j] = (1 + eps) g_h[j] + sum delta_k,
//                         delta_k = g_h[sink_k] * [x_j + e_k > 0].  (One sweep, gine_csr_sweep, behind both.)
//         k_gine_csr_drow a group per destination again: g_a_k = W_e^T delta_k (a group sum per feature; delta_k itself
//                         without `lin`), and the lane's own sums of delta_k a_k^T and delta_k.  At most GINE_PARTS
//                         workgroups, each over a strided set of rows; a workgroup adds its groups up through LDS in
//                         slot order and writes one partial [F, D + 1] into the workspace; k_gine_sum_parts adds the
//                         partials in index order.  edge_attr is reached through csr_perm / the CSC's permutation: it
//                         is never copied into another order.
// dense:  the bit image of the pattern (attn_bits.h; set: adj != 0, the diagonal an ordinary entry) is built once in the
//         forward.  Neighbours come in tiles of 32 = one word of the image; a workgroup whose rows have no bit in a
//         word skips the tile (one __syncthreads_or); otherwise x of the 32 neighbours is staged in LDS,
//         [neighbour][channel], channel fastest (resgatedconv.hip's layout: conflict-free for G >= 32 under
//         ds_read_b32's 32-bank rule).  adj and edge_attr are read for set bits only - every entry when g_adj is wanted.
//         k_gine_dense_fwd / _drow by row block, _dcol by neighbour block over the transposed image (g_h of 32 rows
//         staged).  Neither sweep sums across workgroups; the parameter sums go per workgroup into the workspace.
// g_eps = sum <g_h, x>: fixed_sum.h's fp64 fixed-order dot, the one GINConv uses.
// Nothing accumulates with atomics: every sum runs in a fixed order.  F <= 128, D <= GCM_GINE_MAX_EDGE_DIM; any N.
#include "attn_bits.h"
#include "fixed_sum.h"

namespace {

constexpr int GINE_RPG = 4;      // rows (dense) of a lane group
constexpr int GINE_PARTS = 512;  // workgroups of the sparse row sweep of the backward, at most

__device__ __forceinline__ unsigned gine_valid_word(int w, int N) {
  const int n = N - w * 32;
  return n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : (1u << n) - 1u);
}

// What a lane keeps of `lin` for its NCH channels: DB > 0: rows of W_e (zero beyond D and F) and b_e; DB == 0: no lin.
template <int G, int NCH, int DB>
struct Lin {
  float w[NCH][DB > 0 ? DB : 1], b[NCH];
  int D;

  __device__ __forceinline__ void load(const float* __restrict__ w_e, const float* __restrict__ b_e, int gl, int F,
                                       int D_) {
    D = D_;
    if (DB == 0) return;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      b[ch] = c < F ? b_e[c] : 0.f;
#pragma unroll
      for (int d = 0; d < DB; ++d) w[ch][d] = (c < F && d < D) ? w_e[(size_t)c * D + d] : 0.f;
    }
  }
};

// the features of one edge, as every lane of the group holds them (DB > 0; a broadcast read per feature)
template <int DB>
struct Attr {
  float v[DB > 0 ? DB : 1];
  __device__ __forceinline__ void load(const float* __restrict__ a, int D) {
#pragma unroll
    for (int d = 0; d < DB; ++d) v[d] = d < D ? a[d] : 0.f;
  }
};

// e_k[c] for the lane's channel ch (c < F is the caller's to check in the no-lin form, where a [F] is read per lane)
template <int G, int NCH, int DB>
__device__ __forceinline__ float gine_e(const Lin<G, NCH, DB>& L, const Attr<DB>& A, const float* __restrict__ a,
                                        int ch, int c, int F) {
  if (DB == 0) return c < F ? a[c] : 0.f;
  float e = L.b[ch];
#pragma unroll
  for (int d = 0; d < DB; ++d) e = fmaf(L.w[ch][d], A.v[d], e);
  return e;
}

// ---------------------------------------------------------------------------
// sparse
// ---------------------------------------------------------------------------
// FWD: ptr / idx = the destination CSR, src = x, out = h.  !FWD: ptr / idx = the CSC by source (idx = sinks), src =
// g_h, out = g_x.  perm: the position of entry p in edge_attr's order (NULL: p itself).
template <int G, int NCH, int DB, bool FWD>
__device__ __forceinline__ void gine_csr_sweep(const float* __restrict__ x, const float* __restrict__ src,
                                               const float* __restrict__ ea, const float* __restrict__ w_e,
                                               const float* __restrict__ b_e, const float* __restrict__ eps,
                                               const int64_t* __restrict__ ptr, const int64_t* __restrict__ idx,
                                               const int64_t* __restrict__ perm, float* __restrict__ out, int64_t M,
                                               int F, int D) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (i >= M) return;
  const int gl = threadIdx.x % G;
  Lin<G, NCH, DB> L;
  L.load(w_e, b_e, gl, F, D);
  float xi[NCH], acc[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + ch * G;
    xi[ch] = c < F ? x[(size_t)i * F + c] : 0.f;
    acc[ch] = 0.f;
  }
  if (ptr) {
    const int64_t p1 = ptr[i + 1];
    for (int64_t p = ptr[i]; p < p1; ++p) {
      const int64_t o = idx[p];
      const int64_t k = perm ? perm[p] : p;
      const float* a = ea + (size_t)k * D;
      Attr<DB> A;
      A.load(a, D);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c = gl + ch * G;
        if (c >= F) continue;
        const float e = gine_e(L, A, a, ch, c, F);
        if (FWD) {
          const float pre = x[(size_t)o * F + c] + e;
          acc[ch] += pre > 0.f ? pre : 0.f;
        } else {
          const float pre = xi[ch] + e;
          acc[ch] += pre > 0.f ? src[(size_t)o * F + c] : 0.f;
        }
      }
    }
  }
  const float s = 1.f + eps[0];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + ch * G;
    if (c < F) out[(size_t)i * F + c] = fmaf(s, FWD ? xi[ch] : src[(size_t)i * F + c], acc[ch]);
  }
}

template <int G, int NCH, int DB>
__global__ __launch_bounds__(256) void k_gine_csr_fwd(const float* x, const float* ea, const float* w_e,
                                                      const float* b_e, const float* eps, const int64_t* row_ptr,
                                                      const int64_t* col, const int64_t* perm, float* h, int64_t M,
                                                      int F, int D) {
  gine_csr_sweep<G, NCH, DB, true>(x, nullptr, ea, w_e, b_e, eps, row_ptr, col, perm, h, M, F, D);
}

template <int G, int NCH, int DB>
__global__ __launch_bounds__(256) void k_gine_csr_dcol(const float* x, const float* g_h, const float* ea,
                                                       const float* w_e, const float* b_e, const float* eps,
                                                       const int64_t* col_ptr, const int64_t* rows,
                                                       const int64_t* perm, float* g_x, int64_t M, int F, int D) {
  gine_csr_sweep<G, NCH, DB, false>(x, g_h, ea, w_e, b_e, eps, col_ptr, rows, perm, g_x, M, F, D);
}

// the workgroup's sums of the per-group values v (one per lane) over its slots, in slot order -> slot 0's lanes
template <int G>
__device__ __forceinline__ float gine_slot_sum(float v, float* red) {
  constexpr int S = 256 / G;
  __syncthreads();  // the previous round is read
  red[threadIdx.x] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < G)
    for (int s = 0; s < S; ++s) t += red[s * G + threadIdx.x];
  return t;
}

// the lane's sums gw [NCH][DB], gb [NCH] -> part[blk][c * (D + 1) + d], d == D: the bias
template <int G, int NCH, int DB>
__device__ __forceinline__ void gine_write_part(const float (&gw)[NCH][DB > 0 ? DB : 1], const float (&gb)[NCH],
                                                float* __restrict__ part, float* red, int blk, int F, int D) {
  float* mine = part + (size_t)blk * F * (D + 1);
  const int gl = threadIdx.x % G;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + ch * G;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      if (d < D) {  // uniform
        const float t = gine_slot_sum<G>(gw[ch][d], red);
        if (threadIdx.x < G && c < F) mine[c * (D + 1) + d] = t;
      }
    }
    const float t = gine_slot_sum<G>(gb[ch], red);
    if (threadIdx.x < G && c < F) mine[c * (D + 1) + D] = t;
  }
}

template <int G, int NCH, int DB>
__global__ __launch_bounds__(256) void k_gine_csr_drow(const float* __restrict__ x, const float* __restrict__ g_h,
                                                       const float* __restrict__ ea, const float* __restrict__ w_e,
                                                       const float* __restrict__ b_e,
                                                       const int64_t* __restrict__ row_ptr,
                                                       const int64_t* __restrict__ col,
                                                       const int64_t* __restrict__ perm, float* __restrict__ g_ea,
                                                       float* __restrict__ part, int64_t M, int F, int D) {
  constexpr int S = 256 / G;
  __shared__ float red[256];
  const int slot = threadIdx.x / G, gl = threadIdx.x % G;
  Lin<G, NCH, DB> L;
  L.load(w_e, b_e, gl, F, D);
  float gw[NCH][DB > 0 ? DB : 1], gb[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    gb[ch] = 0.f;
#pragma unroll
    for (int d = 0; d < (DB > 0 ? DB : 1); ++d) gw[ch][d] = 0.f;
  }
  for (int64_t i = (int64_t)blockIdx.x * S + slot; i < M; i += (int64_t)gridDim.x * S) {
    float go[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      go[ch] = c < F ? g_h[(size_t)i * F + c] : 0.f;
    }
    const int64_t p1 = row_ptr[i + 1];
    for (int64_t p = row_ptr[i]; p < p1; ++p) {
      const int64_t j = col[p];
      const int64_t k = perm ? perm[p] : p;
      const float* a = ea + (size_t)k * D;
      Attr<DB> A;
      A.load(a, D);
      float delta[NCH];
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c = gl + ch * G;
        delta[ch] = 0.f;
        if (c >= F) continue;
        const float pre = x[(size_t)j * F + c] + gine_e(L, A, a, ch, c, F);
        delta[ch] = pre > 0.f ? go[ch] : 0.f;
        if (DB == 0 && g_ea) g_ea[(size_t)k * D + c] = delta[ch];
      }
      if (DB > 0) {
#pragma unroll
        for (int d = 0; d < DB; ++d) {
          float t = 0.f;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            t = fmaf(L.w[ch][d], delta[ch], t);
            gw[ch][d] = fmaf(delta[ch], A.v[d], gw[ch][d]);
          }
          if (g_ea && d < D) {  // uniform
            t = group_sum<G>(t);
            if (gl == 0) g_ea[(size_t)k * D + d] = t;
          }
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) gb[ch] += delta[ch];
      }
    }
  }
  if (DB > 0 && part) gine_write_part<G, NCH, DB>(gw, gb, part, red, blockIdx.x, F, D);
}

// out: g_w_e[c * D + d] and g_b_e[c] = the sum over the n partials of part[p][c * (D + 1) + d] in index order.  A
// workgroup takes 16 elements; 16 slices of the partials are summed side by side and then added up in slice order.
__global__ __launch_bounds__(256) void k_gine_sum_parts(const float* __restrict__ part, int n, float* __restrict__ g_w,
                                                        float* __restrict__ g_b, int F, int D) {
  __shared__ float red[256];
  const int L = F * (D + 1);
  const int el = threadIdx.x % 16, sl = threadIdx.x / 16;
  const int e = blockIdx.x * 16 + el;
  const int per = (n + 15) / 16;
  float t = 0.f;
  if (e < L)
    for (int p = sl * per; p < min(n, (sl + 1) * per); ++p) t += part[(size_t)p * L + e];
  red[threadIdx.x] = t;
  __syncthreads();
  if (sl != 0 || e >= L) return;
  t = 0.f;
  for (int s = 0; s < 16; ++s) t += red[s * 16 + el];
  const int c = e / (D + 1), d = e - c * (D + 1);
  if (d < D) {
    if (g_w) g_w[c * D + d] = t;
  } else if (g_b) {
    g_b[c] = t;
  }
}

// ---------------------------------------------------------------------------
// dense
// ---------------------------------------------------------------------------
// stage columns [0, F) of the 32 rows from `first` of src [.., F] as [row][CP]
template <int CP>
__device__ __forceinline__ void gine_stage(float* __restrict__ s0, const float* __restrict__ src, size_t rb, int first,
                                           int N, int F) {
  for (int e = threadIdx.x; e < GT * CP; e += 256) {
    const int t = e / CP, c = e - t * CP;
    const int n = first + t;
    s0[e] = (n < N && c < F) ? src[(rb + n) * F + c] : 0.f;
  }
}

template <int G, int NCH, int DB>
__global__ __launch_bounds__(256) void k_gine_dense_fwd(const unsigned* __restrict__ bits,
                                                        const float* __restrict__ adj, const float* __restrict__ x,
                                                        const float* __restrict__ ea, const float* __restrict__ w_e,
                                                        const float* __restrict__ b_e, const float* __restrict__ eps,
                                                        float* __restrict__ h, int N, int F, int D, int add_loop) {
  constexpr int CP = G * NCH, S = 256 / G;
  __shared__ float sX[GT * CP];  // [j][c]
  const int b = blockIdx.y, i0 = blockIdx.x * (S * GINE_RPG);
  const int slot = threadIdx.x / G, gl = threadIdx.x % G;
  const int W = (N + 31) / 32;
  const size_t rb = (size_t)b * N;
  Lin<G, NCH, DB> L;
  L.load(w_e, b_e, gl, F, D);
  float acc[GINE_RPG][NCH];
#pragma unroll
  for (int r = 0; r < GINE_RPG; ++r)
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) acc[r][ch] = 0.f;

  for (int w = 0; w < W; ++w) {
    unsigned word[GINE_RPG], any = 0u;
#pragma unroll
    for (int r = 0; r < GINE_RPG; ++r) {
      const int i = i0 + r * S + slot;
      word[r] = i < N ? bits[(rb + i) * W + w] : 0u;
      any |= word[r];
    }
    if (!__syncthreads_or(any != 0u)) continue;  // also: the previous tile is consumed
    gine_stage<CP>(sX, x, rb, w * 32, N, F);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GINE_RPG; ++r) {
      const int i = i0 + r * S + slot;
      const size_t abase = (rb + i) * N + w * 32;
      unsigned m = word[r];
      while (m) {
        const int jj = __ffs(m) - 1;
        m &= m - 1u;
        const float av = adj[abase + jj];
        const float* a = ea + (abase + jj) * D;
        Attr<DB> A;
        A.load(a, D);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int c = gl + ch * G;
          const float pre = sX[jj * CP + c] + gine_e(L, A, a, ch, c, F);
          acc[r][ch] = fmaf(av, pre > 0.f ? pre : 0.f, acc[r][ch]);
        }
      }
    }
  }
  const float s = add_loop ? 1.f + eps[0] : 0.f;
#pragma unroll
  for (int r = 0; r < GINE_RPG; ++r) {
    const int i = i0 + r * S + slot;
    if (i >= N) continue;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      if (c >= F) continue;
      float v = acc[r][ch];
      if (add_loop) v = fmaf(s, x[(rb + i) * F + c], v);
      h[(rb + i) * F + c] = v;
    }
  }
}

// by row block: g_adj (every entry, when asked for), g_edge_attr at the visited entries, the parameter partials
template <int G, int NCH, int DB>
__global__ __launch_bounds__(256) void k_gine_dense_drow(const unsigned* __restrict__ bits,
                                                         const float* __restrict__ adj, const float* __restrict__ x,
                                                         const float* __restrict__ g_h, const float* __restrict__ ea,
                                                         const float* __restrict__ w_e, const float* __restrict__ b_e,
                                                         float* __restrict__ g_adj, float* __restrict__ g_ea,
                                                         float* __restrict__ part, int N, int F, int D) {
  constexpr int CP = G * NCH, S = 256 / G;
  __shared__ float sX[GT * CP];
  __shared__ float red[256];
  const int b = blockIdx.y, i0 = blockIdx.x * (S * GINE_RPG);
  const int slot = threadIdx.x / G, gl = threadIdx.x % G;
  const int W = (N + 31) / 32;
  const size_t rb = (size_t)b * N;
  Lin<G, NCH, DB> L;
  L.load(w_e, b_e, gl, F, D);
  float go[GINE_RPG][NCH], gw[NCH][DB > 0 ? DB : 1], gb[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + ch * G;
    gb[ch] = 0.f;
#pragma unroll
    for (int d = 0; d < (DB > 0 ? DB : 1); ++d) gw[ch][d] = 0.f;
#pragma unroll
    for (int r = 0; r < GINE_RPG; ++r) {
      const int i = i0 + r * S + slot;
      go[r][ch] = (i < N && c < F) ? g_h[(rb + i) * F + c] : 0.f;
    }
  }

  for (int w = 0; w < W; ++w) {
    unsigned word[GINE_RPG], any = 0u;
#pragma unroll
    for (int r = 0; r < GINE_RPG; ++r) {
      const int i = i0 + r * S + slot;
      word[r] = i >= N ? 0u : (g_adj ? gine_valid_word(w, N) : bits[(rb + i) * W + w]);
      any |= word[r];
    }
    if (!__syncthreads_or(any != 0u)) continue;
    gine_stage<CP>(sX, x, rb, w * 32, N, F);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GINE_RPG; ++r) {
      const int i = i0 + r * S + slot;
      const size_t abase = (rb + i) * N + w * 32;
      unsigned m = word[r];
      while (m) {
        const int jj = __ffs(m) - 1;
        m &= m - 1u;
        const float av = adj[abase + jj];
        const float* a = ea + (abase + jj) * D;
        float* ga = g_ea ? g_ea + (abase + jj) * D : nullptr;
        Attr<DB> A;
        A.load(a, D);
        float delta[NCH], dot = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int c = gl + ch * G;
          const float pre = sX[jj * CP + c] + gine_e(L, A, a, ch, c, F);
          const bool on = pre > 0.f && c < F;
          dot = fmaf(go[r][ch], on ? pre : 0.f, dot);
          delta[ch] = on ? av * go[r][ch] : 0.f;
          if (DB == 0 && ga && c < F) ga[c] = delta[ch];
        }
        if (g_adj) {
          dot = group_sum<G>(dot);
          if (gl == 0) g_adj[abase + jj] = dot;
        }
        if (DB > 0) {
#pragma unroll
          for (int d = 0; d < DB; ++d) {
            float t = 0.f;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
              t = fmaf(L.w[ch][d], delta[ch], t);
              gw[ch][d] = fmaf(delta[ch], A.v[d], gw[ch][d]);
            }
            if (ga && d < D) {  // uniform
              t = group_sum<G>(t);
              if (gl == 0) ga[d] = t;
            }
          }
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) gb[ch] += delta[ch];
        }
      }
    }
  }
  if (DB > 0 && part) gine_write_part<G, NCH, DB>(gw, gb, part, red, blockIdx.y * gridDim.x + blockIdx.x, F, D);
}

// by neighbour block over the transposed image: g_x[j] = s g_h[j] + sum_i adj_ij g_h[i] * [x_j + e_ij > 0]
template <int G, int NCH, int DB>
__global__ __launch_bounds__(256) void k_gine_dense_dcol(const unsigned* __restrict__ bitsT,
                                                         const float* __restrict__ adj, const float* __restrict__ x,
                                                         const float* __restrict__ g_h, const float* __restrict__ ea,
                                                         const float* __restrict__ w_e, const float* __restrict__ b_e,
                                                         const float* __restrict__ eps, float* __restrict__ g_x, int N,
                                                         int F, int D, int add_loop) {
  constexpr int CP = G * NCH, S = 256 / G;
  __shared__ float sG[GT * CP];  // [i][c]
  const int b = blockIdx.y, j0 = blockIdx.x * (S * GINE_RPG);
  const int slot = threadIdx.x / G, gl = threadIdx.x % G;
  const int W = (N + 31) / 32;
  const size_t rb = (size_t)b * N;
  Lin<G, NCH, DB> L;
  L.load(w_e, b_e, gl, F, D);
  float xj[GINE_RPG][NCH], acc[GINE_RPG][NCH];
#pragma unroll
  for (int r = 0; r < GINE_RPG; ++r) {
    const int j = j0 + r * S + slot;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      xj[r][ch] = (j < N && c < F) ? x[(rb + j) * F + c] : 0.f;
      acc[r][ch] = 0.f;
    }
  }

  for (int w = 0; w < W; ++w) {
    unsigned word[GINE_RPG], any = 0u;
#pragma unroll
    for (int r = 0; r < GINE_RPG; ++r) {
      const int j = j0 + r * S + slot;
      word[r] = j < N ? bitsT[(rb + j) * W + w] : 0u;
      any |= word[r];
    }
    if (!__syncthreads_or(any != 0u)) continue;
    gine_stage<CP>(sG, g_h, rb, w * 32, N, F);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GINE_RPG; ++r) {
      const int j = j0 + r * S + slot;
      unsigned m = word[r];
      while (m) {
        const int ii = __ffs(m) - 1;
        m &= m - 1u;
        const size_t o = (rb + w * 32 + ii) * N + j;
        const float av = adj[o];
        const float* a = ea + o * D;
        Attr<DB> A;
        A.load(a, D);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int c = gl + ch * G;
          const float pre = xj[r][ch] + gine_e(L, A, a, ch, c, F);
          acc[r][ch] = fmaf(av, pre > 0.f ? sG[ii * CP + c] : 0.f, acc[r][ch]);
        }
      }
    }
  }
  const float s = add_loop ? 1.f + eps[0] : 0.f;
#pragma unroll
  for (int r = 0; r < GINE_RPG; ++r) {
    const int j = j0 + r * S + slot;
    if (j >= N) continue;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      if (c >= F) continue;
      float v = acc[r][ch];
      if (add_loop) v = fmaf(s, g_h[(rb + j) * F + c], v);
      g_x[(rb + j) * F + c] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// RelativeEdgeAttr
// ---------------------------------------------------------------------------
// one thread per (edge, column)
__global__ __launch_bounds__(256) void k_rel_fwd(const float* __restrict__ x, const int64_t* __restrict__ ei,
                                                 float* __restrict__ out, int64_t E, int F, int p0, int P, int time,
                                                 float ts) {
  const int D = time + P;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= E * D) return;
  const int64_t k = t / D;
  const int d = (int)(t - k * D);
  const int64_t src = ei[k], dst = ei[E + k];
  out[t] = (time && d == 0) ? (float)(dst - src) * ts
                            : x[(size_t)src * F + p0 + d - time] - x[(size_t)dst * F + p0 + d - time];
}

// one thread per (node, feature column)
__global__ __launch_bounds__(256) void k_rel_bwd(const float* __restrict__ g, const int64_t* __restrict__ row_ptr,
                                                 const int64_t* __restrict__ csr_perm,
                                                 const int64_t* __restrict__ col_ptr,
                                                 const int64_t* __restrict__ csc_perm, float* __restrict__ g_x,
                                                 int64_t M, int F, int p0, int P, int time) {
  const int D = time + P;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * F) return;
  const int64_t n = t / F;
  const int f = (int)(t - n * F);
  float as_src = 0.f, as_dst = 0.f;
  if (f >= p0 && f < p0 + P && row_ptr) {
    const int d = time + f - p0;
    for (int64_t p = col_ptr[n]; p < col_ptr[n + 1]; ++p) as_src += g[(size_t)csc_perm[p] * D + d];
    for (int64_t p = row_ptr[n]; p < row_ptr[n + 1]; ++p) as_dst += g[(size_t)(csr_perm ? csr_perm[p] : p) * D + d];
  }
  g_x[t] = as_src - as_dst;
}

// one thread per (b, i, j, column)
__global__ __launch_bounds__(256) void k_rel_dense_fwd(const float* __restrict__ x, float* __restrict__ out,
                                                       int64_t total, int N, int F, int p0, int P, int time,
                                                       float ts) {
  const int D = time + P;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int d = (int)(t % D);
  const int64_t ij = t / D;
  const int j = (int)(ij % N);
  const int64_t bi = ij / N;  // b * N + i
  const int i = (int)(bi % N);
  const int64_t bj = bi - i + j;
  out[t] = (time && d == 0) ? (float)(i - j) * ts : x[(size_t)bj * F + p0 + d - time] - x[(size_t)bi * F + p0 + d - time];
}

// one thread per (b, n, feature column): the column sum minus the row sum, each in index order
__global__ __launch_bounds__(256) void k_rel_dense_bwd(const float* __restrict__ g, float* __restrict__ g_x,
                                                       int64_t total, int N, int F, int p0, int P, int time) {
  const int D = time + P;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int64_t bn = t / F;
  const int f = (int)(t - bn * F);
  float cs = 0.f, rs = 0.f;
  if (f >= p0 && f < p0 + P) {
    const int d = time + f - p0;
    const int n = (int)(bn % N);
    const size_t base = (size_t)(bn - n) * N;  // b * N * N
    for (int i = 0; i < N; ++i) cs += g[(base + (size_t)i * N + n) * D + d];
    for (int j = 0; j < N; ++j) rs += g[(base + (size_t)n * N + j) * D + d];
  }
  g_x[t] = cs - rs;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool gine_unsupported(int64_t R, int F, int D, bool lin) {
  return F > 128 || R > (1 << 30) || (lin && D > GCM_GINE_MAX_EDGE_DIM);
}

// launch K<G, NCH, DB> with the lane group of this F and the register bucket of this D (0 without lin)
#define GINE_LAUNCH_G(K, DB, GRID, s, ...)                                                          \
  if (F <= 8) hipLaunchKernelGGL((K<8, 1, DB>), GRID(8), dim3(256), 0, s, __VA_ARGS__);             \
  else if (F <= 16) hipLaunchKernelGGL((K<16, 1, DB>), GRID(16), dim3(256), 0, s, __VA_ARGS__);     \
  else if (F <= 32) hipLaunchKernelGGL((K<32, 1, DB>), GRID(32), dim3(256), 0, s, __VA_ARGS__);     \
  else if (F <= 64) hipLaunchKernelGGL((K<64, 1, DB>), GRID(64), dim3(256), 0, s, __VA_ARGS__);     \
  else hipLaunchKernelGGL((K<64, 2, DB>), GRID(64), dim3(256), 0, s, __VA_ARGS__);
#define GINE_LAUNCH(K, GRID, s, ...)                      \
  if (!w_e) {                                             \
    GINE_LAUNCH_G(K, 0, GRID, s, __VA_ARGS__)             \
  } else if (D <= 4) {                                    \
    GINE_LAUNCH_G(K, 4, GRID, s, __VA_ARGS__)             \
  } else {                                                \
    GINE_LAUNCH_G(K, 32, GRID, s, __VA_ARGS__)            \
  }

#define GINE_CSR_GRID(G) dim3(blocks(M * (G), 256))
#define GINE_DROW_GRID(G) dim3(nb)
#define GINE_DENSE_GRID(G) dim3(blocks(N, (256 / (G)) * GINE_RPG), B)

int lane_group(int F) { return F <= 8 ? 8 : F <= 16 ? 16 : F <= 32 ? 32 : 64; }

// the sparse row sweep's grid: one group per row up to GINE_PARTS workgroups, then rows are strided
unsigned csr_drow_blocks(int64_t M, int F) {
  return (unsigned)std::min<int64_t>(GINE_PARTS, blocks(M * lane_group(F), 256));
}
unsigned dense_row_blocks(int N, int F) { return blocks(N, (256 / lane_group(F)) * GINE_RPG); }

int sum_param_parts(const float* part, int n, float* g_w, float* g_b, int F, int D, hipStream_t s) {
  hipLaunchKernelGGL(k_gine_sum_parts, dim3(blocks((int64_t)F * (D + 1), 16)), dim3(256), 0, s, part, n, g_w, g_b, F,
                     D);
  return gcm_launch_status();
}

struct CsrWs {
  size_t dot, part, total;
};
CsrWs csr_ws(int64_t M, int F, int D) {
  CsrWs w;
  Carve c;
  w.dot = c.take(dot_ws_bytes(M * F));
  w.part = c.take((size_t)csr_drow_blocks(M, F) * F * (D + 1) * 4);
  w.total = c.at;
  return w;
}

struct DenseWs {
  size_t dot, part, bitsT, total;
};
DenseWs dense_ws(int B, int N, int F, int D) {
  DenseWs w;
  Carve c;
  w.dot = c.take(dot_ws_bytes((int64_t)B * N * F));
  w.part = c.take((size_t)B * dense_row_blocks(N, F) * F * (D + 1) * 4);
  w.bitsT = c.take((size_t)B * N * ((N + 31) / 32) * 4);
  w.total = c.at;
  return w;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: GINEConv
// ---------------------------------------------------------------------------
extern "C" int gcm_csr_gine_fwd(const float* x, const float* edge_attr, const float* w_e, const float* b_e,
                                const float* eps, const int64_t* row_ptr, const int64_t* col, const int64_t* csr_perm,
                                float* h, int64_t M, int64_t E, int F, int D, gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && eps && h);
  GCM_REQUIRE(M > 0 && E >= 0 && F > 0 && D > 0);
  GCM_REQUIRE(E == 0 || (col && edge_attr));
  GCM_REQUIRE(!w_e == !b_e && (w_e || D == F));
  if (gine_unsupported(M, F, D, w_e != nullptr)) return GCM_EUNSUPPORTED;
  GINE_LAUNCH(k_gine_csr_fwd, GINE_CSR_GRID, (hipStream_t)stream, x, edge_attr, w_e, b_e, eps,
              E > 0 ? row_ptr : nullptr, col, csr_perm, h, M, F, D)
  return gcm_launch_status();
}

extern "C" size_t gcm_csr_gine_bwd_workspace_bytes(int64_t M, int64_t E, int F, int D) {
  if (M <= 0 || E < 0 || F <= 0 || D <= 0) return 0;
  return csr_ws(M, F, D).total;
}

extern "C" int gcm_csr_gine_bwd(const float* g_h, const float* x, const float* edge_attr, const float* w_e,
                                const float* b_e, const float* eps, const int64_t* row_ptr, const int64_t* col,
                                const int64_t* csr_perm, const int64_t* col_ptr, const int64_t* rows,
                                const int64_t* csc_perm, float* g_x, float* g_edge_attr, float* g_w_e, float* g_b_e,
                                float* g_eps, void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int F,
                                int D, gcm_stream_t stream) {
  GCM_REQUIRE(g_h && x && eps && row_ptr && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && F > 0 && D > 0);
  GCM_REQUIRE(E == 0 || (col && edge_attr));
  GCM_REQUIRE(E == 0 || !g_x || (col_ptr && rows && csc_perm));
  GCM_REQUIRE(!w_e == !b_e && (w_e || D == F));
  GCM_REQUIRE(w_e || (!g_w_e && !g_b_e));
  if (gine_unsupported(M, F, D, w_e != nullptr)) return GCM_EUNSUPPORTED;
  const CsrWs K = csr_ws(M, F, D);
  GCM_REQUIRE(workspace_bytes >= K.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int rc;
  if (g_x) {
    GINE_LAUNCH(k_gine_csr_dcol, GINE_CSR_GRID, s, x, g_h, edge_attr, w_e, b_e, eps, E > 0 ? col_ptr : nullptr, rows,
                csc_perm, g_x, M, F, D)
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_edge_attr || g_w_e || g_b_e) {
    float* part = (g_w_e || g_b_e) ? (float*)(ws + K.part) : nullptr;
    const unsigned nb = csr_drow_blocks(M, F);
    GINE_LAUNCH(k_gine_csr_drow, GINE_DROW_GRID, s, x, g_h, edge_attr, w_e, b_e, row_ptr, col, csr_perm, g_edge_attr,
                part, M, F, D)
    if ((rc = gcm_launch_status())) return rc;
    if (part && (rc = sum_param_parts(part, (int)nb, g_w_e, g_b_e, F, D, s))) return rc;
  }
  return g_eps ? dot_sum(g_h, x, M * F, g_eps, ws + K.dot, s) : GCM_OK;
}

// ---------------------------------------------------------------------------
// C ABI: DenseGINEConv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_dense_gine_fwd_workspace_bytes(int B, int N, int F, int D) {
  if (B <= 0 || N <= 0 || F <= 0 || D <= 0) return 0;
  return align256((size_t)B * N * ((N + 31) / 32) * 4);
}

extern "C" int gcm_dense_gine_fwd(const float* x, const float* adj, const float* edge_attr, const float* w_e,
                                  const float* b_e, const float* eps, float* h, void* saved, size_t saved_bytes, int B,
                                  int N, int F, int D, int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && edge_attr && eps && h && saved);
  GCM_REQUIRE(B > 0 && N > 0 && F > 0 && D > 0);
  GCM_REQUIRE(!w_e == !b_e && (w_e || D == F));
  const int64_t R = (int64_t)B * N;
  if (gine_unsupported(R, F, D, w_e != nullptr) || B > 65535) return GCM_EUNSUPPORTED;
  GCM_REQUIRE(saved_bytes >= gcm_dense_gine_fwd_workspace_bytes(B, N, F, D));
  hipStream_t s = (hipStream_t)stream;
  const int W = (N + 31) / 32;
  unsigned* bits = (unsigned*)saved;
  int rc = mask_bits(adj, bits, R, N, W, 0, s);
  if (rc) return rc;
  GINE_LAUNCH(k_gine_dense_fwd, GINE_DENSE_GRID, s, (const unsigned*)bits, adj, x, edge_attr, w_e, b_e, eps, h, N, F,
              D, add_loop)
  return gcm_launch_status();
}

extern "C" size_t gcm_dense_gine_bwd_workspace_bytes(int B, int N, int F, int D) {
  if (B <= 0 || N <= 0 || F <= 0 || D <= 0) return 0;
  return dense_ws(B, N, F, D).total;
}

extern "C" int gcm_dense_gine_bwd(const float* g_h, const float* x, const float* adj, const float* edge_attr,
                                  const float* w_e, const float* b_e, const float* eps, const void* saved, float* g_x,
                                  float* g_adj, float* g_edge_attr, float* g_w_e, float* g_b_e, float* g_eps,
                                  void* workspace, size_t workspace_bytes, int B, int N, int F, int D, int add_loop,
                                  gcm_stream_t stream) {
  GCM_REQUIRE(g_h && x && adj && edge_attr && eps && saved && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && F > 0 && D > 0);
  GCM_REQUIRE(!w_e == !b_e && (w_e || D == F));
  GCM_REQUIRE(w_e || (!g_w_e && !g_b_e));
  const int64_t R = (int64_t)B * N;
  if (gine_unsupported(R, F, D, w_e != nullptr) || B > 65535) return GCM_EUNSUPPORTED;
  const DenseWs K = dense_ws(B, N, F, D);
  GCM_REQUIRE(workspace_bytes >= K.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int W = (N + 31) / 32;
  const unsigned* bits = (const unsigned*)saved;
  int rc;
  if (g_x) {
    unsigned* bitsT = (unsigned*)(ws + K.bitsT);
    if ((rc = mask_bits_t(bits, bitsT, R, N, W, s))) return rc;
    GINE_LAUNCH(k_gine_dense_dcol, GINE_DENSE_GRID, s, (const unsigned*)bitsT, adj, x, g_h, edge_attr, w_e, b_e, eps,
                g_x, N, F, D, add_loop)
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_adj || g_edge_attr || g_w_e || g_b_e) {
    float* part = (g_w_e || g_b_e) ? (float*)(ws + K.part) : nullptr;
    if (g_edge_attr && !g_adj) {  // the sweep visits the set entries only: the rest is zero
      if (hipMemsetAsync(g_edge_attr, 0, (size_t)R * N * D * 4, s) != hipSuccess) return gcm_launch_status();
    }
    GINE_LAUNCH(k_gine_dense_drow, GINE_DENSE_GRID, s, bits, adj, x, g_h, edge_attr, w_e, b_e, g_adj, g_edge_attr, part,
                N, F, D)
    if ((rc = gcm_launch_status())) return rc;
    if (part && (rc = sum_param_parts(part, (int)(B * dense_row_blocks(N, F)), g_w_e, g_b_e, F, D, s))) return rc;
  }
  if (g_eps) {
    if (add_loop) return dot_sum(g_h, x, R * F, g_eps, ws + K.dot, s);
    return sum_parts((const double*)(ws + K.dot), 0, g_eps, s);  // eps is not used: the sum of no partials
  }
  return GCM_OK;
}

// ---------------------------------------------------------------------------
// C ABI: RelativeEdgeAttr
// ---------------------------------------------------------------------------
extern "C" int gcm_rel_edge_attr_fwd(const float* x, const int64_t* edge_index, float* out, int64_t M, int64_t E, int F,
                                     int p0, int P, int time, float time_scale, gcm_stream_t stream) {
  GCM_REQUIRE(M > 0 && E >= 0 && F > 0 && p0 >= 0 && P >= 0 && p0 + P <= F && (time == 0 || time == 1));
  GCM_REQUIRE(time + P > 0 && (P == 0 || x));
  if (E == 0) return GCM_OK;
  GCM_REQUIRE(edge_index && out);
  if (M > (1 << 30) || E * (time + P) > ((int64_t)1 << 38)) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_rel_fwd, dim3(blocks(E * (time + P), 256)), dim3(256), 0, (hipStream_t)stream, x, edge_index,
                     out, E, F, p0, P, time, time_scale);
  return gcm_launch_status();
}

extern "C" int gcm_rel_edge_attr_bwd(const float* g_out, const int64_t* row_ptr, const int64_t* csr_perm,
                                     const int64_t* col_ptr, const int64_t* csc_perm, float* g_x, int64_t M, int64_t E,
                                     int F, int p0, int P, int time, gcm_stream_t stream) {
  GCM_REQUIRE(g_x);
  GCM_REQUIRE(M > 0 && E >= 0 && F > 0 && p0 >= 0 && P >= 0 && p0 + P <= F && (time == 0 || time == 1));
  GCM_REQUIRE(E == 0 || (g_out && row_ptr && col_ptr && csc_perm));
  if (M > (1 << 30)) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_rel_bwd, dim3(blocks(M * F, 256)), dim3(256), 0, (hipStream_t)stream, g_out,
                     E > 0 ? row_ptr : nullptr, csr_perm, col_ptr, csc_perm, g_x, M, F, p0, P, time);
  return gcm_launch_status();
}

extern "C" int gcm_dense_rel_edge_attr_fwd(const float* x, float* out, int B, int N, int F, int p0, int P, int time,
                                           float time_scale, gcm_stream_t stream) {
  GCM_REQUIRE(out);
  GCM_REQUIRE(B > 0 && N > 0 && F > 0 && p0 >= 0 && P >= 0 && p0 + P <= F && (time == 0 || time == 1));
  GCM_REQUIRE(time + P > 0 && (P == 0 || x));
  const int64_t total = (int64_t)B * N * N * (time + P);
  if (total > ((int64_t)1 << 38)) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_rel_dense_fwd, dim3(blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, x, out, total, N, F,
                     p0, P, time, time_scale);
  return gcm_launch_status();
}

extern "C" int gcm_dense_rel_edge_attr_bwd(const float* g_out, float* g_x, int B, int N, int F, int p0, int P, int time,
                                           gcm_stream_t stream) {
  GCM_REQUIRE(g_out && g_x);
  GCM_REQUIRE(B > 0 && N > 0 && F > 0 && p0 >= 0 && P >= 0 && p0 + P <= F && (time == 0 || time == 1));
  const int64_t total = (int64_t)B * N * F;
  if (total > ((int64_t)1 << 38)) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_rel_dense_bwd, dim3(blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, g_out, g_x, total, N,
                     F, p0, P, time);
  return gcm_launch_status();
}
