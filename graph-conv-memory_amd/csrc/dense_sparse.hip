// The bridge between DenseGCM's (nodes [B,N,F], adj [B,N,N]) and the flat edge lists of the sparse layers
// (gcm.gcm.DenseToSparse / SparseToDense; include/gcm_hip_bridge.h), on gfx950.
//
// Dense -> sparse.  The entries adj[b,r,c] > 0 in row-major order (b, r, c) ARE the edge list (torch.nonzero's order),
// and the same entries in column-major order (b, c, r) are the other view the sparse layers need (CSR by sink when the
// row is the source, CSC by source when the row is the sink): a dense adjacency is already sorted both ways, so the
// index is built by counting, without a sort.
//
//   k_bridge_image   one workgroup per graph, up to 16 waves: a wave reads 64 columns of eight rows at a time (the
//                    kernel is bound by the latency of these loads: all of a graph's rows are in flight at once at
//                    N = 128), the ballot of `> 0` is one word of the bit image, its popcount goes to the row's count,
//                    the set lanes count their column in LDS (integer adds: the result has no order)
//   k_bridge_scan    one workgroup: exclusive prefix of the per-graph totals, in chunks of 1024 with a carry
//   k_bridge_fill    one workgroup per graph with the graph's image in LDS, thread = column c of one slice of the
//                    rows, walking its rows upwards: the entry (r, c) is the thread's next column-major number q
//                    (first: the column's offset + the bits of the column above the slice), and its row-major
//                    number p is the row's offset + the popcounts of the words before c's + the set bits below c in
//                    c's word - everything both orders need in one walk (the words of a row are broadcast LDS reads)
//
// Sparse -> dense.  Nodes by a gather per output element; the adjacency by one thread per SINK walking its CSR entries
// in order, which owns column d of its graph: duplicates add in one order, no atomics; the gradients are gathers.
// Every index read from memory is checked against its range before it addresses anything; int64 element offsets.
#include <algorithm>

#include "gcm_common.h"

namespace {

constexpr int kMaxN = GCM_BRIDGE_MAX_N;
constexpr int kImageWaves = 16;   // the most waves of a k_bridge_image workgroup
constexpr int kRows = 8;          // rows a wave of k_bridge_image has in flight
constexpr int kFillThreads = 1024, kFillSlices = 8, kSliceRows = 16;   // k_bridge_fill: 64 W threads per slice of rows
constexpr int kScanThreads = 1024;
constexpr int kThreads = 256;     // the element-wise kernels
static_assert(kMaxN % 64 == 0 && kMaxN <= 1024, "one thread per column, whole waves");

template <typename T>
__global__ __launch_bounds__(64 * kImageWaves) void k_bridge_image(const T* __restrict__ adj, uint64_t* __restrict__ image,
                                                                int32_t* __restrict__ row_cnt,
                                                                int32_t* __restrict__ col_cnt,
                                                                int32_t* __restrict__ total, int N, int W) {
  __shared__ int s_col[kMaxN];
  __shared__ int s_tot[kImageWaves];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  for (int c = threadIdx.x; c < N; c += blockDim.x) s_col[c] = 0;
  __syncthreads();
  const T* __restrict__ g = adj + (size_t)b * N * N;
  uint64_t* __restrict__ img = image + (size_t)b * N * W;
  int tot = 0;
  for (int r0 = wave * kRows; r0 < N; r0 += waves * kRows) {   // (wave-uniform bounds: every ballot is whole)
    int rc[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u) rc[u] = 0;
    for (int k = 0; k < W; ++k) {
      const int c = k * 64 + lane;
      bool bit[kRows];
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        bit[u] = (r0 + u < N && c < N) ? g[(size_t)(r0 + u) * N + c] > T(0) : false;
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
        const uint64_t w = __ballot(bit[u]);
        if (r0 + u < N) {
          if (lane == 0) img[(size_t)(r0 + u) * W + k] = w;
          rc[u] += __popcll(w);
          if (bit[u]) atomicAdd(&s_col[c], 1);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      if (r0 + u < N) {
        if (lane == 0) row_cnt[(size_t)b * N + r0 + u] = rc[u];
        tot += rc[u];
      }
    }
  }
  if (lane == 0) s_tot[wave] = tot;
  __syncthreads();
  for (int c = threadIdx.x; c < N; c += blockDim.x) col_cnt[(size_t)b * N + c] = s_col[c];
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < waves; ++w) t += s_tot[w];
    total[b] = t;
  }
}

__device__ __forceinline__ int64_t shfl_up_i64(int64_t v, int d) {
  const int lo = __shfl_up((int)(v & 0xffffffffll), d), hi = __shfl_up((int)(v >> 32), d);
  return ((int64_t)hi << 32) | (uint32_t)lo;
}

__global__ __launch_bounds__(kScanThreads) void k_bridge_scan(const int32_t* __restrict__ total,
                                                              int64_t* __restrict__ graph_off, int B) {
  __shared__ int64_t s_wave[kScanThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int b0 = 0; b0 < B; b0 += kScanThreads) {     // (block-uniform bounds)
    const int b = b0 + threadIdx.x;
    const int64_t c = b < B ? (total[b] > 0 ? total[b] : 0) : 0;
    int64_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = shfl_up_i64(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int64_t base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
      const int64_t v = s_wave[w];
      if (w < wave) base += v;
      sum += v;
    }
    if (b < B) graph_off[b] = carry + base + incl - c;
    carry += sum;
    __syncthreads();      // s_wave is written again by the next chunk
  }
  if (threadIdx.x == 0) graph_off[B] = carry;
}

template <typename T>
__global__ __launch_bounds__(kFillThreads) void k_bridge_fill(
    const T* __restrict__ adj, const uint64_t* __restrict__ image, const int32_t* __restrict__ row_cnt,
    const int32_t* __restrict__ col_cnt, const int64_t* __restrict__ graph_off, int64_t* __restrict__ edge_index,
    int64_t* __restrict__ row_ptr, int64_t* __restrict__ col_ptr, int64_t* __restrict__ by_col,
    int64_t* __restrict__ col_pos, int64_t* __restrict__ col_rows, float* __restrict__ values, int B, int N, int W,
    int S, int64_t E, int transpose) {
  extern __shared__ uint64_t s_img[];     // the graph's image, N W words
  __shared__ int s_row[kMaxN];            // first row-major number of each row, relative to the graph's
  __shared__ int s_col[kMaxN];            // first column-major number of each column
  __shared__ int s_wave[2][kMaxN / 64];
  // blockDim.x = 64 W S: slice s of the rows, column t, word k < W of a row
  const int b = blockIdx.x, cols = 64 * W, slice = threadIdx.x / cols, t = threadIdx.x - slice * cols;
  const int lane = t & 63, k = t >> 6;
  const int64_t node0 = (int64_t)b * N, e0 = graph_off[b];
  const uint64_t* __restrict__ img = image + (size_t)node0 * W;
  for (int i = threadIdx.x; i < N * W; i += blockDim.x) s_img[i] = img[i];
  int rc = 0, cc = 0, ri = 0, ci = 0;
  if (slice == 0) {                       // (whole waves: 64 W threads a slice)
    rc = t < N ? max(row_cnt[node0 + t], 0) : 0, cc = t < N ? max(col_cnt[node0 + t], 0) : 0;
    ri = rc, ci = cc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int ru = __shfl_up(ri, d), cu = __shfl_up(ci, d);
      if (lane >= d) ri += ru, ci += cu;
    }
    if (lane == 63) s_wave[0][k] = ri, s_wave[1][k] = ci;
  }
  __syncthreads();
  if (slice == 0) {
    int rbase = 0, cbase = 0;
    for (int w = 0; w < k; ++w) rbase += s_wave[0][w], cbase += s_wave[1][w];
    const int rex = rbase + ri - rc, cex = cbase + ci - cc;
    if (t < N) {
      s_row[t] = rex;
      s_col[t] = cex;
      row_ptr[node0 + t] = e0 + rex;
      col_ptr[node0 + t] = e0 + cex;
    }
    if (b == B - 1 && t == 0) row_ptr[node0 + N] = E, col_ptr[node0 + N] = E;
  }
  __syncthreads();
  const int per = (N + S - 1) / S, r0 = slice * per, r1 = min(N, r0 + per);
  if (E == 0 || t >= N || r0 >= r1) return;     // (no barrier and no cross-lane operation below)
  int above = 0;
  for (int r = 0; r < r0; ++r) above += (int)((s_img[r * W + k] >> lane) & 1ull);
  const uint64_t below = (1ull << lane) - 1ull;
  int64_t q = e0 + s_col[t] + above;
  for (int r = r0; r < r1; ++r) {
    const uint64_t* row = s_img + r * W;
    const uint64_t w = row[k];
    int before = 0;
    for (int j = 0; j < k; ++j) before += __popcll(row[j]);
    if ((w >> lane) & 1ull) {
      const int64_t p = e0 + s_row[r] + before + __popcll(w & below);
      if ((uint64_t)p < (uint64_t)E && (uint64_t)q < (uint64_t)E) {
        const int64_t rn = node0 + r, cn = node0 + t;
        edge_index[p] = transpose ? cn : rn;
        edge_index[E + p] = transpose ? rn : cn;
        by_col[q] = p;
        if (col_pos) col_pos[p] = q;
        col_rows[q] = rn;
        if (values) values[p] = (float)adj[((size_t)node0 + r) * N + t];
      }
      ++q;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_bridge_values_bwd(const float* __restrict__ g_values,
                                                                const int64_t* __restrict__ edge_index,
                                                                float* __restrict__ g_adj, int64_t M, int N, int64_t E,
                                                                int transpose) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= E) return;
  const int64_t s = edge_index[p], d = edge_index[E + p];
  const int64_t rn = transpose ? d : s, cn = transpose ? s : d;
  if ((uint64_t)rn >= (uint64_t)M || (uint64_t)cn >= (uint64_t)M) return;
  const int64_t b = rn / N;
  if (cn / N != b) return;
  g_adj[(size_t)rn * N + (cn - b * N)] = g_values[p];
}

__global__ __launch_bounds__(kThreads) void k_bridge_dense_nodes(const float* __restrict__ x_sp,
                                                                 const int64_t* __restrict__ node_ptr,
                                                                 float* __restrict__ x, int64_t M, int64_t total, int N,
                                                                 int F) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int f = (int)(i % F);
  const int64_t bn = i / F, b = bn / N, n = bn - b * N;
  const int64_t lo = node_ptr[b], hi = min(node_ptr[b + 1], M), m = lo + n;
  x[i] = (lo >= 0 && m < hi) ? x_sp[(size_t)m * F + f] : 0.f;
}

__global__ __launch_bounds__(kThreads) void k_bridge_dense_nodes_bwd(const float* __restrict__ g_x,
                                                                     const int64_t* __restrict__ batch_idx,
                                                                     const int64_t* __restrict__ node_ptr,
                                                                     float* __restrict__ g_x_sp, int64_t total, int B,
                                                                     int N, int F) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int f = (int)(i % F);
  const int64_t m = i / F, b = batch_idx[m];
  float g = 0.f;
  if ((uint64_t)b < (uint64_t)B) {
    const int64_t pos = m - node_ptr[b];
    if ((uint64_t)pos < (uint64_t)N) g = g_x[((size_t)b * N + pos) * F + f];
  }
  g_x_sp[i] = g;
}

// (graph, position in it) of node m, or b = -1 when it has no place in [B, N]
struct Place {
  int64_t b, pos;
};
__device__ __forceinline__ Place place_of(int64_t m, const int64_t* __restrict__ batch_idx,
                                          const int64_t* __restrict__ node_ptr, int64_t M, int B, int N) {
  Place r{-1, 0};
  if ((uint64_t)m >= (uint64_t)M) return r;
  const int64_t b = batch_idx[m];
  if ((uint64_t)b >= (uint64_t)B) return r;
  const int64_t pos = m - node_ptr[b];
  if ((uint64_t)pos >= (uint64_t)N) return r;
  r.b = b, r.pos = pos;
  return r;
}

template <bool PERM, bool WEIGHT>
__global__ __launch_bounds__(kThreads) void k_bridge_dense_adj(const int64_t* __restrict__ row_ptr,
                                                               const int64_t* __restrict__ csr_perm,
                                                               const int64_t* __restrict__ edge_index,
                                                               const float* __restrict__ edge_weight,
                                                               const int64_t* __restrict__ batch_idx,
                                                               const int64_t* __restrict__ node_ptr,
                                                               float* __restrict__ adj, int64_t M, int64_t E, int B,
                                                               int N) {
  const int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (m >= M) return;
  const Place d = place_of(m, batch_idx, node_ptr, M, B, N);
  if (d.b < 0) return;
  const int64_t k0 = max(row_ptr[m], (int64_t)0), k1 = min(row_ptr[m + 1], E);
  float* __restrict__ column = adj + (size_t)d.b * N * N + d.pos;     // this thread's alone
  for (int64_t k = k0; k < k1; ++k) {
    int64_t e = k;
    if constexpr (PERM) e = csr_perm[k];
    if ((uint64_t)e >= (uint64_t)E) continue;
    const Place s = place_of(edge_index[e], batch_idx, node_ptr, M, B, N);
    if (s.b != d.b) continue;
    float w = 1.f;
    if constexpr (WEIGHT) w = edge_weight[e];
    column[(size_t)s.pos * N] += w;
  }
}

__global__ __launch_bounds__(kThreads) void k_bridge_dense_adj_bwd(const float* __restrict__ g_adj,
                                                                   const int64_t* __restrict__ edge_index,
                                                                   const int64_t* __restrict__ batch_idx,
                                                                   const int64_t* __restrict__ node_ptr,
                                                                   float* __restrict__ g_weight, int64_t M, int64_t E,
                                                                   int B, int N) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const Place s = place_of(edge_index[e], batch_idx, node_ptr, M, B, N);
  const Place d = place_of(edge_index[E + e], batch_idx, node_ptr, M, B, N);
  g_weight[e] = (s.b >= 0 && s.b == d.b) ? g_adj[((size_t)s.b * N + s.pos) * N + d.pos] : 0.f;
}

// blocks of kThreads over n elements; 0 when the grid would not fit
unsigned blocks_of(int64_t n) {
  const int64_t g = (n + kThreads - 1) / kThreads;
  return g > 0x7fffffffll ? 0u : (unsigned)g;
}

}  // namespace

extern "C" int gcm_bridge_image(const void* adj, int adj_i64, uint64_t* image, int32_t* row_cnt, int32_t* col_cnt,
                                int32_t* total, int B, int N, gcm_stream_t stream) {
  GCM_REQUIRE(adj && image && row_cnt && col_cnt && total && B > 0 && N > 0);
  if (N > kMaxN) return GCM_EUNSUPPORTED;
  const int W = (N + 63) / 64, waves = std::min(kImageWaves, (N + kRows - 1) / kRows);
  return gcm_pick(
      [&](auto i64) {
        using T = std::conditional_t<i64() != 0, int64_t, float>;
        hipLaunchKernelGGL((k_bridge_image<T>), dim3(B), dim3(64 * waves), 0, (hipStream_t)stream, (const T*)adj,
                           image, row_cnt, col_cnt, total, N, W);
        return gcm_launch_status();
      },
      Flag{adj_i64 != 0});
}

extern "C" int gcm_bridge_scan(const int32_t* total, int64_t* graph_off, int B, gcm_stream_t stream) {
  GCM_REQUIRE(total && graph_off && B > 0);
  hipLaunchKernelGGL(k_bridge_scan, dim3(1), dim3(kScanThreads), 0, (hipStream_t)stream, total, graph_off, B);
  return gcm_launch_status();
}

extern "C" int gcm_bridge_fill(const void* adj, int adj_i64, const uint64_t* image, const int32_t* row_cnt,
                               const int32_t* col_cnt, const int64_t* graph_off, int64_t* edge_index,
                               int64_t* row_ptr, int64_t* col_ptr, int64_t* by_col, int64_t* col_pos,
                               int64_t* col_rows, float* values, int B, int N, int64_t E, int transpose,
                               gcm_stream_t stream) {
  GCM_REQUIRE(image && row_cnt && col_cnt && graph_off && row_ptr && col_ptr && B > 0 && N > 0 && E >= 0);
  GCM_REQUIRE(E == 0 || (edge_index && by_col && col_rows));
  GCM_REQUIRE(!values || adj);
  if (N > kMaxN) return GCM_EUNSUPPORTED;
  // slices of at least kSliceRows rows, as many as fit a workgroup of kFillThreads
  const int W = (N + 63) / 64;
  const int S = std::max(1, std::min({kFillSlices, kFillThreads / (64 * W), (N + kSliceRows - 1) / kSliceRows}));
  return gcm_pick(
      [&](auto i64) {
        using T = std::conditional_t<i64() != 0, int64_t, float>;
        hipLaunchKernelGGL((k_bridge_fill<T>), dim3(B), dim3(64 * W * S), sizeof(uint64_t) * N * W,
                           (hipStream_t)stream, (const T*)adj, image, row_cnt, col_cnt, graph_off, edge_index,
                           row_ptr, col_ptr, by_col, col_pos, col_rows, values, B, N, W, S, E, transpose);
        return gcm_launch_status();
      },
      Flag{adj_i64 != 0});
}

extern "C" int gcm_bridge_values_bwd(const float* g_values, const int64_t* edge_index, float* g_adj, int B, int N,
                                     int64_t E, int transpose, gcm_stream_t stream) {
  GCM_REQUIRE(g_adj && B > 0 && N > 0 && E >= 0);
  GCM_REQUIRE(E == 0 || (g_values && edge_index));
  const hipError_t e = hipMemsetAsync(g_adj, 0, sizeof(float) * (size_t)B * N * N, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  if (E == 0) return GCM_OK;
  const unsigned grid = blocks_of(E);
  if (!grid) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_bridge_values_bwd, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g_values, edge_index,
                     g_adj, (int64_t)B * N, N, E, transpose);
  return gcm_launch_status();
}

extern "C" int gcm_bridge_dense_nodes(const float* x_sp, const int64_t* node_ptr, float* x, int64_t M, int B, int N,
                                      int F, gcm_stream_t stream) {
  GCM_REQUIRE(node_ptr && x && M >= 0 && B > 0 && N > 0 && F > 0);
  GCM_REQUIRE(M == 0 || x_sp);
  const int64_t total = (int64_t)B * N * F;
  const unsigned grid = blocks_of(total);
  if (!grid) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_bridge_dense_nodes, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, x_sp, node_ptr, x, M,
                     total, N, F);
  return gcm_launch_status();
}

extern "C" int gcm_bridge_dense_nodes_bwd(const float* g_x, const int64_t* batch_idx, const int64_t* node_ptr,
                                          float* g_x_sp, int64_t M, int B, int N, int F, gcm_stream_t stream) {
  GCM_REQUIRE(M >= 0 && B > 0 && N > 0 && F > 0);
  GCM_REQUIRE(M == 0 || (g_x && batch_idx && node_ptr && g_x_sp));
  if (M == 0) return GCM_OK;
  const int64_t total = M * F;
  const unsigned grid = blocks_of(total);
  if (!grid) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_bridge_dense_nodes_bwd, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g_x, batch_idx,
                     node_ptr, g_x_sp, total, B, N, F);
  return gcm_launch_status();
}

extern "C" int gcm_bridge_dense_adj(const int64_t* row_ptr, const int64_t* csr_perm, const int64_t* edge_index,
                                    const float* edge_weight, const int64_t* batch_idx, const int64_t* node_ptr,
                                    float* adj, int64_t M, int64_t E, int B, int N, gcm_stream_t stream) {
  GCM_REQUIRE(adj && M >= 0 && E >= 0 && B > 0 && N > 0);
  GCM_REQUIRE(E == 0 || (row_ptr && edge_index && batch_idx && node_ptr && M > 0));
  const hipError_t e = hipMemsetAsync(adj, 0, sizeof(float) * (size_t)B * N * N, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  if (E == 0) return GCM_OK;
  const unsigned grid = blocks_of(M);
  if (!grid) return GCM_EUNSUPPORTED;
  return gcm_pick(
      [&](auto pm, auto wt) {
        hipLaunchKernelGGL((k_bridge_dense_adj<bool(pm()), bool(wt())>), dim3(grid), dim3(kThreads), 0,
                           (hipStream_t)stream, row_ptr, csr_perm, edge_index, edge_weight, batch_idx, node_ptr, adj,
                           M, E, B, N);
        return gcm_launch_status();
      },
      Flag{csr_perm != nullptr}, Flag{edge_weight != nullptr});
}

extern "C" int gcm_bridge_dense_adj_bwd(const float* g_adj, const int64_t* edge_index, const int64_t* batch_idx,
                                        const int64_t* node_ptr, float* g_weight, int64_t M, int64_t E, int B, int N,
                                        gcm_stream_t stream) {
  GCM_REQUIRE(M >= 0 && E >= 0 && B > 0 && N > 0);
  GCM_REQUIRE(E == 0 || (g_adj && edge_index && batch_idx && node_ptr && g_weight && M > 0));
  if (E == 0) return GCM_OK;
  const unsigned grid = blocks_of(E);
  if (!grid) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_bridge_dense_adj_bwd, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, g_adj, edge_index,
                     batch_idx, node_ptr, g_weight, M, E, B, N);
  return gcm_launch_status();
}
