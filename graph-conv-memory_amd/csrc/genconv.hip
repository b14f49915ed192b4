// GENConv / DenseGENConv (DeeperGCN's softmax aggregation; PyG's GENConv, aggr="softmax"): the aggregation and its
// gradients on gfx950.  lin_src / lin_dst, the message norm and the mlp are torch modules on top; what is here is
//
//   m_jc   = relu(xs_jc) + eps
//   agg_ic = sum over the set entries j of row i of a_ijc m_jc,   a_ijc = softmax over those j of (t m_jc)
//   g_m_jc = sum over the rows i that hold j of g_ic a_ijc (1 + t (m_jc - agg_ic)),   g_xs = g_m [xs > 0]
//   g_t    = sum over (i, c) of g_ic (sum_j a_ijc m_jc^2 - agg_ic^2)
//
// The set entries of row i are adj[b,i,:] != 0 (dense: the pattern alone is read) or the CSR segment of i (duplicates
// count once each).  t [1] is read from its device pointer inside the kernels: no host read, so the calls stay
// HIP-graph capturable.
//
// Lanes over channels, so the loads of xs / g / agg are contiguous.  CSR: one thread per (row, channel), the column
// index is the same address for the lanes of a row.  Dense: one wave per row; 64 entries of the adjacency row are one
// coalesced load, a ballot turns them into a bit mask, and the wave walks the set bits only.  The masks are written
// out (bits [B*N, ceil(N/64)], 1/32 of the adjacency): the backward reads the transposed pattern from them - a lane
// per row, the word that holds column j, one ballot - instead of walking adj by columns.
//
// The forward is ONE pass over a row's entries with a running max, sum and weighted sum (online softmax); the shift is
// the row's own maximum, so logits of any size and neighbourhoods far below the largest logit of their graph are
// exact.  It saves agg and the log-sum-exp in its two parts, the maximum and the shifted sum (lse = max + log sum):
// the backward forms a weight as exp(t m - max) / sum, with no large logit cancelled against a large log-sum-exp and
// no rounding of a log.  No per-edge weight is stored.  t m - max is one fma, so the rounding of the maximum itself is
// a common factor of a row's terms and cancels in the quotient.
//
// The backward for xs is a column sweep (dense: the bit masks; CSR: the CSC by source) that recomputes a_ijc from the
// saved statistics: a gather, no float atomics.  g_t: every (i, c) forms its term in a second row sweep with the row's
// moments in fp64, fp64 partial sums over fixed ranges go to the workspace and one workgroup adds them in a fixed
// order.  Every sum has one order: results are bitwise reproducible.  C <= 128.
#include <algorithm>

#include "fixed_sum.h"

namespace {

constexpr int TPB = 256;
constexpr int WPB = TPB / 64;  // dense: waves = rows per workgroup
constexpr int SLOTS = 2;       // dense: channels lane, lane + 64 (C <= 128)

__device__ __forceinline__ float gen_msg(float xs, float eps) { return fmaxf(xs, 0.f) + eps; }

// the running statistics of one (row, channel)
struct Online {
  float M = -INFINITY, S = 0.f, W = 0.f;
  __device__ __forceinline__ void add(float m, float t) {
    const float l = __fmul_rn(t, m);
    if (l > M) {  // a new maximum: what was summed so far moves to the new shift (exp(-inf) = 0 at the first entry)
      const float r = expf(M - l);
      S *= r;
      W *= r;
      M = l;
    }
    const float p = expf(fmaf(t, m, -M));
    S += p;
    W = fmaf(p, m, W);
  }
  __device__ __forceinline__ void store(float* agg, float* mx, float* sum) const {
    const bool any = S > 0.f;  // the maximum's own term is exp(~0): S >= ~1 for a row with entries
    *agg = any ? W / S : 0.f;
    *mx = any ? M : 0.f;
    *sum = any ? S : 1.f;
  }
};

// a_ijc from the saved statistics of (i, c)
__device__ __forceinline__ float gen_alpha(float t, float m, float mx, float sum) {
  return expf(fmaf(t, m, -mx)) / sum;
}

// one term of g_m_jc, o = i * C + c
__device__ __forceinline__ float gen_gm_term(float acc, float t, float m, int64_t o, int64_t L,
                                             const float* __restrict__ g, const float* __restrict__ agg,
                                             const float* __restrict__ lse) {
  const float a = gen_alpha(t, m, lse[o], lse[L + o]);
  return fmaf(g[o] * a, fmaf(t, m - agg[o], 1.f), acc);
}

// the moments of one (row, channel) for g_t, in fp64 from the fp32 messages, shifted by the saved maximum (the
// difference of the two squares would cancel in fp32, and one scalar collects the rounding of every (i, c): a weight
// good to 1e-7 is not good enough)
struct Moments {
  double S = 0.0, W = 0.0, Q = 0.0;
  __device__ __forceinline__ void add(double m, double t, double mx) {
    const double p = exp(fma(t, m, -mx));
    S += p;
    W = fma(p, m, W);
    Q = fma(p * m, m, Q);
  }
  __device__ __forceinline__ double variance() const {
    if (!(S > 0.0)) return 0.0;
    const double mean = W / S;
    return Q / S - mean * mean;
  }
};

// ---------------------------------------------------------------------------
// dense: one wave per row
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_gen_dense_fwd(const float* __restrict__ xs, const float* __restrict__ adj,
                                                       const float* __restrict__ t_ptr, float eps,
                                                       float* __restrict__ agg, float* __restrict__ lse,
                                                       int64_t* __restrict__ bits, int64_t rows, int N, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (i >= rows) return;  // the whole wave
  const int64_t L = rows * C, base = i / N * N;
  const int W64 = (N + 63) >> 6;
  const float t = t_ptr[0];
  const float* arow = adj + i * N;
  Online st[SLOTS];
  for (int k0 = 0, w = 0; k0 < N; k0 += 64, ++w) {
    const int k = k0 + lane;
    const float v = k < N ? arow[k] : 0.f;
    unsigned long long mask = __ballot(v != 0.f);
    if (lane == 0) bits[i * W64 + w] = (int64_t)mask;
    while (mask) {
      const float* xr = xs + (base + k0 + gcm_first_bit(mask)) * C;
      mask &= mask - 1;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int c = lane + 64 * s;
        if (c < C) st[s].add(gen_msg(xr[c], eps), t);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c = lane + 64 * s;
    const int64_t e = i * C + c;
    if (c < C) st[s].store(agg + e, lse + e, lse + L + e);
  }
}

// g_xs of source row j: the rows i of its graph whose mask holds bit j, 64 rows per ballot, in ascending order
__global__ __launch_bounds__(TPB) void k_gen_dense_bwd_x(const float* __restrict__ g, const float* __restrict__ xs,
                                                         const int64_t* __restrict__ bits,
                                                         const float* __restrict__ t_ptr, float eps,
                                                         const float* __restrict__ agg,
                                                         const float* __restrict__ lse, float* __restrict__ g_xs,
                                                         int64_t rows, int N, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  if (j >= rows) return;  // the whole wave
  const int64_t L = rows * C, b0 = j / N * N;
  const int jl = (int)(j - b0), W64 = (N + 63) >> 6;
  const int word = jl >> 6, bit = jl & 63;
  const float t = t_ptr[0];
  float x[SLOTS], m[SLOTS], acc[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c = lane + 64 * s;
    x[s] = c < C ? xs[j * C + c] : 0.f;
    m[s] = gen_msg(x[s], eps);
    acc[s] = 0.f;
  }
  for (int k0 = 0; k0 < N; k0 += 64) {
    const int k = k0 + lane;
    const unsigned long long u = k < N ? (unsigned long long)bits[(b0 + k) * W64 + word] : 0ull;
    unsigned long long mask = __ballot((int)((u >> bit) & 1ull));
    while (mask) {
      const int64_t i = b0 + k0 + gcm_first_bit(mask);
      mask &= mask - 1;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int c = lane + 64 * s;
        if (c < C) acc[s] = gen_gm_term(acc[s], t, m[s], i * C + c, L, g, agg, lse);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c = lane + 64 * s;
    if (c < C) g_xs[j * C + c] = x[s] > 0.f ? acc[s] : 0.f;
  }
}

// g_t, pass 1: part[blk] = sum over the rows [blk * WPB * r, (blk + 1) * WPB * r) - r consecutive rows per wave - and
// their channels of g_ic (sum_j a_ijc m_jc^2 - (sum_j a_ijc m_jc)^2), threads combined in a fixed order
__global__ __launch_bounds__(TPB) void k_gen_dense_gt_parts(const float* __restrict__ g, const float* __restrict__ xs,
                                                            const int64_t* __restrict__ bits,
                                                            const float* __restrict__ t_ptr, float eps,
                                                            const float* __restrict__ lse, int64_t rows, int N, int C,
                                                            int r, double* __restrict__ part) {
  __shared__ double sp[TPB];
  const int lane = threadIdx.x & 63;
  const int W64 = (N + 63) >> 6;
  const double t = (double)t_ptr[0];
  const int64_t i0 = ((int64_t)blockIdx.x * WPB + (threadIdx.x >> 6)) * r;
  const int64_t i1 = min(rows, i0 + r);
  double sum = 0.0;
  for (int64_t i = i0; i < i1; ++i) {
    const int64_t base = i / N * N;
    Moments mo[SLOTS];
    double mx[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c = lane + 64 * s;
      mx[s] = c < C ? (double)lse[i * C + c] : 0.0;
    }
    for (int w = 0; w < W64; ++w) {
      unsigned long long mask = (unsigned long long)bits[i * W64 + w];  // the same word for the whole wave
      while (mask) {
        const float* xr = xs + (base + 64 * w + gcm_first_bit(mask)) * C;
        mask &= mask - 1;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
          const int c = lane + 64 * s;
          if (c < C) mo[s].add((double)gen_msg(xr[c], eps), t, mx[s]);
        }
      }
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c = lane + 64 * s;
      if (c < C) sum += (double)g[i * C + c] * mo[s].variance();
    }
  }
  const double total = block_sum(sum, sp);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// ---------------------------------------------------------------------------
// CSR: one thread per (row, channel)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_gen_csr_fwd(const float* __restrict__ xs,
                                                     const int64_t* __restrict__ row_ptr,
                                                     const int64_t* __restrict__ col,
                                                     const float* __restrict__ t_ptr, float eps,
                                                     float* __restrict__ agg, float* __restrict__ lse, int64_t M,
                                                     int C) {
  const int64_t L = M * C;
  const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (e >= L) return;
  const int64_t i = e / C;
  const int c = (int)(e - i * C);
  const float t = t_ptr[0];
  Online st;
  if (row_ptr) {
    const int64_t k1 = row_ptr[i + 1];
    for (int64_t k = row_ptr[i]; k < k1; ++k) st.add(gen_msg(xs[col[k] * C + c], eps), t);
  }
  st.store(agg + e, lse + e, lse + L + e);
}

// g_xs at e = row j * C + c: the sweep over the CSC column of j (the sinks of j's out-edges)
__global__ __launch_bounds__(TPB) void k_gen_csr_bwd_x(const float* __restrict__ g, const float* __restrict__ xs,
                                                       const int64_t* __restrict__ col_ptr,
                                                       const int64_t* __restrict__ rws,
                                                       const float* __restrict__ t_ptr, float eps,
                                                       const float* __restrict__ agg, const float* __restrict__ lse,
                                                       float* __restrict__ g_xs, int64_t M, int C) {
  const int64_t L = M * C;
  const int64_t e = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (e >= L) return;
  const int64_t j = e / C;
  const int c = (int)(e - j * C);
  const float t = t_ptr[0];
  const float x = xs[e];
  const float m = gen_msg(x, eps);
  float acc = 0.f;
  if (col_ptr) {
    const int64_t k1 = col_ptr[j + 1];
    for (int64_t k = col_ptr[j]; k < k1; ++k) acc = gen_gm_term(acc, t, m, rws[k] * C + c, L, g, agg, lse);
  }
  g_xs[e] = x > 0.f ? acc : 0.f;
}

// g_t, pass 1: part[blk] = sum over the block's element range [blk * chunk, (blk + 1) * chunk) of
// g_ic (sum_j a_ijc m_jc^2 - (sum_j a_ijc m_jc)^2), threads combined in a fixed order
__global__ __launch_bounds__(TPB) void k_gen_csr_gt_parts(const float* __restrict__ g, const float* __restrict__ xs,
                                                          const int64_t* __restrict__ row_ptr,
                                                          const int64_t* __restrict__ col,
                                                          const float* __restrict__ t_ptr, float eps,
                                                          const float* __restrict__ lse, int64_t M, int C,
                                                          int64_t chunk, double* __restrict__ part) {
  __shared__ double sp[TPB];
  const int64_t L = M * C;
  const int64_t e0 = (int64_t)blockIdx.x * chunk;
  const int64_t e1 = min(L, e0 + chunk);
  const double t = (double)t_ptr[0];
  double sum = 0.0;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += TPB) {
    const int64_t i = e / C;
    const int c = (int)(e - i * C);
    const double mx = (double)lse[e];
    Moments mo;
    if (row_ptr) {
      const int64_t k1 = row_ptr[i + 1];
      for (int64_t k = row_ptr[i]; k < k1; ++k) mo.add((double)gen_msg(xs[col[k] * C + c], eps), t, mx);
    }
    sum += (double)g[e] * mo.variance();
  }
  const double total = block_sum(sum, sp);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// the g_t partials: at most GT_BLOCKS of them
constexpr int GT_BLOCKS = 4096;

// CSR: element ranges, a multiple of the workgroup
void csr_gt_plan(int64_t L, int* nblocks, int64_t* chunk) {
  int64_t c = (L + GT_BLOCKS - 1) / GT_BLOCKS;
  c = std::max<int64_t>((c + TPB - 1) / TPB * TPB, TPB);
  *chunk = c;
  *nblocks = (int)((L + c - 1) / c);
}

// dense: r consecutive rows per wave
void dense_gt_plan(int64_t rows, int* nblocks, int* r) {
  const int64_t per = std::max<int64_t>((rows + (int64_t)WPB * GT_BLOCKS - 1) / ((int64_t)WPB * GT_BLOCKS), 1);
  *r = (int)per;
  *nblocks = (int)((rows + WPB * per - 1) / (WPB * per));
}

size_t parts_bytes(int n) { return ((size_t)n * sizeof(double) + 255) / 256 * 256; }

size_t csr_gt_ws_bytes(int64_t L) {
  int n;
  int64_t c;
  csr_gt_plan(L, &n, &c);
  return parts_bytes(n);
}

size_t dense_gt_ws_bytes(int64_t rows) {
  int n, r;
  dense_gt_plan(rows, &n, &r);
  return parts_bytes(n);
}

unsigned grid_of(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

bool too_large(int64_t rows, int C) { return C > 64 * SLOTS || rows > (1 << 30); }

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: DenseGENConv
// ---------------------------------------------------------------------------
extern "C" int gcm_dense_gen_fwd(const float* xs, const float* adj, const float* t, float eps, float* agg, float* lse,
                                 int64_t* bits, int B, int N, int C, gcm_stream_t stream) {
  GCM_REQUIRE(xs && adj && t && agg && lse && bits);
  GCM_REQUIRE(B > 0 && N > 0 && C > 0);
  const int64_t rows = (int64_t)B * N;
  if (too_large(rows, C)) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_gen_dense_fwd, dim3(grid_of(rows, WPB)), dim3(TPB), 0, (hipStream_t)stream, xs, adj, t, eps,
                     agg, lse, bits, rows, N, C);
  return gcm_launch_status();
}

extern "C" size_t gcm_dense_gen_bwd_workspace_bytes(int B, int N, int C) {
  if (B <= 0 || N <= 0 || C <= 0) return 0;
  return dense_gt_ws_bytes((int64_t)B * N);
}

extern "C" int gcm_dense_gen_bwd(const float* g_agg, const float* xs, const int64_t* bits, const float* t, float eps,
                                 const float* agg, const float* lse, float* g_xs, float* g_t, void* workspace,
                                 size_t workspace_bytes, int B, int N, int C, gcm_stream_t stream) {
  GCM_REQUIRE(g_agg && xs && bits && t && agg && lse);
  GCM_REQUIRE(B > 0 && N > 0 && C > 0);
  const int64_t rows = (int64_t)B * N;
  if (too_large(rows, C)) return GCM_EUNSUPPORTED;
  GCM_REQUIRE(!g_t || (workspace && workspace_bytes >= dense_gt_ws_bytes(rows)));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (g_xs) {
    hipLaunchKernelGGL(k_gen_dense_bwd_x, dim3(grid_of(rows, WPB)), dim3(TPB), 0, s, g_agg, xs, bits, t, eps, agg, lse,
                       g_xs, rows, N, C);
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_t) {
    int n, r;
    dense_gt_plan(rows, &n, &r);
    double* part = (double*)workspace;
    hipLaunchKernelGGL(k_gen_dense_gt_parts, dim3(n), dim3(TPB), 0, s, g_agg, xs, bits, t, eps, lse, rows, N, C, r,
                       part);
    if ((rc = gcm_launch_status())) return rc;
    if ((rc = sum_parts(part, n, g_t, s))) return rc;
  }
  return GCM_OK;
}

// ---------------------------------------------------------------------------
// C ABI: GENConv
// ---------------------------------------------------------------------------
extern "C" int gcm_csr_gen_fwd(const float* xs, const int64_t* row_ptr, const int64_t* col, const float* t, float eps,
                               float* agg, float* lse, int64_t M, int64_t E, int C, gcm_stream_t stream) {
  GCM_REQUIRE(xs && row_ptr && t && agg && lse);
  GCM_REQUIRE(M > 0 && E >= 0 && C > 0);
  GCM_REQUIRE(E == 0 || col);
  if (too_large(M, C)) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_gen_csr_fwd, dim3(grid_of(M * C, TPB)), dim3(TPB), 0, (hipStream_t)stream, xs,
                     E > 0 ? row_ptr : nullptr, col, t, eps, agg, lse, M, C);
  return gcm_launch_status();
}

extern "C" size_t gcm_csr_gen_bwd_workspace_bytes(int64_t M, int64_t E, int C) {
  if (M <= 0 || E < 0 || C <= 0) return 0;
  return csr_gt_ws_bytes(M * C);
}

extern "C" int gcm_csr_gen_bwd(const float* g_agg, const float* xs, const float* t, float eps, const float* agg,
                               const float* lse, const int64_t* row_ptr, const int64_t* col, const int64_t* col_ptr,
                               const int64_t* rows, float* g_xs, float* g_t, void* workspace, size_t workspace_bytes,
                               int64_t M, int64_t E, int C, gcm_stream_t stream) {
  GCM_REQUIRE(g_agg && xs && t && agg && lse);
  GCM_REQUIRE(M > 0 && E >= 0 && C > 0);
  GCM_REQUIRE(E == 0 || !g_xs || (col_ptr && rows));
  GCM_REQUIRE(E == 0 || !g_t || (row_ptr && col));
  if (too_large(M, C)) return GCM_EUNSUPPORTED;
  const int64_t L = M * C;
  GCM_REQUIRE(!g_t || (workspace && workspace_bytes >= csr_gt_ws_bytes(L)));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (g_xs) {
    hipLaunchKernelGGL(k_gen_csr_bwd_x, dim3(grid_of(L, TPB)), dim3(TPB), 0, s, g_agg, xs, E > 0 ? col_ptr : nullptr,
                       rows, t, eps, agg, lse, g_xs, M, C);
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_t) {
    int n;
    int64_t chunk;
    csr_gt_plan(L, &n, &chunk);
    double* part = (double*)workspace;
    hipLaunchKernelGGL(k_gen_csr_gt_parts, dim3(n), dim3(TPB), 0, s, g_agg, xs, E > 0 ? row_ptr : nullptr, col, t, eps,
                       lse, M, C, chunk, part);
    if ((rc = gcm_launch_status())) return rc;
    if ((rc = sum_parts(part, n, g_t, s))) return rc;
  }
  return GCM_OK;
}
