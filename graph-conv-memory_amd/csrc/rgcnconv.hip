// RGCNConv / DenseRGCNConv (Schlichtkrull et al.; PyG's RGCNConv) and TypedEdge's merge on gfx950.
//
//   out_i = sum_r s_r(i) sum_j m_r(i,j) a(i,j) x_j W_r  +  x_i root  +  bias
//
// m_r: bit r of the relation code of the entry (dense: the plane `rel`, a float32 holding an integer; sparse: one
// code per edge), a: the adjacency value (sparse: 1), s_r(i) = 1 / max(1, #{j: m_r(i,j)}) for the mean, 1 for the sum.
//
// Transform first: Y_r = X W_r for every relation in one batched k_gcn_mm launch, x root + bias as a second, then
// ONE aggregation launch over K = R N whose A-loader returns m_r(i,j) a(i,j) s_r(i) - a coefficient that is exactly 0
// where the bit is not set, whatever the adjacency holds there - and adds the root term in its epilogue.  Every K
// tile of 32 starts from a zero accumulator (gcn_mm.h's rule: no fp32 chain over 32 products).  The sparse layer
// gathers the same Y over the destination CSR, one thread per output element, in chunks of 32 edges.
//
// Backward: H_r = C_r^T g (dense: one tile GEMM per (graph, relation), the planes read transposed; sparse: a gather
// over the CSC by source), then for both layers g_x = [H_0 .. H_{R-1} g] [W_0 .. W_{R-1} root]^T as one tile GEMM over
// K = (R + 1) Fo, g_W = X^T H_r for all relations as one batched split-K launch summed slab by slab, g_root and g_bias
// by gcn_mm.h's wgrad and colsum.  Dense g_adj(i,j) = sum_r m_r(i,j) s_r(i) <g_i, Y_r(j)>: one tile product per
// relation, masked in registers.  No atomics anywhere: bitwise reproducible.  Fi, Fo <= 128, R <= 16.
#include "gcn_mm.h"

namespace {

constexpr int MAX_R = 16;
constexpr int MAX_F = 128;

// the relation code of a plane entry: the integer it holds when positive (exact below 2^24), else none
__device__ __forceinline__ unsigned rel_code(float v) {
  return v > 0.f ? (unsigned)((long long)fminf(v, 9.0e18f) & 0xFFFFFF) : 0u;
}

// the relation code of an edge: its bit code (mask_mode) or the one bit of its relation id (none outside [0, R))
__device__ __forceinline__ unsigned edge_code(int64_t t, int R, int mask_mode) {
  const unsigned all = (1u << R) - 1u;
  if (mask_mode) return t > 0 ? (unsigned)(t & 0xFFFF) & all : 0u;
  return (t >= 0 && t < R) ? 1u << (int)t : 0u;
}

// ---------------------------------------------------------------------------
// dense
// ---------------------------------------------------------------------------
// scale[b, r, i] = 1 / max(1, #{j: bit r of rel[b,i,j]});  one wave per row, the counts by ballot
__global__ __launch_bounds__(256) void k_rgcn_dense_scale(const float* __restrict__ rel, float* __restrict__ scale,
                                                          int64_t rows, int N, int R) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const float* rp = rel + (size_t)row * N;
  int cnt[MAX_R];
#pragma unroll
  for (int r = 0; r < MAX_R; ++r) cnt[r] = 0;
  for (int j0 = 0; j0 < N; j0 += 64) {
    const int j = j0 + lane;
    const unsigned code = j < N ? rel_code(rp[j]) : 0u;
#pragma unroll
    for (int r = 0; r < MAX_R; ++r) cnt[r] += __popcll(__ballot((code >> r) & 1u));
  }
  const int64_t b = row / N;
  const int i = (int)(row - b * N);
#pragma unroll
  for (int r = 0; r < MAX_R; ++r)
    if (r < R && lane == r) scale[((size_t)b * R + r) * N + i] = 1.f / (float)max(1, cnt[r]);
}

// out(b,i,:) = sum over gk = (r, j) of coef_r(b,i,j) Y_r(b,j,:)  (+ out(b,i,:) when accumulate, else + bias)
template <int NCT>
__global__ __launch_bounds__(256) void k_rgcn_dense_fwd(const float* __restrict__ adj, const float* __restrict__ rel,
                                                        const float* __restrict__ scale, const float* __restrict__ Y,
                                                        const float* __restrict__ bias, float* __restrict__ out, int N,
                                                        int Fo, int R, int64_t y_rs, int accumulate) {
  __shared__ float sA[MB * (KT + 1)];        // [i][k]
  __shared__ float sB[KT * (32 * NCT + 1)];  // [k][f]
  const int b = blockIdx.z;
  const int i0 = blockIdx.x * MB;
  const TileLane t = tile_lane();
  const float* Ab = adj + (size_t)b * N * N;
  const float* Rb = rel + (size_t)b * N * N;
  const float* Sb = scale ? scale + (size_t)b * R * N : nullptr;
  const float* Yb = Y + (size_t)b * N * Fo;
  float* Ob = out + (size_t)b * N * Fo;
  f32x16 acc[NCT];
  tile_zero(acc);
  tile_mma<NCT, true>(
      acc, t, sA, sB, i0, 0, N, Fo, 0, R * N, false, false,
      [=](int gi, int gk) {
        const int r = gk / N, j = gk - r * N;
        const size_t o = (size_t)gi * N + j;
        if (!((rel_code(Rb[o]) >> r) & 1u)) return 0.f;
        const float a = Ab[o];
        return Sb ? a * Sb[(size_t)r * N + gi] : a;
      },
      [=](int gk, int gj) {
        const int r = gk / N, j = gk - r * N;
        return Yb[(size_t)r * y_rs + (size_t)j * Fo + gj];
      });
  tile_store(acc, t, i0, 0, N, Fo, [=](int j) {
    const float bj = (!accumulate && bias) ? bias[j] : 0.f;
    return [=](int i, float v) {
      const size_t off = (size_t)i * Fo + j;
      Ob[off] = accumulate ? Ob[off] + v : v + bj;
    };
  });
}

// H_r(b,j,:) = sum_i coef_r(b,i,j) g(b,i,:);  blockIdx.z = b R + r
template <int NCT>
__global__ __launch_bounds__(256) void k_rgcn_dense_aggT(const float* __restrict__ adj, const float* __restrict__ rel,
                                                         const float* __restrict__ scale, const float* __restrict__ g,
                                                         float* __restrict__ H, int N, int Fo, int R, int64_t h_rs) {
  __shared__ float sA[MB * (KT + 1)];        // [j][i]
  __shared__ float sB[KT * (32 * NCT + 1)];  // [i][f]
  const int b = blockIdx.z / R, r = blockIdx.z - b * R;
  const int j0 = blockIdx.x * MB;
  const TileLane t = tile_lane();
  const float* Ab = adj + (size_t)b * N * N;
  const float* Rb = rel + (size_t)b * N * N;
  const float* Sr = scale ? scale + ((size_t)b * R + r) * N : nullptr;
  const float* Gb = g + (size_t)b * N * Fo;
  float* Hb = H + (size_t)r * h_rs + (size_t)b * N * Fo;
  f32x16 acc[NCT];
  tile_zero(acc);
  tile_mma<NCT, true>(
      acc, t, sA, sB, j0, 0, N, Fo, 0, N, true, false,  // the row of the tile (j) is the fast index in memory
      [=](int gj, int gi) {
        const size_t o = (size_t)gi * N + gj;
        if (!((rel_code(Rb[o]) >> r) & 1u)) return 0.f;
        const float a = Ab[o];
        return Sr ? a * Sr[gi] : a;
      },
      [=](int gi, int gf) { return Gb[(size_t)gi * Fo + gf]; });
  tile_store(acc, t, j0, 0, N, Fo,
             [=](int f) { return [=](int j, float v) { Hb[(size_t)j * Fo + f] = v; }; });
}

// g_adj(b,i,j) = sum_r bit_r(rel(b,i,j)) s_r(b,i) <g(b,i,:), Y_r(b,j,:)>
template <int NCT>
__global__ __launch_bounds__(256) void k_rgcn_dense_gadj(const float* __restrict__ rel,
                                                         const float* __restrict__ scale, const float* __restrict__ g,
                                                         const float* __restrict__ Y, float* __restrict__ g_adj, int N,
                                                         int Fo, int R, int64_t y_rs) {
  __shared__ float sA[MB * (KT + 1)];        // [i][f]
  __shared__ float sB[KT * (32 * NCT + 1)];  // [f][j]
  const int b = blockIdx.z;
  const int i0 = blockIdx.x * MB, j0 = blockIdx.y * 32 * NCT;
  const TileLane t = tile_lane();
  const float* Rb = rel + (size_t)b * N * N;
  const float* Sb = scale ? scale + (size_t)b * R * N : nullptr;
  const float* Gb = g + (size_t)b * N * Fo;
  const float* Yb = Y + (size_t)b * N * Fo;
  unsigned code[NCT][16];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int i = i0 + t.wave * 32 + acc_row(e, t.lh), j = j0 + c * 32 + t.li;
      code[c][e] = (i < N && j < N) ? rel_code(Rb[(size_t)i * N + j]) : 0u;
    }
  f32x16 tot[NCT];
  tile_zero(tot);
  for (int r = 0; r < R; ++r) {
    const float* Yr = Yb + (size_t)r * y_rs;
    f32x16 acc[NCT];
    tile_zero(acc);
    tile_mma<NCT, true>(
        acc, t, sA, sB, i0, j0, N, N, 0, Fo, false, true,
        [=](int gi, int gf) { return Gb[(size_t)gi * Fo + gf]; },
        [=](int gf, int gj) { return Yr[(size_t)gj * Fo + gf]; });
#pragma unroll
    for (int c = 0; c < NCT; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        if (!((code[c][e] >> r) & 1u)) continue;
        const int i = i0 + t.wave * 32 + acc_row(e, t.lh);
        tot[c][e] += Sb ? Sb[(size_t)r * N + i] * acc[c][e] : acc[c][e];
      }
  }
  float* Cb = g_adj + (size_t)b * N * N;
  tile_store(tot, t, i0, j0, N, N, [=](int j) { return [=](int i, float v) { Cb[(size_t)i * N + j] = v; }; });
}

// ---------------------------------------------------------------------------
// shared by both layers
// ---------------------------------------------------------------------------
// g_x(i,:) = sum_r H_r(i,:) W_r^T + g(i,:) root^T  as one product over K = (R + has_root) Fo;  W [R,Fi,Fo], root [Fi,Fo]
template <int NCT>
__global__ __launch_bounds__(256) void k_rgcn_gx(const float* __restrict__ H, const float* __restrict__ g,
                                                 const float* __restrict__ W, const float* __restrict__ root,
                                                 float* __restrict__ g_x, int rows, int Fi, int Fo, int R,
                                                 int64_t h_rs) {
  __shared__ float sA[MB * (KT + 1)];        // [i][k]
  __shared__ float sB[KT * (32 * NCT + 1)];  // [k][fi]
  const int i0 = blockIdx.x * MB;
  const TileLane t = tile_lane();
  const int K = (R + (root ? 1 : 0)) * Fo;
  f32x16 acc[NCT];
  tile_zero(acc);
  tile_mma<NCT, true>(
      acc, t, sA, sB, i0, 0, rows, Fi, 0, K, false, true,
      [=](int gi, int gk) {
        const int r = gk / Fo, f = gk - r * Fo;
        return r < R ? H[(size_t)r * h_rs + (size_t)gi * Fo + f] : g[(size_t)gi * Fo + f];
      },
      [=](int gk, int gj) {
        const int r = gk / Fo, f = gk - r * Fo;
        return r < R ? W[((size_t)r * Fi + gj) * Fo + f] : root[(size_t)gj * Fo + f];
      });
  tile_store(acc, t, i0, 0, rows, Fi,
             [=](int j) { return [=](int i, float v) { g_x[(size_t)i * Fi + j] = v; }; });
}

__global__ __launch_bounds__(256) void k_rgcn_zero(float* __restrict__ p, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) p[e] = 0.f;
}

// Y_r = X W_r, every relation in one launch:  Y [R, rows, Fo]
int transform(const float* x, const float* W, float* Y, int64_t rows, int Fi, int Fo, int R, hipStream_t s) {
  MmArgs p = mm_args();
  p.A = x, p.a_bs = 0, p.a_is = Fi, p.a_ks = 1;
  p.B = W, p.b_bs = (int64_t)Fi * Fo, p.b_ks = Fo, p.b_js = 1;
  p.C = Y, p.c_bs = rows * Fo, p.c_is = Fo, p.c_js = 1;
  p.M = (int)rows, p.N = Fo, p.K = Fi, p.batch = R;
  return launch_mm(p, 1, s);
}

// out = x root + bias
int root_term(const float* x, const float* root, const float* bias, float* out, int64_t rows, int Fi, int Fo,
              hipStream_t s) {
  MmArgs p = mm_args();
  p.A = x, p.a_is = Fi, p.a_ks = 1;
  p.B = root, p.b_ks = Fo, p.b_js = 1;
  p.C = out, p.c_is = Fo, p.c_js = 1, p.c_bias = bias;
  p.M = (int)rows, p.N = Fo, p.K = Fi;
  return launch_mm(p, 1, s);
}

size_t slab_floats(int64_t rows, int Fi, int Fo, int R) {
  int nsplit, kchunk;
  wgrad_split64(rows, &nsplit, &kchunk);
  return std::max((size_t)nsplit * R * Fi * Fo, (size_t)colsum_slabs(rows) * Fo);
}

// what both backwards do once H is there: g_x, g_W, g_root, g_bias (each may be NULL).  The slab region is used by
// one reduction after the other (stream order).
int param_grads(const float* g, const float* x, const float* H, const float* W, const float* root, float* g_x,
                float* g_W, float* g_root, float* g_bias, float* slabs, int64_t rows, int Fi, int Fo, int R,
                hipStream_t s) {
  int rc;
  const int64_t h_rs = rows * Fo;
  if (g_x) {
    dispatch_nct(nct_of(Fi), [&](auto n) {
      hipLaunchKernelGGL(k_rgcn_gx<n()>, dim3(blocks(rows, MB)), dim3(256), 0, s, H, g, W, root, g_x, (int)rows, Fi, Fo,
                         R, h_rs);
    });
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_W) {  // g_W[r] = X^T H_r: split-K slabs of all relations, then one ordered sum
    int nsplit, kchunk;
    wgrad_split64(rows, &nsplit, &kchunk);
    MmArgs p = mm_args();
    p.A = x, p.a_bs = 0, p.a_is = 1, p.a_ks = Fi;
    p.B = H, p.b_bs = h_rs, p.b_ks = Fo, p.b_js = 1;
    p.C = slabs, p.c_bs = (int64_t)Fi * Fo, p.c_is = Fo, p.c_js = 1, p.c_ss = (int64_t)R * Fi * Fo;
    p.M = Fi, p.N = Fo, p.K = (int)rows, p.batch = R, p.kchunk = kchunk;
    if ((rc = launch_mm(p, nsplit, s))) return rc;
    if ((rc = gcm_sum_slabs(slabs, nsplit, R * Fi * Fo, g_W, s))) return rc;
  }
  if (g_root && (rc = wgrad(x, g, g_root, slabs, rows, Fo, Fi, s, wgrad_split64))) return rc;  // X^T g: [Fi, Fo]
  if (g_bias && (rc = colsum(g, rows, Fo, g_bias, slabs, s))) return rc;
  return GCM_OK;
}

bool widths_ok(int Fi, int Fo, int R) { return Fi <= MAX_F && Fo <= MAX_F && R <= MAX_R; }

// ---------------------------------------------------------------------------
// sparse
// ---------------------------------------------------------------------------
// scale[i, r] = 1 / max(1, #{entries of CSR row i with bit r})
__global__ __launch_bounds__(256) void k_rgcn_csr_scale(const int64_t* __restrict__ ptr,
                                                        const int64_t* __restrict__ et, float* __restrict__ scale,
                                                        int64_t M, int R, int mask_mode) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * R) return;
  const int64_t i = t / R;
  const int r = (int)(t - i * R);
  int cnt = 0;
  if (ptr) {
    const int64_t k1 = ptr[i + 1];
    for (int64_t k = ptr[i]; k < k1; ++k) cnt += (edge_code(et[k], R, mask_mode) >> r) & 1u;
  }
  scale[t] = 1.f / (float)max(1, cnt);
}

// out[i,f] (+)= sum over the CSR row i and the bits r of each entry of s_r(i) Y_r[col,f], in chunks of 32 entries
__global__ __launch_bounds__(256) void k_rgcn_csr_fwd(const float* __restrict__ Y, const int64_t* __restrict__ ptr,
                                                      const int64_t* __restrict__ col,
                                                      const int64_t* __restrict__ et, const float* __restrict__ scale,
                                                      const float* __restrict__ bias, float* __restrict__ out,
                                                      int64_t M, int Fo, int R, int64_t y_rs, int mask_mode,
                                                      int accumulate) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * Fo) return;
  const int64_t i = t / Fo;
  const int f = (int)(t - i * Fo);
  float a = 0.f, p = 0.f;
  if (ptr) {
    const int64_t k1 = ptr[i + 1];
    int n = 0;
    for (int64_t k = ptr[i]; k < k1; ++k) {
      unsigned code = edge_code(et[k], R, mask_mode);
      if (!code) continue;
      const float* y = Y + (size_t)col[k] * Fo + f;
      while (code) {
        const int r = __ffs((int)code) - 1;
        code &= code - 1;
        const float v = y[(size_t)r * y_rs];
        p = scale ? fmaf(scale[i * R + r], v, p) : p + v;
      }
      if (++n == 32) a += p, p = 0.f, n = 0;
    }
  }
  a += p;
  out[t] = accumulate ? out[t] + a : a + (bias ? bias[f] : 0.f);
}

// H_r[j,f] = sum over the CSC column j of bit_r(entry) s_r(sink) g[sink,f];  one thread per (r, j, f)
__global__ __launch_bounds__(256) void k_rgcn_csr_aggT(const float* __restrict__ g, const int64_t* __restrict__ cptr,
                                                       const int64_t* __restrict__ rows,
                                                       const int64_t* __restrict__ perm,
                                                       const int64_t* __restrict__ et, const float* __restrict__ scale,
                                                       float* __restrict__ H, int64_t M, int Fo, int R, int mask_mode) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)R * M * Fo) return;
  const int64_t mf = M * Fo;
  const int r = (int)(t / mf);
  const int64_t rem = t - (int64_t)r * mf;
  const int64_t j = rem / Fo;
  const int f = (int)(rem - j * Fo);
  float a = 0.f, p = 0.f;
  if (cptr) {
    const int64_t k1 = cptr[j + 1];
    int n = 0;
    for (int64_t k = cptr[j]; k < k1; ++k) {
      if (!((edge_code(et[perm[k]], R, mask_mode) >> r) & 1u)) continue;
      const int64_t i = rows[k];
      const float v = g[(size_t)i * Fo + f];
      p = scale ? fmaf(scale[i * R + r], v, p) : p + v;
      if (++n == 32) a += p, p = 0.f, n = 0;
    }
  }
  H[t] = a + p;
}

// ---------------------------------------------------------------------------
// TypedEdge
// ---------------------------------------------------------------------------
struct TypedArgs {
  const float* child[MAX_R];
  unsigned bit[MAX_R];
  int n;
};

// adj_out = diff_or(adj, children) (res + t - res t, left to right), rel_out = rel | the bits of the children > 0
__global__ __launch_bounds__(256) void k_typed_merge(const float* __restrict__ adj, const float* __restrict__ rel,
                                                     TypedArgs a, float* __restrict__ adj_out,
                                                     float* __restrict__ rel_out, int64_t L) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= L) return;
  float o = adj_out ? adj[e] : 0.f;
  unsigned add = 0u;
  for (int k = 0; k < a.n; ++k) {
    const float c = a.child[k][e];
    o = o + c - o * c;
    if (c > 0.f) add |= a.bit[k];
  }
  if (adj_out) adj_out[e] = o;
  const float rin = rel[e];
  rel_out[e] = add ? (float)(rel_code(rin) | add) : rin;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: DenseRGCNConv
// ---------------------------------------------------------------------------
static bool dense_dims_ok(int B, int N, int R) {
  return (int64_t)B * R <= 65535 && (int64_t)B * N <= (1 << 30) && (int64_t)R * N < (1LL << 31);
}

extern "C" size_t gcm_dense_rgcnconv_fwd_workspace_bytes(int B, int N, int Fi, int Fo, int R) {
  if (B <= 0 || N <= 0 || Fi <= 0 || Fo <= 0 || R <= 0) return 0;
  return align256((size_t)R * B * N * Fo * sizeof(float));
}

extern "C" int gcm_dense_rgcnconv_fwd(const float* x, const float* adj, const float* rel, const float* weight,
                                      const float* root, const float* bias, float* out, float* scale, void* workspace,
                                      size_t workspace_bytes, int B, int N, int Fi, int Fo, int R, int mean,
                                      gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && rel && weight && out && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && Fo > 0 && R > 0);
  GCM_REQUIRE(!mean || scale);
  if (!widths_ok(Fi, Fo, R) || !dense_dims_ok(B, N, R)) return GCM_EUNSUPPORTED;
  if (workspace_bytes < gcm_dense_rgcnconv_fwd_workspace_bytes(B, N, Fi, Fo, R)) return GCM_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * N;
  float* Y = (float*)workspace;
  int rc;
  if (mean) {
    hipLaunchKernelGGL(k_rgcn_dense_scale, dim3(blocks(rows, 4)), dim3(256), 0, s, rel, scale, rows, N, R);
    if ((rc = gcm_launch_status())) return rc;
  }
  if ((rc = transform(x, weight, Y, rows, Fi, Fo, R, s))) return rc;
  if (root && (rc = root_term(x, root, bias, out, rows, Fi, Fo, s))) return rc;
  dispatch_nct(nct_of(Fo), [&](auto n) {
    hipLaunchKernelGGL(k_rgcn_dense_fwd<n()>, dim3(blocks(N, MB), 1, B), dim3(256), 0, s, adj, rel,
                       mean ? scale : nullptr, Y, bias, out, N, Fo, R, rows * Fo, root ? 1 : 0);
  });
  return gcm_launch_status();
}

extern "C" size_t gcm_dense_rgcnconv_bwd_workspace_bytes(int B, int N, int Fi, int Fo, int R) {
  if (B <= 0 || N <= 0 || Fi <= 0 || Fo <= 0 || R <= 0) return 0;
  const int64_t rows = (int64_t)B * N;
  Carve c;
  c.take((size_t)R * rows * Fo * sizeof(float));  // H
  c.take((size_t)R * rows * Fo * sizeof(float));  // Y (for g_adj)
  c.take(slab_floats(rows, Fi, Fo, R) * sizeof(float));
  return c.at;
}

extern "C" int gcm_dense_rgcnconv_bwd(const float* g_out, const float* x, const float* adj, const float* rel,
                                      const float* weight, const float* root, const float* scale, float* g_x,
                                      float* g_adj, float* g_weight, float* g_root, float* g_bias, void* workspace,
                                      size_t workspace_bytes, int B, int N, int Fi, int Fo, int R,
                                      gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && adj && rel && weight && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && Fo > 0 && R > 0);
  GCM_REQUIRE(!g_root || root);
  if (!widths_ok(Fi, Fo, R) || !dense_dims_ok(B, N, R)) return GCM_EUNSUPPORTED;
  if (workspace_bytes < gcm_dense_rgcnconv_bwd_workspace_bytes(B, N, Fi, Fo, R)) return GCM_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * N;
  Carve c;
  float* H = (float*)((char*)workspace + c.take((size_t)R * rows * Fo * sizeof(float)));
  float* Y = (float*)((char*)workspace + c.take((size_t)R * rows * Fo * sizeof(float)));
  float* slabs = (float*)((char*)workspace + c.take(0));
  int rc;
  if (g_x || g_weight) {
    dispatch_nct(nct_of(Fo), [&](auto n) {
      hipLaunchKernelGGL(k_rgcn_dense_aggT<n()>, dim3(blocks(N, MB), 1, B * R), dim3(256), 0, s, adj, rel, scale,
                         g_out, H, N, Fo, R, rows * Fo);
    });
    if ((rc = gcm_launch_status())) return rc;
  }
  if ((rc = param_grads(g_out, x, H, weight, root, g_x, g_weight, g_root, g_bias, slabs, rows, Fi, Fo, R, s)))
    return rc;
  if (g_adj) {
    if ((rc = transform(x, weight, Y, rows, Fi, Fo, R, s))) return rc;
    const int nct = std::min(nct_of(N), 2);
    gcm_pick(
        [&](auto n) {
          hipLaunchKernelGGL(k_rgcn_dense_gadj<n()>, dim3(blocks(N, MB), blocks(N, 32 * n()), B), dim3(256), 0, s, rel,
                             scale, g_out, Y, g_adj, N, Fo, R, rows * Fo);
          return GCM_OK;
        },
        OneOf<1, 2>{nct});
    if ((rc = gcm_launch_status())) return rc;
  }
  return GCM_OK;
}

// ---------------------------------------------------------------------------
// C ABI: RGCNConv
// ---------------------------------------------------------------------------
static bool csr_dims_ok(int64_t M, int Fo, int R) { return M <= (1 << 30) && (int64_t)R * M * Fo < (1LL << 40); }

extern "C" size_t gcm_csr_rgcnconv_fwd_workspace_bytes(int64_t M, int64_t E, int Fi, int Fo, int R) {
  if (M <= 0 || E < 0 || Fi <= 0 || Fo <= 0 || R <= 0) return 0;
  return align256((size_t)R * M * Fo * sizeof(float));
}

extern "C" int gcm_csr_rgcnconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col,
                                    const int64_t* edge_type, const float* weight, const float* root,
                                    const float* bias, float* out, float* scale, void* workspace,
                                    size_t workspace_bytes, int64_t M, int64_t E, int Fi, int Fo, int R, int mean,
                                    int mask_mode, gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && weight && out && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && Fo > 0 && R > 0);
  GCM_REQUIRE(E == 0 || (col && edge_type));
  GCM_REQUIRE(!mean || scale);
  if (!widths_ok(Fi, Fo, R) || !csr_dims_ok(M, Fo, R)) return GCM_EUNSUPPORTED;
  if (workspace_bytes < gcm_csr_rgcnconv_fwd_workspace_bytes(M, E, Fi, Fo, R)) return GCM_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float* Y = (float*)workspace;
  const int64_t* ptr = E > 0 ? row_ptr : nullptr;
  int rc;
  if (mean) {
    hipLaunchKernelGGL(k_rgcn_csr_scale, dim3(blocks(M * R, 256)), dim3(256), 0, s, ptr, edge_type, scale, M, R,
                       mask_mode);
    if ((rc = gcm_launch_status())) return rc;
  }
  if ((rc = transform(x, weight, Y, M, Fi, Fo, R, s))) return rc;
  if (root && (rc = root_term(x, root, bias, out, M, Fi, Fo, s))) return rc;
  hipLaunchKernelGGL(k_rgcn_csr_fwd, dim3(blocks(M * Fo, 256)), dim3(256), 0, s, Y, ptr, col, edge_type,
                     mean ? scale : nullptr, bias, out, M, Fo, R, M * Fo, mask_mode, root ? 1 : 0);
  return gcm_launch_status();
}

extern "C" size_t gcm_csr_rgcnconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int Fo, int R) {
  if (M <= 0 || E < 0 || Fi <= 0 || Fo <= 0 || R <= 0) return 0;
  Carve c;
  c.take((size_t)R * M * Fo * sizeof(float));  // H
  c.take(slab_floats(M, Fi, Fo, R) * sizeof(float));
  return c.at;
}

extern "C" int gcm_csr_rgcnconv_bwd(const float* g_out, const float* x, const int64_t* edge_type,
                                    const int64_t* col_ptr, const int64_t* rows, const int64_t* perm,
                                    const float* weight, const float* root, const float* scale, float* g_x,
                                    float* g_weight, float* g_root, float* g_bias, void* workspace,
                                    size_t workspace_bytes, int64_t M, int64_t E, int Fi, int Fo, int R, int mask_mode,
                                    gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && weight && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && Fo > 0 && R > 0);
  GCM_REQUIRE(!g_root || root);
  const bool need_h = g_x || g_weight;
  GCM_REQUIRE(E == 0 || !need_h || (edge_type && col_ptr && rows && perm));
  if (!widths_ok(Fi, Fo, R) || !csr_dims_ok(M, Fo, R)) return GCM_EUNSUPPORTED;
  if (workspace_bytes < gcm_csr_rgcnconv_bwd_workspace_bytes(M, E, Fi, Fo, R)) return GCM_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  Carve c;
  float* H = (float*)((char*)workspace + c.take((size_t)R * M * Fo * sizeof(float)));
  float* slabs = (float*)((char*)workspace + c.take(0));
  int rc;
  if (need_h) {
    hipLaunchKernelGGL(k_rgcn_csr_aggT, dim3(blocks((int64_t)R * M * Fo, 256)), dim3(256), 0, s, g_out,
                       E > 0 ? col_ptr : nullptr, rows, perm, edge_type, scale, H, M, Fo, R, mask_mode);
    if ((rc = gcm_launch_status())) return rc;
  }
  return param_grads(g_out, x, H, weight, root, g_x, g_weight, g_root, g_bias, slabs, M, Fi, Fo, R, s);
}

// ---------------------------------------------------------------------------
// C ABI: TypedEdge
// ---------------------------------------------------------------------------
extern "C" int gcm_typed_merge(const float* adj, const float* rel, const float* const* children, const int* bits,
                               int n_children, float* adj_out, float* rel_out, int64_t L, gcm_stream_t stream) {
  GCM_REQUIRE(rel && rel_out && children && bits);
  GCM_REQUIRE(!adj_out || adj);
  GCM_REQUIRE(n_children > 0 && L > 0);
  if (n_children > MAX_R) return GCM_EUNSUPPORTED;
  TypedArgs a = {};
  a.n = n_children;
  for (int k = 0; k < n_children; ++k) {
    GCM_REQUIRE(children[k]);
    if (bits[k] < 0 || bits[k] >= MAX_R) return GCM_EUNSUPPORTED;
    a.child[k] = children[k];
    a.bit[k] = 1u << bits[k];
  }
  hipLaunchKernelGGL(k_typed_merge, dim3(blocks(L, 256)), dim3(256), 0, (hipStream_t)stream, adj, rel, a, adj_out,
                     rel_out, L);
  return gcm_launch_status();
}
