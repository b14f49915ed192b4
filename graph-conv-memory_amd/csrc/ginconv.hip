// GINConv / DenseGINConv (PyG): the aggregation and its gradients on gfx950.  The layer's `nn` is an arbitrary
// module and stays in torch; what is here is
//
//   dense:  h = s x + adj @ x,  s = add_loop ? 1 + eps : 0      g_x = adj^T g_h + s g_h
//           g_adj[b,i,j] = <g_h[b,i,:], x[b,j,:]>                g_eps = sum <g_h, x>
//   sparse: h_i = (1 + eps) x_i + sum over the CSR row i of x[col]
//           g_x[j] = (1 + eps) g_h[j] + sum over the CSC column j of g_h[rows]
//
// eps is read from its device pointer inside the kernels: no host read, so the calls stay HIP-graph capturable.
// The dense contraction runs on v_mfma_f32_32x32x2_f32 in the tile layout of gcn_mm.h (128 rows x 32*NCT columns per
// workgroup, K in tiles of 32 staged through LDS with zero padding, masked stores) with the self term added in the
// epilogue: one launch for h, the same kernel with the adjacency read transposed for g_x.  g_adj is gcn_mm.h's
// k_gcn_mm as it is.  g_eps: fp64 partial sums of fixed element ranges into the workspace, summed in a fixed order by
// one workgroup (fixed_sum.h's dot_sum) - deterministic, no atomics.  F <= 128; any N.
#include "fixed_sum.h"
#include "gcn_mm.h"

namespace {

// C(b,i,:) = sum_k A(b,i,k) X(b,k,:) + s X(b,i,:);  A(b,i,k) = adj[b,i,k], or adj[b,k,i] when tr
template <int NCT>
__global__ __launch_bounds__(256) void k_gin_mm(const float* __restrict__ adj, const float* __restrict__ X,
                                                const float* __restrict__ eps, float* __restrict__ C, int N, int F,
                                                int tr, int add_loop) {
  __shared__ float sA[MB * (KT + 1)];        // [i][k]
  __shared__ float sB[KT * (32 * NCT + 1)];  // [k][j]
  const int b = blockIdx.z;
  const int i0 = blockIdx.x * MB;
  const TileLane t = tile_lane();
  const float* Ab = adj + (size_t)b * N * N;
  const float* Xb = X + (size_t)b * N * F;
  float* Cb = C + (size_t)b * N * F;
  f32x16 acc[NCT];
  tile_zero(acc);
  tile_mma<NCT, false>(
      acc, t, sA, sB, i0, 0, N, F, 0, N, tr != 0, false,  // the fast index of the global read is the fast thread index
      [=](int gi, int gk) { return tr ? Ab[(size_t)gk * N + gi] : Ab[(size_t)gi * N + gk]; },
      [=](int gk, int gj) { return Xb[(size_t)gk * F + gj]; });
  const float s = add_loop ? 1.f + eps[0] : 0.f;
  tile_store(acc, t, i0, 0, N, F, [=](int j) {
    return [=](int i, float v) {
      const size_t off = (size_t)i * F + j;
      if (add_loop) v = fmaf(s, Xb[off], v);
      Cb[off] = v;
    };
  });
}

int launch_gin_mm(const float* adj, const float* X, const float* eps, float* C, int B, int N, int F, int tr,
                  int add_loop, hipStream_t s) {
  const dim3 grid(blocks(N, MB), 1, B);
  dispatch_nct(nct_of(F), [&](auto n) {
    hipLaunchKernelGGL(k_gin_mm<n()>, grid, dim3(256), 0, s, adj, X, eps, C, N, F, tr, add_loop);
  });
  return gcm_launch_status();
}

// out[i,:] = (1 + eps) src[i,:] + sum over ptr[i] <= k < ptr[i+1] of src[idx[k],:]   (one thread per element; the
// destination CSR with x for the forward, the CSC by source with g_h for the backward; ptr NULL: no entries)
__global__ __launch_bounds__(256) void k_gin_gather(const float* __restrict__ src, const int64_t* __restrict__ ptr,
                                                    const int64_t* __restrict__ idx, const float* __restrict__ eps,
                                                    float* __restrict__ out, int64_t M, int F) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * F) return;
  const int64_t i = t / F;
  const int f = (int)(t - i * F);
  float a = 0.f;
  if (ptr) {
    const int64_t k1 = ptr[i + 1];
    for (int64_t k = ptr[i]; k < k1; ++k) a += src[(size_t)idx[k] * F + f];
  }
  out[t] = fmaf(1.f + eps[0], src[t], a);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: DenseGINConv
// ---------------------------------------------------------------------------
extern "C" int gcm_dense_gin_fwd(const float* x, const float* adj, const float* eps, float* h, int B, int N, int F,
                                 int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && eps && h);
  GCM_REQUIRE(B > 0 && N > 0 && F > 0);
  if (F > 128 || B > 65535 || (int64_t)B * N > (1 << 30)) return GCM_EUNSUPPORTED;
  return launch_gin_mm(adj, x, eps, h, B, N, F, 0, add_loop, (hipStream_t)stream);
}

extern "C" size_t gcm_dense_gin_bwd_workspace_bytes(int B, int N, int F) {
  if (B <= 0 || N <= 0 || F <= 0) return 0;
  return dot_ws_bytes((int64_t)B * N * F);
}

extern "C" int gcm_dense_gin_bwd(const float* g_h, const float* x, const float* adj, const float* eps, float* g_x,
                                 float* g_adj, float* g_eps, void* workspace, size_t workspace_bytes, int B, int N,
                                 int F, int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(g_h && x && adj && eps && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && F > 0);
  if (F > 128 || B > 65535 || (int64_t)B * N > (1 << 30)) return GCM_EUNSUPPORTED;
  const int64_t L = (int64_t)B * N * F;
  GCM_REQUIRE(workspace_bytes >= dot_ws_bytes(L));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (g_x && (rc = launch_gin_mm(adj, g_h, eps, g_x, B, N, F, 1, add_loop, s))) return rc;
  if (g_adj) {  // g_adj_ij = <g_h_i, x_j>
    MmArgs p = mm_args();
    p.A = g_h, p.a_bs = (int64_t)N * F, p.a_is = F, p.a_ks = 1;
    p.B = x, p.b_bs = (int64_t)N * F, p.b_ks = 1, p.b_js = F;
    p.C = g_adj, p.c_bs = (int64_t)N * N, p.c_is = N, p.c_js = 1;
    p.M = N, p.N = N, p.K = F, p.batch = B;
    if ((rc = launch_mm(p, 1, s))) return rc;
  }
  if (g_eps) {
    if (add_loop) {
      if ((rc = dot_sum(g_h, x, L, g_eps, workspace, s))) return rc;
    } else {  // eps is not used: the sum of no partials
      if ((rc = sum_parts((const double*)workspace, 0, g_eps, s))) return rc;
    }
  }
  return GCM_OK;
}

// ---------------------------------------------------------------------------
// C ABI: GINConv
// ---------------------------------------------------------------------------
extern "C" int gcm_csr_gin_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* eps, float* h,
                               int64_t M, int64_t E, int F, gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && eps && h);
  GCM_REQUIRE(M > 0 && E >= 0 && F > 0);
  GCM_REQUIRE(E == 0 || col);
  if (F > 128 || M > (1 << 30)) return GCM_EUNSUPPORTED;
  hipLaunchKernelGGL(k_gin_gather, dim3(blocks(M * F, 256)), dim3(256), 0, (hipStream_t)stream, x,
                     E > 0 ? row_ptr : nullptr, col, eps, h, M, F);
  return gcm_launch_status();
}

extern "C" size_t gcm_csr_gin_bwd_workspace_bytes(int64_t M, int64_t E, int F) {
  if (M <= 0 || E < 0 || F <= 0) return 0;
  return dot_ws_bytes(M * F);
}

extern "C" int gcm_csr_gin_bwd(const float* g_h, const float* x, const float* eps, const int64_t* col_ptr,
                               const int64_t* rows, float* g_x, float* g_eps, void* workspace, size_t workspace_bytes,
                               int64_t M, int64_t E, int F, gcm_stream_t stream) {
  GCM_REQUIRE(g_h && eps && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && F > 0);
  GCM_REQUIRE(!g_eps || x);
  GCM_REQUIRE(E == 0 || !g_x || (col_ptr && rows));
  if (F > 128 || M > (1 << 30)) return GCM_EUNSUPPORTED;
  GCM_REQUIRE(workspace_bytes >= dot_ws_bytes(M * F));
  hipStream_t s = (hipStream_t)stream;
  if (g_x) {
    hipLaunchKernelGGL(k_gin_gather, dim3(blocks(M * F, 256)), dim3(256), 0, s, g_h, E > 0 ? col_ptr : nullptr, rows,
                       eps, g_x, M, F);
    const int rc = gcm_launch_status();
    if (rc) return rc;
  }
  return g_eps ? dot_sum(g_h, x, M * F, g_eps, workspace, s) : GCM_OK;
}
