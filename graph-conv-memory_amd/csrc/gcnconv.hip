// GCNConv / DenseGCNConv (PyG) forward and backward on gfx950.
//
//   dense:  A = adj with A[i,i] = loop_value (add_loop);  deg = max(rowsum(A), 1);  d = deg^-1/2
//           out = d_i * sum_j A_ij d_j (x W^T)_j + bias
//   sparse: PyG's gcn_norm over the destination CSR (add_remaining_self_loops, in-degree,
//           deg^-1/2 with inf -> 0), then out = (A~ x) W^T + bias with A~ = the per-edge
//           coefficients plus a per-row loop coefficient.
//
// The contractions run on v_mfma_f32_32x32x2_f32: the sparse forward in its own gather + linear
// kernel (k_gcn_csr_fwd), every other one in one strided, batched tile kernel (k_gcn_mm, gcn_mm.h): 128 rows x 32*NCT columns per workgroup, K in tiles of 32 staged through LDS with
// zero padding, masked stores.  Its operand and epilogue hooks carry the GCN-specific parts:
// the diagonal override of the staged adjacency, the d_j scaling of the staged B rows, the
// d_i d_j scaling of the output and the row term of the adjacency gradient.  The normalised
// adjacency is never written to memory.  Fi, Fo <= 128; any N.
#include "gcn_mm.h"

namespace {

// ---------------------------------------------------------------------------
// dense: row degrees from the adjacency with the diagonal override (one wave per row)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_gcn_dense_deg(const float* __restrict__ adj, float* __restrict__ deg,
                                                       float* __restrict__ dinv, int64_t rows, int N,
                                                       int add_loop, float loop_value) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int i = (int)(row % N);
  const float* a = adj + (size_t)row * N;
  float s = 0.f;
  for (int j = lane; j < N; j += 64) s += (add_loop && j == i) ? loop_value : a[j];
  s = gcm_wave_sum(s);
  if (lane == 0) {
    deg[row] = s;
    dinv[row] = 1.f / sqrtf(fmaxf(s, 1.f));
  }
}

// dense backward, row-local part (one wave per row j):
//   gd_j = <G_j, P_j> + <gZ_j, Y_j>        (d_j's two uses: output scale, operand scale)
//   c_j  = -1/2 d_j^3 gd_j  where rowsum >= 1 (clamp(min=1) passes the gradient at the bound)
//   gY_j = d_j gZ_j                          (in place over gZ)
__global__ __launch_bounds__(256) void k_gcn_dense_rowgrad(const float* __restrict__ g_out,
                                                           const float* __restrict__ agg,
                                                           const float* __restrict__ y,
                                                           const float* __restrict__ deg,
                                                           const float* __restrict__ dinv,
                                                           float* __restrict__ gz, float* __restrict__ c,
                                                           int64_t rows, int Fo) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const size_t o = (size_t)row * Fo;
  const float d = dinv[row];
  float s = 0.f;
  for (int f = lane; f < Fo; f += 64) {
    const float g = gz[o + f];
    s = fmaf(g_out[o + f], agg[o + f], s);
    s = fmaf(g, y[o + f], s);
    gz[o + f] = d * g;
  }
  s = gcm_wave_sum(s);
  if (lane == 0) c[row] = deg[row] >= 1.f ? -0.5f * d * d * d * s : 0.f;
}

// ---------------------------------------------------------------------------
// sparse: gcn_norm over the destination CSR
// ---------------------------------------------------------------------------
// one thread per node i: loop weight (last existing i->i edge in edge order, else fill), in-degree,
// dinv, loop coefficient.  Self-loop edges count as ordinary edges unless loops are added.
__global__ void k_gcn_norm_rows(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col,
                                const float* __restrict__ w, float* __restrict__ dinv,
                                float* __restrict__ loop_w, float* __restrict__ loop_coef,
                                int64_t* __restrict__ loop_e, int64_t M, int normalize, int add_loops,
                                float fill) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  if (!normalize) {
    dinv[i] = 1.f, loop_w[i] = 0.f, loop_coef[i] = 0.f, loop_e[i] = -1;
    return;
  }
  float deg = 0.f;
  int64_t le = -1;
  for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
    if (add_loops && col[e] == i) {
      le = e;
      continue;
    }
    deg += w ? w[e] : 1.f;
  }
  const float lw = add_loops ? (le >= 0 ? (w ? w[le] : 1.f) : fill) : 0.f;
  deg += lw;
  const float d = deg == 0.f ? 0.f : 1.f / sqrtf(deg);
  dinv[i] = d, loop_w[i] = lw, loop_coef[i] = d * lw * d, loop_e[i] = le;
}

// one thread per CSR edge: coef = d_src w d_dst (w alone without normalisation), 0 for a self-loop
// that the added loop replaces
__global__ void k_gcn_norm_edges(const int64_t* __restrict__ col, const int64_t* __restrict__ dst,
                                 const float* __restrict__ w, const float* __restrict__ dinv,
                                 float* __restrict__ coef, int64_t E, int normalize, int add_loops) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const float we = w ? w[e] : 1.f;
  const int64_t s = col[e], t = dst[e];
  if (!normalize) coef[e] = we;
  else coef[e] = (add_loops && s == t) ? 0.f : dinv[s] * we * dinv[t];
}

// forward: agg_i = sum_e coef_e x_src + loop_coef_i x_i gathered into LDS, then out = agg W^T + b
template <int NCT>
__global__ __launch_bounds__(256) void k_gcn_csr_fwd(
    const float* __restrict__ x, const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col,
    const float* __restrict__ coef, const float* __restrict__ loop_coef, const float* __restrict__ w,
    const float* __restrict__ bias, float* __restrict__ out, float* __restrict__ agg_out, int64_t M,
    int Fi, int Fo) {
  constexpr int FiP = 32 * NCT;
  const int64_t r0 = (int64_t)blockIdx.x * MB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  __shared__ float sAgg[MB * (FiP + 1)];
  __shared__ float sW[FiP * 33];

  for (int idx = threadIdx.x; idx < MB * FiP; idx += 256) {
    const int r = idx / FiP, f = idx - r * FiP;
    const int64_t row = r0 + r;
    float a = 0.f;
    if (row < M && f < Fi) {
      a = loop_coef[row] * x[(size_t)row * Fi + f];
      const int64_t e1 = row_ptr[row + 1];
      for (int64_t e = row_ptr[row]; e < e1; ++e) a = fmaf(coef[e], x[(size_t)col[e] * Fi + f], a);
      if (agg_out) agg_out[(size_t)row * Fi + f] = a;
    }
    sAgg[r * (FiP + 1) + f] = a;
  }
  for (int o0 = 0; o0 < Fo; o0 += 32) {
    __syncthreads();
    for (int e = threadIdx.x; e < 32 * FiP; e += 256) {  // sW[k][n] = w[o0 + n][k]
      const int n = e / FiP, k = e - n * FiP;
      sW[k * 33 + n] = (o0 + n < Fo && k < Fi) ? w[(size_t)(o0 + n) * Fi + k] : 0.f;
    }
    __syncthreads();
    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    mma32(o, sAgg + wave * 32 * (FiP + 1), FiP + 1, 1, sW, 33, 1, FiP, li, lh);
    const int c = o0 + li;
    const float bv = (bias && c < Fo) ? bias[c] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = r0 + wave * 32 + acc_row(r, lh);
      if (row < M && c < Fo) out[(size_t)row * Fo + c] = o[r] + bv;
    }
  }
}

// g_x[j] = loop_coef_j dAgg_j + sum over the CSC column j of coef * dAgg[dst]
__global__ void k_gcn_scatter_T(const float* __restrict__ dagg, const int64_t* __restrict__ col_ptr,
                                const int64_t* __restrict__ rows, const int64_t* __restrict__ perm,
                                const float* __restrict__ coef, const float* __restrict__ loop_coef,
                                float* __restrict__ g_x, int64_t M, int Fi) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * Fi) return;
  const int64_t j = i / Fi;
  const int f = (int)(i - j * Fi);
  float a = loop_coef[j] * dagg[i];
  if (col_ptr)
    for (int64_t k = col_ptr[j]; k < col_ptr[j + 1]; ++k) a = fmaf(coef[perm[k]], dagg[(size_t)rows[k] * Fi + f], a);
  g_x[i] = a;
}

// edge-weight backward, pass 1 (one thread per CSR row i):
//   gcoef_e = <x_src, dAgg_i>;  g_lw_i = d_i^2 <x_i, dAgg_i>
//   gd_i (in-edge part) = sum_e gcoef_e d_src w_e + 2 d_i lw_i <x_i, dAgg_i>
__global__ void k_gcn_wgrad_rows(const float* __restrict__ x, const float* __restrict__ dagg,
                                 const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col,
                                 const float* __restrict__ w, const float* __restrict__ dinv,
                                 const float* __restrict__ loop_w, float* __restrict__ gcoef,
                                 float* __restrict__ gd, float* __restrict__ g_lw, int64_t M, int Fi,
                                 int normalize, int add_loops) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float* gi = dagg + (size_t)i * Fi;
  float acc = 0.f;
  for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
    const int64_t s = col[e];
    float g = 0.f;
    for (int f = 0; f < Fi; ++f) g = fmaf(x[(size_t)s * Fi + f], gi[f], g);
    gcoef[e] = g;
    if (normalize && !(add_loops && s == i)) acc = fmaf(g, dinv[s] * (w ? w[e] : 1.f), acc);
  }
  if (!normalize) return;
  float gl = 0.f;
  for (int f = 0; f < Fi; ++f) gl = fmaf(x[(size_t)i * Fi + f], gi[f], gl);
  const float d = dinv[i];
  gd[i] = fmaf(2.f * d * loop_w[i], gl, acc);
  g_lw[i] = d * d * gl;
}

// pass 2 (one thread per node j, over its CSC column): out-edge part of gd_j, then
// g_deg_j = -1/2 d_j^3 gd_j (0 where deg == 0: the inf -> 0 fill)
__global__ void k_gcn_wgrad_cols(const int64_t* __restrict__ col_ptr, const int64_t* __restrict__ rows,
                                 const int64_t* __restrict__ perm, const float* __restrict__ w,
                                 const float* __restrict__ dinv, const float* __restrict__ gcoef,
                                 float* __restrict__ gd, int64_t M, int add_loops) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M) return;
  float a = gd[j];
  if (col_ptr)
    for (int64_t k = col_ptr[j]; k < col_ptr[j + 1]; ++k) {
      const int64_t t = rows[k], e = perm[k];
      if (add_loops && t == j) continue;
      a = fmaf(gcoef[e], (w ? w[e] : 1.f) * dinv[t], a);
    }
  const float d = dinv[j];
  gd[j] = d == 0.f ? 0.f : -0.5f * d * d * d * a;
}

// pass 3 (one thread per CSR edge): g_w_e = gcoef_e d_src d_dst + g_deg_dst; the kept self-loop gets
// g_lw + g_deg of its node, the other self-loops 0
__global__ void k_gcn_wgrad_edges(const int64_t* __restrict__ col, const int64_t* __restrict__ dst,
                                  const float* __restrict__ dinv, const float* __restrict__ gcoef,
                                  const float* __restrict__ gdeg, const float* __restrict__ g_lw,
                                  const int64_t* __restrict__ loop_e, float* __restrict__ g_w, int64_t E,
                                  int normalize, int add_loops) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  if (!normalize) {
    g_w[e] = gcoef[e];
    return;
  }
  const int64_t s = col[e], t = dst[e];
  if (add_loops && s == t) g_w[e] = loop_e[t] == e ? g_lw[t] + gdeg[t] : 0.f;
  else g_w[e] = fmaf(gcoef[e], dinv[s] * dinv[t], gdeg[t]);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: DenseGCNConv
// ---------------------------------------------------------------------------
extern "C" int gcm_dense_gcnconv_fwd(const float* x, const float* adj, const float* w, const float* bias,
                                     float* out, float* y, float* agg, float* deg, float* dinv, int B, int N,
                                     int Fi, int Fo, int add_loop, float loop_value, gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && w && out && y && deg && dinv);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && Fo > 0);
  if (Fi > 128 || Fo > 128 || B > 65535 || (int64_t)B * N > (1 << 30)) return GCM_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * N;
  hipLaunchKernelGGL(k_gcn_dense_deg, dim3(blocks(rows, 4)), dim3(256), 0, s, adj, deg, dinv, rows, N,
                     add_loop, loop_value);
  int rc = gcm_launch_status();
  if (rc) return rc;
  if ((rc = mm_xwt(x, w, nullptr, y, rows, Fi, Fo, s))) return rc;  // y = x W^T over all B*N rows
  MmArgs p = mm_args();  // out = d_i sum_k A_ik d_k y_k + bias;  agg = sum_k A_ik d_k y_k
  p.A = adj, p.a_bs = (int64_t)N * N, p.a_is = N, p.a_ks = 1;
  p.a_diag = add_loop, p.diag_val = loop_value;
  p.B = y, p.b_bs = (int64_t)N * Fo, p.b_ks = Fo, p.b_js = 1, p.b_kscale = dinv;
  p.C = out, p.c_bs = (int64_t)N * Fo, p.c_is = Fo, p.c_js = 1, p.C2 = agg;
  p.c_rscale = dinv, p.c_bias = bias, p.s_bs = N;
  p.M = N, p.N = Fo, p.K = N, p.batch = B;
  return launch_mm(p, 1, s);
}

namespace {
struct DenseBwdWs {
  size_t gz, c, slabs, total;
};
DenseBwdWs dense_bwd_ws(int B, int N, int Fi, int Fo) {
  DenseBwdWs w;
  const int64_t rows = (int64_t)B * N;
  int nsplit, kchunk;
  wgrad_split(rows, &nsplit, &kchunk);
  const size_t slab_f = std::max<size_t>((size_t)nsplit * Fo * Fi, (size_t)colsum_slabs(rows) * Fo);
  w.gz = 0;
  w.c = align256(rows * Fo * sizeof(float));
  w.slabs = w.c + align256(rows * sizeof(float));
  w.total = w.slabs + slab_f * sizeof(float);
  return w;
}
}  // namespace

extern "C" size_t gcm_dense_gcnconv_bwd_workspace_bytes(int B, int N, int Fi, int Fo) {
  if (B <= 0 || N <= 0 || Fi <= 0 || Fo <= 0) return 0;
  return dense_bwd_ws(B, N, Fi, Fo).total;
}

extern "C" int gcm_dense_gcnconv_bwd(const float* g_out, const float* x, const float* adj, const float* w,
                                     const float* y, const float* agg, const float* deg, const float* dinv,
                                     float* g_x, float* g_adj, float* g_w, float* g_bias, void* workspace,
                                     size_t workspace_bytes, int B, int N, int Fi, int Fo, int add_loop,
                                     float loop_value, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && adj && w && y && agg && deg && dinv && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && Fo > 0);
  if (Fi > 128 || Fo > 128 || B > 65535 || (int64_t)B * N > (1 << 30)) return GCM_EUNSUPPORTED;
  const DenseBwdWs L = dense_bwd_ws(B, N, Fi, Fo);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* gz = (float*)(ws + L.gz);
  float* c = (float*)(ws + L.c);
  float* slabs = (float*)(ws + L.slabs);
  const int64_t rows = (int64_t)B * N;
  int rc;
  if (g_bias && (rc = colsum(g_out, rows, Fo, g_bias, slabs, s))) return rc;
  if (!g_x && !g_adj && !g_w) return GCM_OK;
  MmArgs p = mm_args();  // gZ_j = sum_i A_ij d_i G_i
  p.A = adj, p.a_bs = (int64_t)N * N, p.a_is = 1, p.a_ks = N;
  p.a_diag = add_loop, p.diag_val = loop_value;
  p.B = g_out, p.b_bs = (int64_t)N * Fo, p.b_ks = Fo, p.b_js = 1, p.b_kscale = dinv, p.s_bs = N;
  p.C = gz, p.c_bs = (int64_t)N * Fo, p.c_is = Fo, p.c_js = 1;
  p.M = N, p.N = Fo, p.K = N, p.batch = B;
  if ((rc = launch_mm(p, 1, s))) return rc;
  hipLaunchKernelGGL(k_gcn_dense_rowgrad, dim3(blocks(rows, 4)), dim3(256), 0, s, g_out, agg, y, deg, dinv,
                     gz, c, rows, Fo);
  if ((rc = gcm_launch_status())) return rc;
  if (g_x && (rc = mm_gw(gz, w, g_x, rows, Fi, Fo, s))) return rc;  // g_x = gY W
  if (g_w && (rc = wgrad(gz, x, g_w, slabs, rows, Fi, Fo, s))) return rc;
  if (g_adj) {  // g_adj_ij = d_i d_j <G_i, y_j> + c_i, 0 on an overwritten diagonal
    p = mm_args();
    p.A = g_out, p.a_bs = (int64_t)N * Fo, p.a_is = Fo, p.a_ks = 1;
    p.B = y, p.b_bs = (int64_t)N * Fo, p.b_ks = 1, p.b_js = Fo;
    p.C = g_adj, p.c_bs = (int64_t)N * N, p.c_is = N, p.c_js = 1;
    p.c_rscale = dinv, p.c_cscale = dinv, p.c_radd = c, p.s_bs = N, p.c_zero_diag = add_loop;
    p.M = N, p.N = N, p.K = Fo, p.batch = B;
    if ((rc = launch_mm(p, 1, s))) return rc;
  }
  return GCM_OK;
}

// ---------------------------------------------------------------------------
// C ABI: GCNConv
// ---------------------------------------------------------------------------
extern "C" int gcm_gcn_norm(const int64_t* row_ptr, const int64_t* col, const int64_t* dst, const float* w,
                            float* coef, float* dinv, float* loop_w, float* loop_coef, int64_t* loop_e,
                            int64_t M, int64_t E, int normalize, int add_self_loops, float fill,
                            gcm_stream_t stream) {
  GCM_REQUIRE(row_ptr && dinv && loop_w && loop_coef && loop_e);
  GCM_REQUIRE(M > 0 && E >= 0);
  GCM_REQUIRE(E == 0 || (col && dst && coef));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_gcn_norm_rows, dim3(blocks(M, 256)), dim3(256), 0, s, row_ptr, col, w, dinv, loop_w,
                     loop_coef, loop_e, M, normalize, add_self_loops, fill);
  int rc = gcm_launch_status();
  if (rc || E == 0) return rc;
  hipLaunchKernelGGL(k_gcn_norm_edges, dim3(blocks(E, 256)), dim3(256), 0, s, col, dst, w, dinv, coef, E,
                     normalize, add_self_loops);
  return gcm_launch_status();
}

extern "C" int gcm_csr_gcnconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* coef,
                                   const float* loop_coef, const float* w, const float* bias, float* out,
                                   float* agg, int64_t M, int64_t E, int Fi, int Fo, gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && loop_coef && w && out);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && Fo > 0);
  GCM_REQUIRE(E == 0 || (col && coef));
  if (Fi > 128 || Fo > 128) return GCM_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(blocks(M, MB));
  dispatch_nct((Fi + 31) / 32, [&](auto n) {
    hipLaunchKernelGGL(k_gcn_csr_fwd<n()>, grid, dim3(256), 0, s, x, row_ptr, col, coef, loop_coef, w, bias, out, agg,
                       M, Fi, Fo);
  });
  return gcm_launch_status();
}

namespace {
struct CsrBwdWs {
  size_t dagg, gcoef, gd, glw, slabs, total;
};
CsrBwdWs csr_bwd_ws(int64_t M, int64_t E, int Fi, int Fo) {
  CsrBwdWs w;
  int nsplit, kchunk;
  wgrad_split(M, &nsplit, &kchunk);
  const size_t slab_f = std::max<size_t>((size_t)nsplit * Fo * Fi, (size_t)colsum_slabs(M) * Fo);
  w.dagg = 0;
  w.gcoef = align256(M * Fi * sizeof(float));
  w.gd = w.gcoef + align256(std::max<int64_t>(E, 1) * sizeof(float));
  w.glw = w.gd + align256(M * sizeof(float));
  w.slabs = w.glw + align256(M * sizeof(float));
  w.total = w.slabs + slab_f * sizeof(float);
  return w;
}
}  // namespace

extern "C" size_t gcm_csr_gcnconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int Fo) {
  if (M <= 0 || E < 0 || Fi <= 0 || Fo <= 0) return 0;
  return csr_bwd_ws(M, E, Fi, Fo).total;
}

extern "C" int gcm_csr_gcnconv_bwd(const float* g_out, const float* x, const float* agg, const int64_t* row_ptr,
                                   const int64_t* col, const int64_t* dst, const int64_t* col_ptr,
                                   const int64_t* rows, const int64_t* perm, const float* w_edge,
                                   const float* coef, const float* dinv, const float* loop_w,
                                   const float* loop_coef, const int64_t* loop_e, const float* w, float* g_x,
                                   float* g_edge, float* g_w, float* g_bias, void* workspace,
                                   size_t workspace_bytes, int64_t M, int64_t E, int Fi, int Fo, int normalize,
                                   int add_self_loops, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && agg && row_ptr && dinv && loop_w && loop_coef && loop_e && w && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && Fo > 0);
  GCM_REQUIRE(E == 0 || (col && dst && coef && col_ptr && rows && perm) || (!g_x && !g_edge));
  if (Fi > 128 || Fo > 128 || M > (1 << 30)) return GCM_EUNSUPPORTED;
  const CsrBwdWs L = csr_bwd_ws(M, E, Fi, Fo);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* dagg = (float*)(ws + L.dagg);
  float* gcoef = (float*)(ws + L.gcoef);
  float* gd = (float*)(ws + L.gd);
  float* glw = (float*)(ws + L.glw);
  float* slabs = (float*)(ws + L.slabs);
  int rc;
  if (g_bias && (rc = colsum(g_out, M, Fo, g_bias, slabs, s))) return rc;
  if (g_w && (rc = wgrad(g_out, agg, g_w, slabs, M, Fi, Fo, s))) return rc;
  if (!g_x && !g_edge) return GCM_OK;
  if ((rc = mm_gw(g_out, w, dagg, M, Fi, Fo, s))) return rc;  // dAgg = G W
  const bool has_e = E > 0;
  if (g_x) {
    hipLaunchKernelGGL(k_gcn_scatter_T, dim3(blocks(M * Fi, 256)), dim3(256), 0, s, dagg,
                       has_e ? col_ptr : nullptr, rows, perm, coef, loop_coef, g_x, M, Fi);
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_edge && has_e) {
    hipLaunchKernelGGL(k_gcn_wgrad_rows, dim3(blocks(M, 256)), dim3(256), 0, s, x, dagg, row_ptr, col, w_edge,
                       dinv, loop_w, gcoef, gd, glw, M, Fi, normalize, add_self_loops);
    if ((rc = gcm_launch_status())) return rc;
    if (normalize) {
      hipLaunchKernelGGL(k_gcn_wgrad_cols, dim3(blocks(M, 256)), dim3(256), 0, s, col_ptr, rows, perm, w_edge,
                         dinv, gcoef, gd, M, add_self_loops);
      if ((rc = gcm_launch_status())) return rc;
    }
    hipLaunchKernelGGL(k_gcn_wgrad_edges, dim3(blocks(E, 256)), dim3(256), 0, s, col, dst, dinv, gcoef, gd, glw,
                       loop_e, g_edge, E, normalize, add_self_loops);
    if ((rc = gcm_launch_status())) return rc;
  }
  return GCM_OK;
}
