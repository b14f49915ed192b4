// TransformerConv / DenseTransformerConv (PyG, without edge features) forward and backward on gfx950.
//
//   [q | k | v | r] = x W_all^T + b_all (one tile GEMM over the stacked weights), each of q, k, v viewed [rows, H, C]
//   s[i,j,h] = <q[i,h,:], k[j,h,:]> / sqrt(C) over the neighbours j of i, alpha = softmax_j(s)
//   o[i,h,:] = sum_j alpha v[j,h,:];  om = concat_h(o) or mean_h(o)
//   out = om + r, or with the gate g = sigmoid(<w_beta, [om, r, om - r]>): out = g r + (1 - g) om
//
// A row with no neighbour aggregates nothing: its o is 0 and its out is r (0 without the skip).
//
// dense: the bit image of the pattern (attn_bits.h) is built once.  k_tr_dense_fwd is a masked flash attention: a
// workgroup owns 128 rows of a graph, heads outer, tiles of 32 neighbours inner; S^T = K Q^T on
// v_mfma_f32_32x32x2_f32 with the contraction over C (the row of a lane's 16 scores is the lane's own, so the online
// softmax needs one cross-lane step), P V on the matrix cores, only the row statistics (max, sum) leave.  The
// backward recomputes P from them in two kernels, neither of which sums across workgroups: k_tr_dense_dq by row
// block (sweep 1: delta_i = sum_j P dP from the recomputed P; sweep 2: dS = P (dP - delta), dQ = dS K), and
// k_tr_dense_dkv by neighbour block (dV = P^T dO, dK = dS^T Q), every product on the matrix cores.  delta is the sum
// over the same P that multiplies (dP - delta), not <dO_i, o_i>: sum_j dS_ij then cancels as far as the sum's own
// rounding, which the key bias gradient (exactly 0 in exact arithmetic) consists of.
// sparse: a group of 8..64 lanes per (destination, head) walks the CSR row once (online softmax), each lane holding
// C / group channels, the C-long dot products summed across the group; the backward does the same twice per row
// (delta, then dS and dQ) and gathers dK, dV per (source, column) through the CSC view.
// The stacked projection gradient [dQ | dK | dV | dR] gives g_x, g_w_all and g_b_all in one GEMM, one split-K
// weight gradient and one column sum (gcn_mm.h).  Nothing accumulates with atomics: every sum runs in a fixed order.
// Fi, H*C <= 128; any N.
#include "transformer_common.h"

// ---------------------------------------------------------------------------
// C ABI: DenseTransformerConv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_dense_transformerconv_fwd_workspace_bytes(int B, int N, int Fi, int H, int C, int concat,
                                                                int root) {
  if (B <= 0 || N <= 0 || Fi <= 0 || H <= 0 || C <= 0) return 0;
  const int64_t R = (int64_t)B * N;
  return saved_layout(dims(R, Fi, H, C, concat, root), R * ((N + 31) / 32)).total;
}

extern "C" int gcm_dense_transformerconv_fwd(const float* x, const float* adj, const float* w_all, const float* b_all,
                                             const float* w_beta, float* out, void* saved, size_t saved_bytes, int B,
                                             int N, int Fi, int H, int C, int concat, int root, int add_loop,
                                             gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && w_all && b_all && out && saved);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && H > 0 && C > 0);
  GCM_REQUIRE(root || !w_beta);
  const int64_t R = (int64_t)B * N;
  if (unsupported(R, Fi, H, C) || B > 65535) return GCM_EUNSUPPORTED;
  const Dims d = dims(R, Fi, H, C, concat, root);
  const int W = (N + 31) / 32;
  const Saved L = saved_layout(d, R * W);
  GCM_REQUIRE(saved_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* sv = (char*)saved;
  unsigned* bits = (unsigned*)(sv + L.bits);
  float* proj = (float*)(sv + L.proj);
  int rc = mask_bits(adj, bits, R, N, W, add_loop, s);
  if (rc || (rc = project(x, w_all, b_all, proj, d, s))) return rc;
  const dim3 grid(dense_blocks(N), B);
  const float scale = 1.f / sqrtf((float)C);
  dispatch_nct((C + 31) / 32, [&](auto n) {
    hipLaunchKernelGGL(k_tr_dense_fwd<n()>, grid, dim3(256), 0, s, bits, proj, d.P, (float*)(sv + L.o),
                       (float*)(sv + L.m), (float*)(sv + L.l), N, H, C, scale);
  });
  if ((rc = gcm_launch_status())) return rc;
  return fwd_tail(w_beta, out, L, sv, d, concat, s);
}

extern "C" size_t gcm_dense_transformerconv_bwd_workspace_bytes(int B, int N, int Fi, int H, int C, int concat,
                                                                int root) {
  if (B <= 0 || N <= 0 || Fi <= 0 || H <= 0 || C <= 0) return 0;
  return bwd_ws(dims((int64_t)B * N, Fi, H, C, concat, root), 0).total;
}

extern "C" int gcm_dense_transformerconv_bwd(const float* g_out, const float* x, const float* w_all,
                                             const float* w_beta, const void* saved, float* g_x, float* g_w_all,
                                             float* g_b_all, float* g_w_beta, void* workspace, size_t workspace_bytes,
                                             int B, int N, int Fi, int H, int C, int concat, int root,
                                             gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && w_all && saved && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && H > 0 && C > 0);
  GCM_REQUIRE((root || !w_beta) && (w_beta || !g_w_beta));
  const int64_t R = (int64_t)B * N;
  if (unsupported(R, Fi, H, C) || B > 65535) return GCM_EUNSUPPORTED;
  const Dims d = dims(R, Fi, H, C, concat, root);
  const int W = (N + 31) / 32;
  const Saved L = saved_layout(d, R * W);
  const BwdWs K = bwd_ws(d, 0);
  GCM_REQUIRE(workspace_bytes >= K.total);
  if (!g_x && !g_w_all && !g_b_all && !g_w_beta) return GCM_OK;
  hipStream_t s = (hipStream_t)stream;
  const char* sv = (const char*)saved;
  char* ws = (char*)workspace;
  int rc = bwd_head(g_out, w_beta, g_w_beta, L, sv, K, ws, d, concat, s);
  if (rc) return rc;
  const unsigned* bits = (const unsigned*)(sv + L.bits);
  const float* proj = (const float*)(sv + L.proj);
  const float* row_m = (const float*)(sv + L.m);
  const float* row_l = (const float*)(sv + L.l);
  const float* dO = (const float*)(ws + K.dO);
  float* delta = (float*)(ws + K.delta);
  float* gp = (float*)(ws + K.gp);
  const dim3 grid(dense_blocks(N), B);
  const float scale = 1.f / sqrtf((float)C);
  dispatch_nct((C + 31) / 32, [&](auto n) {
    hipLaunchKernelGGL(k_tr_dense_dq<n()>, grid, dim3(256), 0, s, bits, proj, d.P, dO, row_m, row_l, delta, gp, N, H, C,
                       scale);
  });
  if ((rc = gcm_launch_status())) return rc;
  dispatch_nct((C + 31) / 32, [&](auto n) {
    hipLaunchKernelGGL(k_tr_dense_dkv<n()>, grid, dim3(256), 0, s, bits, proj, d.P, dO, row_m, row_l,
                       (const float*)delta, gp, N, H, C, scale);
  });
  if ((rc = gcm_launch_status())) return rc;
  return bwd_tail(x, w_all, g_x, g_w_all, g_b_all, K, ws, d, s);
}

// ---------------------------------------------------------------------------
// C ABI: TransformerConv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_csr_transformerconv_fwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int concat,
                                                              int root) {
  if (M <= 0 || E < 0 || Fi <= 0 || H <= 0 || C <= 0) return 0;
  return saved_layout(dims(M, Fi, H, C, concat, root), 0).total;
}

extern "C" int gcm_csr_transformerconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col,
                                           const float* w_all, const float* b_all, const float* w_beta, float* out,
                                           void* saved, size_t saved_bytes, int64_t M, int64_t E, int Fi, int H, int C,
                                           int concat, int root, gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && w_all && b_all && out && saved);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && H > 0 && C > 0);
  GCM_REQUIRE(E == 0 || col);
  GCM_REQUIRE(root || !w_beta);
  if (unsupported(M, Fi, H, C)) return GCM_EUNSUPPORTED;
  const Dims d = dims(M, Fi, H, C, concat, root);
  const Saved L = saved_layout(d, 0);
  GCM_REQUIRE(saved_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* sv = (char*)saved;
  float* proj = (float*)(sv + L.proj);
  int rc = project(x, w_all, b_all, proj, d, s);
  if (rc) return rc;
  const float scale = 1.f / sqrtf((float)C);
  TR_LAUNCH_GROUP(k_tr_csr_fwd, M * H, s, row_ptr, col, (const float*)proj, d.P, (float*)(sv + L.o),
                  (float*)(sv + L.m), (float*)(sv + L.l), M, H, C, scale)
  if ((rc = gcm_launch_status())) return rc;
  return fwd_tail(w_beta, out, L, sv, d, concat, s);
}

extern "C" size_t gcm_csr_transformerconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int concat,
                                                              int root) {
  if (M <= 0 || E < 0 || Fi <= 0 || H <= 0 || C <= 0) return 0;
  return bwd_ws(dims(M, Fi, H, C, concat, root), E).total;
}

extern "C" int gcm_csr_transformerconv_bwd(const float* g_out, const float* x, const int64_t* row_ptr,
                                           const int64_t* col, const int64_t* col_ptr, const int64_t* rows,
                                           const int64_t* perm, const float* w_all, const float* w_beta,
                                           const void* saved, float* g_x, float* g_w_all, float* g_b_all,
                                           float* g_w_beta, void* workspace, size_t workspace_bytes, int64_t M,
                                           int64_t E, int Fi, int H, int C, int concat, int root,
                                           gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && row_ptr && w_all && saved && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && H > 0 && C > 0);
  GCM_REQUIRE(E == 0 || (col && col_ptr && rows && perm));
  GCM_REQUIRE((root || !w_beta) && (w_beta || !g_w_beta));
  if (unsupported(M, Fi, H, C)) return GCM_EUNSUPPORTED;
  const Dims d = dims(M, Fi, H, C, concat, root);
  const Saved L = saved_layout(d, 0);
  const BwdWs K = bwd_ws(d, E);
  GCM_REQUIRE(workspace_bytes >= K.total);
  if (!g_x && !g_w_all && !g_b_all && !g_w_beta) return GCM_OK;
  hipStream_t s = (hipStream_t)stream;
  const char* sv = (const char*)saved;
  char* ws = (char*)workspace;
  int rc = bwd_head(g_out, w_beta, g_w_beta, L, sv, K, ws, d, concat, s);
  if (rc) return rc;
  const float* proj = (const float*)(sv + L.proj);
  const float* dO = (const float*)(ws + K.dO);
  float* alpha = (float*)(ws + K.alpha);
  float* ds = (float*)(ws + K.ds);
  float* gp = (float*)(ws + K.gp);
  const float scale = 1.f / sqrtf((float)C);
  TR_LAUNCH_GROUP(k_tr_csr_dq, M * H, s, row_ptr, col, proj, d.P, dO, (const float*)(sv + L.m),
                  (const float*)(sv + L.l), alpha, ds, gp, M, H, C, scale)
  if ((rc = gcm_launch_status())) return rc;
  hipLaunchKernelGGL(k_tr_csr_dkv, dim3(blocks(M * H * C, 256)), dim3(256), 0, s, E ? col_ptr : nullptr, rows, perm,
                     (const float*)alpha, (const float*)ds, proj, d.P, dO, gp, M, H, C, scale);
  if ((rc = gcm_launch_status())) return rc;
  return bwd_tail(x, w_all, g_x, g_w_all, g_b_all, K, ws, d, s);
}
