/* gcm_hip_resgated.h - the ResGatedGraphConv section of the C ABI (csrc/resgatedconv.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the TransformerConv section: device pointers only, int return
 * (GCM_EINVAL on null / invalid arguments, GCM_EUNSUPPORTED when Fi or C > 128), launches on `stream`, no allocation,
 * no host synchronisation and no float atomics: every sum runs in a fixed order, results are bitwise reproducible.
 * Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as gcm_hip.h
 * (gcm/_abi.py, gcm/_hip.py).
 *
 * The layer (PyG's ResGatedGraphConv without edge features), rows R = B*N (dense) or M (sparse):
 *   [k | q | v | r] = x W_all^T + b_all,  W_all [P,Fi] = [W_key; W_query; W_value; W_skip] stacked, P = 3 C + (root ? C : 0);
 *                     the skip has no bias: its slots of b_all are zero
 *   out[i,:] = r[i,:] + sum over the in-neighbours j of i of a_ij sigmoid(k[i,:] + q[j,:]) * v[j,:] + bias
 *   (a_ij: the adjacency value, dense; 1 per edge, sparse.  r = 0 without root, bias may be NULL.)
 * The gates are never stored: the backward recomputes them.  `saved` is written by the forward and read by the
 * backward and holds [k|q|v|r] [R,P] and, dense, the bit image of the pattern - nothing else; its size is the forward's
 * workspace query. */
#ifndef GCM_HIP_RESGATED_H
#define GCM_HIP_RESGATED_H

/* Dense: adj [B,N,N], adj[b,i,j]: the weight of the edge j -> i; an entry equal to 0 is no edge and is skipped; with
 * add_loop the diagonal counts as 1 whatever it holds.  x [B,N,Fi], out [B,N,C].  B <= 65535, any N. */
size_t gcm_dense_resgatedconv_fwd_workspace_bytes(int B, int N, int Fi, int C, int root);
int gcm_dense_resgatedconv_fwd(const float* x, const float* adj, const float* w_all, const float* b_all,
                               const float* bias, float* out, void* saved, size_t saved_bytes, int B, int N, int Fi,
                               int C, int root, int add_loop, gcm_stream_t stream);

/* Backward of the above.  Outputs (each may be NULL to skip, all overwritten): g_x [B,N,Fi], g_w_all [P,Fi], g_b_all
 * [P], g_bias [C] (the column sums of g_out), g_adj [B,N,N].
 *   g_adj[b,i,j] = sum_c g_out[b,i,c] sigmoid(k[b,i,c] + q[b,j,c]) v[b,j,c]  for EVERY entry, also where adj is 0 (the
 *   derivative there is not 0), with the diagonal 0 when add_loop.  Asking for it makes the row sweep visit all N
 *   neighbours of a row instead of the set bits only. */
size_t gcm_dense_resgatedconv_bwd_workspace_bytes(int B, int N, int Fi, int C, int root);
int gcm_dense_resgatedconv_bwd(const float* g_out, const float* x, const float* adj, const float* w_all,
                               const void* saved, float* g_x, float* g_w_all, float* g_b_all, float* g_bias,
                               float* g_adj, void* workspace, size_t workspace_bytes, int B, int N, int Fi, int C,
                               int root, int add_loop, gcm_stream_t stream);

/* Sparse: destination CSR (row_ptr [M+1], col [E] = sources; col may be NULL when E == 0).  The entries are used as
 * given: no loop is added or removed, duplicates count once each.  x [M,Fi], out [M,C]. */
size_t gcm_csr_resgatedconv_fwd_workspace_bytes(int64_t M, int64_t E, int Fi, int C, int root);
int gcm_csr_resgatedconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* w_all,
                             const float* b_all, const float* bias, float* out, void* saved, size_t saved_bytes,
                             int64_t M, int64_t E, int Fi, int C, int root, gcm_stream_t stream);

/* Backward.  col_ptr [M+1] / rows [E]: the CSC by source (sink of each entry), may be NULL when E == 0; no per-edge
 * value is kept, so the CSC's permutation is not needed.  Outputs (NULL to skip) as the dense backward's. */
size_t gcm_csr_resgatedconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int C, int root);
int gcm_csr_resgatedconv_bwd(const float* g_out, const float* x, const int64_t* row_ptr, const int64_t* col,
                             const int64_t* col_ptr, const int64_t* rows, const float* w_all, const void* saved,
                             float* g_x, float* g_w_all, float* g_b_all, float* g_bias, void* workspace,
                             size_t workspace_bytes, int64_t M, int64_t E, int Fi, int C, int root,
                             gcm_stream_t stream);

#endif /* GCM_HIP_RESGATED_H */
