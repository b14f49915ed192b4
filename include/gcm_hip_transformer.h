/* gcm_hip_transformer.h - the TransformerConv section of the C ABI (csrc/transformerconv.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GAT section there: device pointers only, int return (GCM_EINVAL on
 * null / invalid arguments, GCM_EUNSUPPORTED when Fi or H*C > 128), launches on `stream`, no allocation, no host
 * synchronisation and no float atomics: results are bitwise reproducible.  Additive: GCM_ABI_VERSION is unchanged.
 * The Python binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * The layer (PyG's TransformerConv without edge features), rows R = B*N (dense) or M (sparse), D = H*C if concat else C:
 *   [q | k | v | r] = x W_all^T + b_all,  W_all [P,Fi] = [W_query; W_key; W_value; W_skip] stacked, P = 3 H C + (root ? D : 0)
 *   s[i,j,h] = <q[i,h,:], k[j,h,:]> / sqrt(C) over the in-neighbours j of i, alpha = softmax_j(s)
 *   o[i,h,:] = sum_j alpha[i,j,h] v[j,h,:]  (0 for a row without a neighbour),  om = concat_h(o) or mean_h(o)
 *   w_beta [3 D] given (root only): g = sigmoid(<w_beta, [om, r, om - r]>), out = g r + (1 - g) om
 *   else: out = om + r (root) or om
 * `saved` is written by the forward and read by the backward ([q|k|v|r], o, the softmax row statistics, the gate and,
 * dense, the bit image of the pattern); its size is the forward's workspace query. */
#ifndef GCM_HIP_TRANSFORMER_H
#define GCM_HIP_TRANSFORMER_H

/* Dense: adj [B,N,N], adj[b,i,j] != 0: i attends to j (only the pattern is read; the diagonal counts as set when
 * add_loop).  x [B,N,Fi], out [B,N,D].  B <= 65535, any N. */
size_t gcm_dense_transformerconv_fwd_workspace_bytes(int B, int N, int Fi, int H, int C, int concat, int root);
int gcm_dense_transformerconv_fwd(const float* x, const float* adj, const float* w_all, const float* b_all,
                                  const float* w_beta, float* out, void* saved, size_t saved_bytes, int B, int N,
                                  int Fi, int H, int C, int concat, int root, int add_loop, gcm_stream_t stream);

/* Backward of the above (the adjacency gets no gradient).  Outputs (each may be NULL to skip, all overwritten): g_x
 * [B,N,Fi], g_w_all [P,Fi], g_b_all [P], g_w_beta [3 D] (NULL without w_beta). */
size_t gcm_dense_transformerconv_bwd_workspace_bytes(int B, int N, int Fi, int H, int C, int concat, int root);
int gcm_dense_transformerconv_bwd(const float* g_out, const float* x, const float* w_all, const float* w_beta,
                                  const void* saved, float* g_x, float* g_w_all, float* g_b_all, float* g_w_beta,
                                  void* workspace, size_t workspace_bytes, int B, int N, int Fi, int H, int C,
                                  int concat, int root, gcm_stream_t stream);

/* Sparse: destination CSR (row_ptr [M+1], col [E] = sources; col may be NULL when E == 0).  The entries are used as
 * given: no loop is added or removed, duplicates are separate terms of the softmax.  x [M,Fi], out [M,D]. */
size_t gcm_csr_transformerconv_fwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int concat, int root);
int gcm_csr_transformerconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* w_all,
                                const float* b_all, const float* w_beta, float* out, void* saved, size_t saved_bytes,
                                int64_t M, int64_t E, int Fi, int H, int C, int concat, int root,
                                gcm_stream_t stream);

/* Backward.  col_ptr/rows/perm: the CSC by source as for gcm_csr_graphconv_bwd (may be NULL when E == 0).  Outputs
 * (NULL to skip) as the dense backward's. */
size_t gcm_csr_transformerconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int concat, int root);
int gcm_csr_transformerconv_bwd(const float* g_out, const float* x, const int64_t* row_ptr, const int64_t* col,
                                const int64_t* col_ptr, const int64_t* rows, const int64_t* perm, const float* w_all,
                                const float* w_beta, const void* saved, float* g_x, float* g_w_all, float* g_b_all,
                                float* g_w_beta, void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int Fi,
                                int H, int C, int concat, int root, gcm_stream_t stream);

#endif /* GCM_HIP_TRANSFORMER_H */
