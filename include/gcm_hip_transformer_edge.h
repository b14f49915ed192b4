/* gcm_hip_transformer_edge.h - TransformerConv with edge features (PyG's edge_dim) and its dense twin
 * (csrc/transformer_edge.hip, in libgcm_hip.so), forward and backward.
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the TransformerConv section (gcm_hip_transformer.h): device pointers
 * only, int return (GCM_EINVAL on null / invalid arguments, GCM_EUNSUPPORTED when Fi > 128, H * C > 128 or
 * D > GCM_TRE_MAX_EDGE_DIM, before any launch), launches on `stream`, no allocation, no host synchronisation and no
 * float atomics: every sum runs in a fixed order, results are bitwise reproducible.  Additive: GCM_ABI_VERSION is
 * unchanged.  The Python binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * The layer is gcm_hip_transformer.h's with, for a term k = (j -> i) whose edge feature is a_k [D] and
 * e_k = W_e a_k viewed [H,C] (w_e [H*C, D], no bias):
 *   s_k[h] = <q_i[h], k_j[h] + e_k[h]> / sqrt(C),  alpha = softmax of s over the terms of i
 *   o_i[h] = sum_k alpha_k[h] (v_j[h] + e_k[h])
 * computed in the factored form, in which nothing per term is wider than D:
 *   u_i[h] = W_e[h]^T q_i[h] / sqrt(C)  [rows,H,D],  s_k[h] = <q_i[h], k_j[h]> / sqrt(C) + <u_i[h], a_k>
 *   abar_i[h] = sum_k alpha_k[h] a_k  [rows,H,D],     o_i[h] = sum_k alpha_k[h] v_j[h] + W_e[h] abar_i[h]
 * No e_k, no key k_j + e_k, no message v_j + e_k and (dense) no score is written to memory.  `saved` holds what the
 * edge-free forward saves plus u and abar; its size is the forward's workspace query. */
#ifndef GCM_HIP_TRANSFORMER_EDGE_H
#define GCM_HIP_TRANSFORMER_EDGE_H

#define GCM_TRE_MAX_EDGE_DIM 32

/* Sparse forward over the destination CSR (row_ptr [M+1], col [E] = sources; col may be NULL when E == 0).  edge_attr
 * [E,D] is in the order of the caller's edge list: csr_perm [E] is the position of CSR entry p in it, NULL when the
 * list is in CSR order already.  The entries are used as given.  x [M,Fi], out [M, H*C or C]. */
size_t gcm_csr_transformer_edge_fwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int D, int concat,
                                                    int root);
int gcm_csr_transformer_edge_fwd(const float* x, const float* edge_attr, const int64_t* row_ptr, const int64_t* col,
                                 const int64_t* csr_perm, const float* w_all, const float* b_all, const float* w_e,
                                 const float* w_beta, float* out, void* saved, size_t saved_bytes, int64_t M,
                                 int64_t E, int Fi, int H, int C, int D, int concat, int root, gcm_stream_t stream);

/* Sparse backward.  col_ptr / rows / perm: the CSC by source as for gcm_csr_transformerconv_bwd (entry k of the CSC is
 * CSR entry perm[k]; may be NULL when E == 0).  Outputs (each may be NULL to skip, all overwritten): g_x [M,Fi],
 * g_w_all [P,Fi], g_b_all [P], g_w_e [H*C,D], g_w_beta [3 Do] (NULL without w_beta), g_edge_attr [E,D] in edge_attr's
 * order. */
size_t gcm_csr_transformer_edge_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int D, int concat,
                                                    int root);
int gcm_csr_transformer_edge_bwd(const float* g_out, const float* x, const float* edge_attr, const int64_t* row_ptr,
                                 const int64_t* col, const int64_t* csr_perm, const int64_t* col_ptr,
                                 const int64_t* rows, const int64_t* perm, const float* w_all, const float* w_e,
                                 const float* w_beta, const void* saved, float* g_x, float* g_w_all, float* g_b_all,
                                 float* g_w_e, float* g_w_beta, float* g_edge_attr, void* workspace,
                                 size_t workspace_bytes, int64_t M, int64_t E, int Fi, int H, int C, int D, int concat,
                                 int root, gcm_stream_t stream);

/* Dense forward.  adj [B,N,N], adj[b,i,j] != 0: i attends to j (only the pattern is read; the diagonal counts as set
 * when add_loop, and its feature is edge_attr[b,i,i]).  edge_attr [B,N,N,D] is read at the terms only: the other
 * entries may hold anything.  x [B,N,Fi], out [B,N, H*C or C].  B <= 65535, any N. */
size_t gcm_dense_transformer_edge_fwd_workspace_bytes(int B, int N, int Fi, int H, int C, int D, int concat, int root);
int gcm_dense_transformer_edge_fwd(const float* x, const float* adj, const float* edge_attr, const float* w_all,
                                   const float* b_all, const float* w_e, const float* w_beta, float* out, void* saved,
                                   size_t saved_bytes, int B, int N, int Fi, int H, int C, int D, int concat, int root,
                                   int add_loop, gcm_stream_t stream);

/* Dense backward (the adjacency gets no gradient).  Outputs as the sparse backward's; g_edge_attr [B,N,N,D] is written
 * whole: zero where there is no term. */
size_t gcm_dense_transformer_edge_bwd_workspace_bytes(int B, int N, int Fi, int H, int C, int D, int concat, int root);
int gcm_dense_transformer_edge_bwd(const float* g_out, const float* x, const float* edge_attr, const float* w_all,
                                   const float* w_e, const float* w_beta, const void* saved, float* g_x,
                                   float* g_w_all, float* g_b_all, float* g_w_e, float* g_w_beta, float* g_edge_attr,
                                   void* workspace, size_t workspace_bytes, int B, int N, int Fi, int H, int C, int D,
                                   int concat, int root, gcm_stream_t stream);

#endif /* GCM_HIP_TRANSFORMER_EDGE_H */
