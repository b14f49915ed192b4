/* gcm_hip_tag.h - the TAGConv section of the C ABI (csrc/tagconv.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GatedGraphConv section: device pointers only, int return
 * (GCM_EINVAL on null / invalid arguments; GCM_EUNSUPPORTED when Fi or Fo > 128), launches on `stream`, no
 * allocation, no host synchronisation and no float atomics: every sum runs in a fixed order, results are bitwise
 * reproducible.  Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as
 * gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * The layer (PyG's TAGConv, Du et al.), rows R = B*N (dense) or M (sparse), K >= 0 hops:
 *   h_0 = x [R,Fi];   h_k = A^ h_{k-1};   out = sum_{k=0..K} h_k weight[k]^T + bias      weight [K+1,Fo,Fi], bias [Fo]
 *   A^ = D^-1/2 A D^-1/2 with deg_i = sum_j A_ij (the weights INTO node i) and d_i = deg_i^-1/2, 0 where deg_i == 0,
 *   when `normalize`; A^ = A otherwise.  No loop is added or removed (sparse); add_loop overwrites the diagonal with 1
 *   before the degrees are taken (dense).
 *
 * `saved` is written by the forward and read by the backward; its size is the forward's workspace query:
 *   dense   4 * (K * R * Fi + R) bytes: h_1 .. h_K [K,R,Fi], then d [R]
 *   sparse  4 * K * M * Fi bytes (at least 256): h_1 .. h_K [K,M,Fi]
 * The queries return 0 for an empty problem (a dimension <= 0; K < 0). */
#ifndef GCM_HIP_TAG_H
#define GCM_HIP_TAG_H

/* Dense: adj [B,N,N], adj[b,i,j]: the weight of the edge j -> i.  x [B,N,Fi], out [B,N,Fo].  B <= 65535, any N.
 * N <= 128 runs every hop in ONE launch, one workgroup per graph (the adjacency is read once, the degrees are taken
 * in the same launch); a larger N takes one launch per hop. */
size_t gcm_dense_tagconv_fwd_workspace_bytes(int B, int N, int Fi, int K);
int gcm_dense_tagconv_fwd(const float* x, const float* adj, const float* weight, const float* bias, float* out,
                          void* saved, size_t saved_bytes, int B, int N, int Fi, int Fo, int K, int normalize,
                          int add_loop, gcm_stream_t stream);

/* Backward of the above.  Outputs (each may be NULL to skip, all overwritten): g_x [B,N,Fi], g_adj [B,N,N], g_weight
 * [K+1,Fo,Fi], g_bias [Fo].
 *   r_K = g weight[K];  r_k = g weight[k] + A^^T r_{k+1};  g_x = r_0;  g_weight[k] = g^T h_k
 *   g_adj[b,i,j] = d_i d_j sum_{k=1..K} <r_k[b,i,:], h_{k-1}[b,j,:]> + the degree term of row i, for EVERY entry, also
 *   where adj is 0; the diagonal is 0 when add_loop. */
size_t gcm_dense_tagconv_bwd_workspace_bytes(int B, int N, int Fi, int Fo, int K);
int gcm_dense_tagconv_bwd(const float* g_out, const float* x, const float* adj, const float* weight, const void* saved,
                          float* g_x, float* g_adj, float* g_weight, float* g_bias, void* workspace,
                          size_t workspace_bytes, int B, int N, int Fi, int Fo, int K, int normalize, int add_loop,
                          gcm_stream_t stream);

/* Sparse: destination CSR (row_ptr [M+1], col [E] = sources), coef [E] in CSR order: the coefficients c_e of
 * gcm_gcn_norm(normalize, add_self_loops = 0).  col and coef may be NULL when E == 0.  x [M,Fi], out [M,Fo].  One
 * launch per hop: the gather of h_k and h_k weight[k]^T accumulated into out. */
size_t gcm_csr_tagconv_fwd_workspace_bytes(int64_t M, int Fi, int K);
int gcm_csr_tagconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* coef,
                        const float* weight, const float* bias, float* out, void* saved, size_t saved_bytes, int64_t M,
                        int64_t E, int Fi, int Fo, int K, gcm_stream_t stream);

/* Backward.  dst [E]: the sink of each CSR entry; col_ptr [M+1] / rows [E] / perm [E]: the CSC by source (entry k of
 * the CSC is CSR entry perm[k]); all may be NULL when E == 0.  dinv [M]: gcm_gcn_norm's d.  Outputs (NULL to skip) as
 * the dense backward's, with g_edge_weight [E] (CSR order) in the place of g_adj:
 *   g_edge_weight[e] = d_src d_dst sum_k <r_k[dst], h_{k-1}[src]> + the degree term of dst   (normalize)
 *                    = sum_k <r_k[dst], h_{k-1}[src]>                                        (otherwise). */
size_t gcm_csr_tagconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int Fo, int K);
int gcm_csr_tagconv_bwd(const float* g_out, const float* x, const int64_t* row_ptr, const int64_t* col,
                        const int64_t* dst, const int64_t* col_ptr, const int64_t* rows, const int64_t* perm,
                        const float* coef, const float* dinv, const float* weight, const void* saved, float* g_x,
                        float* g_edge_weight, float* g_weight, float* g_bias, void* workspace, size_t workspace_bytes,
                        int64_t M, int64_t E, int Fi, int Fo, int K, int normalize, gcm_stream_t stream);

#endif /* GCM_HIP_TAG_H */
