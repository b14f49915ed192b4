/* gcm_hip_aggr.h - the mean / max aggregation section of the C ABI (csrc/aggrconv.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GCN / GAT sections there: device pointers only, a
 * *_bwd_workspace_bytes query per backward, int return (GCM_EINVAL on null / invalid arguments, GCM_EUNSUPPORTED when
 * Fi or Fo > 128), launches on `stream`, no allocation and no host synchronisation.  Additive: GCM_ABI_VERSION is
 * unchanged.  The Python binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py). */
#ifndef GCM_HIP_AGGR_H
#define GCM_HIP_AGGR_H

#define GCM_AGGR_MEAN 1
#define GCM_AGGR_MAX 2

/* Dense: out = agg W_rel^T + x W_root^T + bias, adj[b,i,j]: i aggregates from j.
 *   GCM_AGGR_MEAN: agg_i = (sum_j adj_ij x_j) / max(sum_j adj_ij, 1)   (adj values are weights)
 *   GCM_AGGR_MAX:  agg_ic = max over {j : adj_ij != 0} of x_jc, 0 for a row without a neighbour; the lowest j
 *                  wins a tie (only the pattern of adj is read)
 * x [B,N,Fi], adj [B,N,N], w_rel [Fo,Fi], w_root [Fo,Fi] or NULL (no root term), bias [Fo] or NULL, out [B,N,Fo].
 * Saved for the backward: agg [B,N,Fi] (required); mean: deg = rowsum(adj) before the clamp and dinv = 1 / max(deg, 1)
 * [B,N]; max: winner [B,N,Fi], the winning j or -1.  Fi, Fo <= 128, N <= 32767; GCM_EUNSUPPORTED otherwise. */
int gcm_dense_aggrconv_fwd(const float* x, const float* adj, const float* w_rel, const float* w_root,
                           const float* bias, float* out, float* agg, float* deg, float* dinv, int16_t* winner,
                           int B, int N, int Fi, int Fo, int aggr, gcm_stream_t stream);

/* Backward of the above.  Outputs (each may be NULL to skip, all overwritten): g_x [B,N,Fi]; g_adj [B,N,N], mean only
 * (dinv_i <dAgg_i, x_j> plus the degree term of row i on every entry, the clamp passing the gradient at rowsum == 1;
 * must be NULL for max); g_w_rel, g_w_root [Fo,Fi]; g_bias [Fo]. */
size_t gcm_dense_aggrconv_bwd_workspace_bytes(int B, int N, int Fi, int Fo);
int gcm_dense_aggrconv_bwd(const float* g_out, const float* x, const float* adj, const float* w_rel,
                           const float* w_root, const float* agg, const float* deg, const float* dinv,
                           const int16_t* winner, float* g_x, float* g_adj, float* g_w_rel, float* g_w_root,
                           float* g_bias, void* workspace, size_t workspace_bytes, int B, int N, int Fi, int Fo,
                           int aggr, gcm_stream_t stream);

/* Sparse: the same layer over a destination CSR (row_ptr [M+1], col [E] = sources, w_edge [E] in CSR order or NULL =
 * unit weights).
 *   GCM_AGGR_MEAN: agg_i = (sum_{e -> i} w_e x_src(e)) / #{e -> i}     (the entry count, not the weight sum)
 *   GCM_AGGR_MAX:  agg_ic = max over e -> i of w_e x_src(e),c; the first CSR entry wins a tie; duplicates compete
 * A node without an entry aggregates 0.  x [M,Fi], out [M,Fo], agg [M,Fi] (required); max: winner [M,Fi], the winning
 * CSR entry or -1.  Fi, Fo <= 128, E < 2^31. */
int gcm_csr_aggrconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* w_edge,
                         const float* w_rel, const float* w_root, const float* bias, float* out, float* agg,
                         int32_t* winner, int64_t M, int64_t E, int Fi, int Fo, int aggr, gcm_stream_t stream);

/* Backward.  dst [E]: the row of every CSR entry; col_ptr/rows/perm: the CSC by source as for gcm_csr_graphconv_bwd
 * (may be NULL when E == 0).  Outputs (NULL to skip): g_x [M,Fi], g_edge [E] (CSR order; max: through the channels the
 * entry won), g_w_rel, g_w_root [Fo,Fi], g_bias [Fo]. */
size_t gcm_csr_aggrconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int Fo);
int gcm_csr_aggrconv_bwd(const float* g_out, const float* x, const float* agg, const int64_t* row_ptr,
                         const int64_t* col, const int64_t* dst, const int64_t* col_ptr, const int64_t* rows,
                         const int64_t* perm, const float* w_edge, const int32_t* winner, const float* w_rel,
                         const float* w_root, float* g_x, float* g_edge, float* g_w_rel, float* g_w_root,
                         float* g_bias, void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int Fi, int Fo,
                         int aggr, gcm_stream_t stream);

#endif /* GCM_HIP_AGGR_H */
