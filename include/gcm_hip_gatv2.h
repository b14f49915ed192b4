/* gcm_hip_gatv2.h - the GATv2 section of the C ABI (csrc/gatv2conv.hip, in libgcm_hip.so): PyG's GATv2Conv with
 * edge_dim, and its dense twin, forward and backward.
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GAT and GINE sections: device pointers only, int return
 * (GCM_EINVAL on null / invalid arguments, GCM_EUNSUPPORTED when Fi > 128, H * C > 128 or D > GCM_GATV2_MAX_EDGE_DIM,
 * before any launch), launches on `stream`, no allocation, no host synchronisation and no float atomics: every sum
 * runs in a fixed order, results are bitwise reproducible.  Additive: GCM_ABI_VERSION is unchanged.  The Python
 * binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 *   x_l = x W_l^T + b_l,  x_r = x W_r^T + b_r   viewed [rows, H, C]   (w_r NULL: shared weights, x_r = x_l)
 *   for a term k = (j -> i):  z_k = x_l[j] + x_r[i] (+ W_e a_k),  s_k[h] = sum_c att[h,c] leaky_relu(z_k[h,c])
 *   alpha = softmax of s over the terms of i;  o[i,h,:] = sum_k alpha_k[h] x_l[j,h,:]
 *   out = concat_h(o) + bias, or mean_h(o) + bias.  A row without a term: o = 0, out = bias.
 * The derivative of leaky_relu at exactly 0 is negative_slope.
 * Nothing per edge is written by the forward: no z, no W_e a_k, no scores, no messages.  It saves x_l, x_r and the
 * softmax's per-row maximum and sum; the backward recomputes z and alpha from those.
 * w_l, w_r [H*C, Fi]; b_l, b_r [H*C] or NULL; att [H*C]; w_e [H*C, D] or NULL (then D == 0 and edge_attr is not read);
 * bias [H*C] (concat) or [C], or NULL.
 * Loop terms (add_self_loops / add_loop): every i -> i entry is skipped in place and row i gets one term (i -> i) after
 * its entries, whose edge feature is fill_value in every column, or with fill_mean != 0 the mean of the features of
 * the row's remaining entries (zero when it has none). */
#ifndef GCM_HIP_GATV2_H
#define GCM_HIP_GATV2_H

#define GCM_GATV2_MAX_EDGE_DIM 32

/* Sparse forward over the destination CSR (row_ptr [M+1], col [E] = sources; col may be NULL when E == 0).  edge_attr
 * [E,D] is in the order of the caller's edge list: csr_perm [E] is the position of CSR entry p in it, NULL when the list
 * is in CSR order already.  x [M,Fi]; out [M,H*C] or [M,C].  Saved for the backward: xl, xr [M,H*C] (xr may be NULL
 * when w_r is), row_m (-inf for a row without a term), row_l [M,H].  workspace: the per-head aggregate when !concat. */
size_t gcm_csr_gatv2_fwd_workspace_bytes(int64_t M, int H, int C, int concat);
int gcm_csr_gatv2_fwd(const float* x, const float* w_l, const float* b_l, const float* w_r, const float* b_r,
                      const float* att, const float* w_e, const float* bias, const float* edge_attr,
                      const int64_t* row_ptr, const int64_t* col, const int64_t* csr_perm, float* out, float* xl,
                      float* xr, float* row_m, float* row_l, void* workspace, size_t workspace_bytes, int64_t M,
                      int64_t E, int Fi, int H, int C, int D, int concat, int add_self_loops, int fill_mean,
                      float fill_value, float negative_slope, gcm_stream_t stream);

/* Sparse backward.  col_ptr [M+1] / rows [E] / csc_perm [E]: the CSC by source, the sink of each entry and its position
 * in edge_attr's order (may be NULL when E == 0, or when none of g_x, g_w_l, g_b_l is asked for).  Outputs (each may be
 * NULL to skip, all overwritten): g_x [M,Fi]; g_w_l, g_w_r [H*C,Fi]; g_b_l, g_b_r [H*C] (with shared weights g_w_r and
 * g_b_r must be NULL and g_w_l / g_b_l receive the sum of both uses); g_att [H*C]; g_w_e [H*C,D]; g_edge_attr [E,D] in
 * edge_attr's order (the share that reaches it through a mean loop feature included; zero at skipped i -> i entries);
 * g_bias. */
size_t gcm_csr_gatv2_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int D, int concat);
int gcm_csr_gatv2_bwd(const float* g_out, const float* x, const float* w_l, const float* w_r, const float* att,
                      const float* w_e, const float* edge_attr, const int64_t* row_ptr, const int64_t* col,
                      const int64_t* csr_perm, const int64_t* col_ptr, const int64_t* rows, const int64_t* csc_perm,
                      const float* xl, const float* xr, const float* row_m, const float* row_l, float* g_x,
                      float* g_w_l, float* g_b_l, float* g_w_r, float* g_b_r, float* g_att, float* g_w_e,
                      float* g_edge_attr, float* g_bias, void* workspace, size_t workspace_bytes, int64_t M, int64_t E,
                      int Fi, int H, int C, int D, int concat, int add_self_loops, int fill_mean, float fill_value,
                      float negative_slope, gcm_stream_t stream);

/* Dense forward.  x [B,N,Fi], adj [B,N,N] (adj[b,i,j] != 0: i attends to j; only the pattern is read, once, into
 * `bits` [B,N,ceil(N/32)], which the backward reads too), edge_attr [B,N,N,D], read at the set entries only.  With
 * add_loop the diagonal is a term whether or not it is set in adj, and its feature is the fill.  B <= 65535, any N. */
size_t gcm_dense_gatv2_fwd_workspace_bytes(int B, int N, int H, int C, int concat);
int gcm_dense_gatv2_fwd(const float* x, const float* adj, const float* w_l, const float* b_l, const float* w_r,
                        const float* b_r, const float* att, const float* w_e, const float* bias,
                        const float* edge_attr, float* out, float* xl, float* xr, float* row_m, float* row_l,
                        unsigned* bits, void* workspace, size_t workspace_bytes, int B, int N, int Fi, int H, int C,
                        int D, int concat, int add_loop, int fill_mean, float fill_value, float negative_slope,
                        gcm_stream_t stream);

/* Dense backward (the adjacency gets no gradient).  Outputs as the sparse backward's; g_edge_attr [B,N,N,D] is written
 * whole: zero at the unset entries (and at the diagonal with add_loop). */
size_t gcm_dense_gatv2_bwd_workspace_bytes(int B, int N, int Fi, int H, int C, int D, int concat);
int gcm_dense_gatv2_bwd(const float* g_out, const float* x, const float* w_l, const float* w_r, const float* att,
                        const float* w_e, const float* edge_attr, const unsigned* bits, const float* xl,
                        const float* xr, const float* row_m, const float* row_l, float* g_x, float* g_w_l,
                        float* g_b_l, float* g_w_r, float* g_b_r, float* g_att, float* g_w_e, float* g_edge_attr,
                        float* g_bias, void* workspace, size_t workspace_bytes, int B, int N, int Fi, int H, int C,
                        int D, int concat, int add_loop, int fill_mean, float fill_value, float negative_slope,
                        gcm_stream_t stream);

#endif /* GCM_HIP_GATV2_H */
