/* gcm_hip_gine.h - the GINE section of the C ABI (csrc/gineconv.hip, in libgcm_hip.so): the aggregation of PyG's
 * GINEConv and of its dense twin with its gradients, and the RelativeEdgeAttr transform.
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GIN section: device pointers only, int return (GCM_EINVAL on null /
 * invalid arguments, GCM_EUNSUPPORTED when F > 128 or D > GCM_GINE_MAX_EDGE_DIM, before any launch), launches on
 * `stream`, no allocation, no host synchronisation and no float atomics: every sum runs in a fixed order, results are
 * bitwise reproducible.  Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same
 * reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * The layer's `nn` is an arbitrary module and stays with the caller; what is here is
 *   e_k     = W_e a_k + b_e   (w_e [F,D], b_e [F]: the layer's `lin`), or a_k itself when w_e is NULL (then D == F)
 *   sparse:  h[i,:]   = (1 + eps) x[i,:] + sum over the edges k = (j -> i) of relu(x[j,:] + e_k)
 *   dense :  h[b,i,:] = s x[b,i,:] + sum over j with adj[b,i,j] != 0 of adj[b,i,j] relu(x[b,j,:] + e[b,i,j,:]),
 *            s = add_loop ? 1 + eps : 0
 * Neither e [E,F] nor the messages [E,F] are ever written to memory: the backward recomputes x_j + e_k and its sign
 * (the derivative of relu at exactly 0 is 0).  No workspace grows with E * F.  eps [1] is a DEVICE pointer read inside
 * the kernels (never on the host: the calls stay HIP-graph capturable).  w_e and b_e are given together or not at all. */
#ifndef GCM_HIP_GINE_H
#define GCM_HIP_GINE_H

#define GCM_GINE_MAX_EDGE_DIM 32

/* Sparse forward over the destination CSR (row_ptr [M+1], col [E] = sources; col may be NULL when E == 0).
 * edge_attr [E,D] is in the order of the caller's edge list: csr_perm [E] is the position of CSR entry p in it, NULL
 * when the list is in CSR order already.  The entries are used as given.  x, h [M,F]. */
int gcm_csr_gine_fwd(const float* x, const float* edge_attr, const float* w_e, const float* b_e, const float* eps,
                     const int64_t* row_ptr, const int64_t* col, const int64_t* csr_perm, float* h, int64_t M,
                     int64_t E, int F, int D, gcm_stream_t stream);

/* Sparse backward.  col_ptr [M+1] / rows [E] / csc_perm [E]: the CSC by source, the sink of each entry and its position
 * in edge_attr's order (all three may be NULL when E == 0 or g_x is NULL).  Outputs (each may be NULL to skip, all
 * overwritten), with delta_k = g_h[sink_k,:] * [x[source_k,:] + e_k > 0]:
 *   g_x [M,F]: g_x[j] = (1 + eps) g_h[j] + sum over the CSC column j of delta_k
 *   g_edge_attr [E,D] in edge_attr's order: W_e^T delta_k (delta_k itself without w_e)
 *   g_w_e [F,D] = sum_k delta_k a_k^T, g_b_e [F] = sum_k delta_k: per workgroup into the workspace, then one pass in
 *   a fixed order;  g_eps [1] = sum <g_h, x> (fp64, fixed order). */
size_t gcm_csr_gine_bwd_workspace_bytes(int64_t M, int64_t E, int F, int D);
int gcm_csr_gine_bwd(const float* g_h, const float* x, const float* edge_attr, const float* w_e, const float* b_e,
                     const float* eps, const int64_t* row_ptr, const int64_t* col, const int64_t* csr_perm,
                     const int64_t* col_ptr, const int64_t* rows, const int64_t* csc_perm, float* g_x,
                     float* g_edge_attr, float* g_w_e, float* g_b_e, float* g_eps, void* workspace,
                     size_t workspace_bytes, int64_t M, int64_t E, int F, int D, gcm_stream_t stream);

/* Dense forward.  x [B,N,F], adj [B,N,N] (adj[b,i,j]: i aggregates from j; the values are weights, the diagonal is an
 * ordinary entry, an entry equal to 0 is no edge), edge_attr [B,N,N,D], read at the set entries only.  `saved` (the
 * workspace query's size) receives the bit image of the pattern for the backward.  B <= 65535, any N. */
size_t gcm_dense_gine_fwd_workspace_bytes(int B, int N, int F, int D);
int gcm_dense_gine_fwd(const float* x, const float* adj, const float* edge_attr, const float* w_e, const float* b_e,
                       const float* eps, float* h, void* saved, size_t saved_bytes, int B, int N, int F, int D,
                       int add_loop, gcm_stream_t stream);

/* Dense backward.  Outputs (each may be NULL to skip, all overwritten):
 *   g_x [B,N,F]; g_edge_attr [B,N,N,D] (zero at the unset entries: the whole tensor is written); g_w_e, g_b_e, g_eps
 *   (0 without add_loop) as above;
 *   g_adj [B,N,N]: g_adj[b,i,j] = <g_h[b,i,:], relu(x[b,j,:] + e[b,i,j,:])> for EVERY entry, also where adj is 0.  Asking
 *   for it makes the row sweep visit all N neighbours of a row: every entry of edge_attr is then read. */
size_t gcm_dense_gine_bwd_workspace_bytes(int B, int N, int F, int D);
int gcm_dense_gine_bwd(const float* g_h, const float* x, const float* adj, const float* edge_attr, const float* w_e,
                       const float* b_e, const float* eps, const void* saved, float* g_x, float* g_adj,
                       float* g_edge_attr, float* g_w_e, float* g_b_e, float* g_eps, void* workspace,
                       size_t workspace_bytes, int B, int N, int F, int D, int add_loop, gcm_stream_t stream);

/* RelativeEdgeAttr, sparse.  edge_index [2,E] = (source, sink); out [E,D], D = (time ? 1 : 0) + P, in edge_index order:
 *   out[k] = [(sink_k - source_k) * time_scale, x[source_k, p0:p0+P] - x[sink_k, p0:p0+P]].  0 <= p0, p0 + P <= F. */
int gcm_rel_edge_attr_fwd(const float* x, const int64_t* edge_index, float* out, int64_t M, int64_t E, int F, int p0,
                          int P, int time, float time_scale, gcm_stream_t stream);

/* Its gradient to x [M,F] (all of it is written; zero outside the pose columns): for node n and pose column p the
 * sum of g_out[k, t + p] over its CSC column (n is the source) minus the sum over its CSR row (n is the sink), each in
 * index order.  row_ptr / csr_perm as in gcm_csr_gine_fwd, col_ptr / csc_perm as in gcm_csr_gine_bwd. */
int gcm_rel_edge_attr_bwd(const float* g_out, const int64_t* row_ptr, const int64_t* csr_perm, const int64_t* col_ptr,
                          const int64_t* csc_perm, float* g_x, int64_t M, int64_t E, int F, int p0, int P, int time,
                          gcm_stream_t stream);

/* RelativeEdgeAttr, dense: out [B,N,N,D], out[b,i,j] = [(i - j) * time_scale, x[b,j,p0:p0+P] - x[b,i,p0:p0+P]] for
 * every entry; g_x[b,n,p0+p] = sum_i g_out[b,i,n,t+p] - sum_j g_out[b,n,j,t+p] (column sums minus row sums). */
int gcm_dense_rel_edge_attr_fwd(const float* x, float* out, int B, int N, int F, int p0, int P, int time,
                                float time_scale, gcm_stream_t stream);
int gcm_dense_rel_edge_attr_bwd(const float* g_out, float* g_x, int B, int N, int F, int p0, int P, int time,
                                gcm_stream_t stream);

#endif /* GCM_HIP_GINE_H */
