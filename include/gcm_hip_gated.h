/* gcm_hip_gated.h - the GatedGraphConv section of the C ABI (csrc/gatedgraphconv.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the ResGatedGraphConv section: device pointers only, int return
 * (GCM_EINVAL on null / invalid arguments, Fi > C among them; GCM_EUNSUPPORTED when C > 128), launches on `stream`, no
 * allocation, no host synchronisation and no float atomics: every sum runs in a fixed order, results are bitwise
 * reproducible.  Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as
 * gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * The layer (PyG's GatedGraphConv, aggr "add"), rows R = B*N (dense) or M (sparse), L rounds:
 *   h_0 = x [R,Fi] zero-padded on the right to C columns (Fi <= C)
 *   m   = A (h_l weight[l])        weight [L,C,C], NOT transposed; A: adj (dense) or the weighted edge list (sparse)
 *   gi  = m w_ih^T + b_ih,  gh = h_l w_hh^T + b_hh      w_ih, w_hh [3C,C], b_ih, b_hh [3C] or NULL; gate order r, z, n
 *   r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n),  h_{l+1} = (1 - z) n + z h_l
 *   out = h_L [R,C]
 * (torch.nn.GRUCell's parameters as they are.)
 *
 * `saved` is written by the forward and read by the backward.  Its size is the forward's workspace query, exactly
 *   4 * (6 * L * R * C  +  R * ceil(N / 32))  bytes dense,     4 * 6 * L * R * C  bytes sparse:
 * six [L,R,C] float tensors - h_l, m_l, r, z, n and gh_n (bias included) of every round - and, dense, the bit image of
 * the pattern, one word per 32 neighbours of a row.  Nothing of size [B,N,N,.] is kept.  The queries return 0 for an
 * empty batch (a dimension <= 0). */
#ifndef GCM_HIP_GATED_H
#define GCM_HIP_GATED_H

/* Dense: adj [B,N,N], adj[b,i,j]: the weight of the edge j -> i; an entry equal to 0 is no edge and is skipped; with
 * add_loop the diagonal counts as 1 whatever it holds.  x [B,N,Fi], out [B,N,C].  B <= 65535, any N. */
size_t gcm_dense_gatedgraphconv_fwd_workspace_bytes(int B, int N, int C, int L);
int gcm_dense_gatedgraphconv_fwd(const float* x, const float* adj, const float* weight, const float* w_ih,
                                 const float* w_hh, const float* b_ih, const float* b_hh, float* out, void* saved,
                                 size_t saved_bytes, int B, int N, int Fi, int C, int L, int add_loop,
                                 gcm_stream_t stream);

/* Backward of the above.  Outputs (each may be NULL to skip, all overwritten): g_x [B,N,Fi] (the first Fi columns of
 * the gradient of h_0), g_weight [L,C,C], g_w_ih, g_w_hh [3C,C], g_b_ih, g_b_hh [3C] (sums over all rounds), g_adj
 * [B,N,N].
 *   g_adj[b,i,j] = sum_l <g_m_l[b,i,:], (h_l weight[l])[b,j,:]>  for EVERY entry, also where adj is 0 (the derivative
 *   there is not 0), with the diagonal 0 when add_loop. */
size_t gcm_dense_gatedgraphconv_bwd_workspace_bytes(int B, int N, int C, int L);
int gcm_dense_gatedgraphconv_bwd(const float* g_out, const float* adj, const float* weight, const float* w_ih,
                                 const float* w_hh, const void* saved, float* g_x, float* g_weight, float* g_w_ih,
                                 float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_adj, void* workspace,
                                 size_t workspace_bytes, int B, int N, int Fi, int C, int L, int add_loop,
                                 gcm_stream_t stream);

/* Sparse: destination CSR (row_ptr [M+1], col [E] = sources; col may be NULL when E == 0), edge_weight [E] in CSR
 * order or NULL (every weight 1).  The entries are used as given: no loop is added or removed, duplicates are separate
 * terms.  x [M,Fi], out [M,C]. */
size_t gcm_csr_gatedgraphconv_fwd_workspace_bytes(int64_t M, int64_t E, int C, int L);
int gcm_csr_gatedgraphconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* edge_weight,
                               const float* weight, const float* w_ih, const float* w_hh, const float* b_ih,
                               const float* b_hh, float* out, void* saved, size_t saved_bytes, int64_t M, int64_t E,
                               int Fi, int C, int L, gcm_stream_t stream);

/* Backward.  col_ptr [M+1] / rows [E] / perm [E]: the CSC by source (sink of each entry; entry k of the CSC is CSR
 * entry perm[k], needed with edge_weight only); all may be NULL when E == 0.  Outputs (NULL to skip) as the dense
 * backward's, with g_edge_weight [E] (CSR order; needs edge_weight) in the place of g_adj. */
size_t gcm_csr_gatedgraphconv_bwd_workspace_bytes(int64_t M, int64_t E, int C, int L);
int gcm_csr_gatedgraphconv_bwd(const float* g_out, const int64_t* row_ptr, const int64_t* col, const int64_t* col_ptr,
                               const int64_t* rows, const int64_t* perm, const float* edge_weight, const float* weight,
                               const float* w_ih, const float* w_hh, const void* saved, float* g_x, float* g_weight,
                               float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh, float* g_edge_weight,
                               void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int Fi, int C, int L,
                               gcm_stream_t stream);

#endif /* GCM_HIP_GATED_H */
