/* gcm_hip_rgcn.h - the relational section of the C ABI (csrc/rgcnconv.hip, in libgcm_hip.so): RGCNConv /
 * DenseRGCNConv and the merge of the TypedEdge selector.
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GCN section there: device pointers only (gcm_typed_merge's two
 * small HOST arrays are the one exception, named below), int return (GCM_EINVAL on null / invalid arguments,
 * GCM_EUNSUPPORTED when Fi or Fo > 128 or R > 16, GCM_EWORKSPACE), launches on `stream`, no allocation, no host
 * synchronisation and no float atomics: results are bitwise reproducible.  Additive: GCM_ABI_VERSION is unchanged.
 * The Python binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 *   out_i = sum_r s_r(i) sum_j m_r(i,j) a(i,j) x_j W_r  +  x_i root  +  bias
 *
 * weight [R,Fi,Fo], root [Fi,Fo] (NULL: no root term), bias [Fo] (NULL: none): PyG's layouts, x W (not x W^T).
 * m_r(i,j): bit r of the entry's relation code; codes <= 0 are no edge, bits >= R are ignored.
 * s_r(i) = 1 / max(1, #{j: m_r(i,j)}) when `mean` (a count of the pattern, not of the values), else 1. */
#ifndef GCM_HIP_RGCN_H
#define GCM_HIP_RGCN_H

/* Dense forward.  x [B,N,Fi], adj [B,N,N] (adj[b,i,j]: i aggregates from j; the VALUES are used where a bit is set
 * and never read into the result elsewhere), rel [B,N,N] float32 holding the integer codes, out [B,N,Fo].
 * scale [B,R,N]: written when `mean` (keep it for the backward), may be NULL otherwise.
 * workspace: gcm_dense_rgcnconv_fwd_workspace_bytes.  B * R <= 65535, B * N <= 2^30. */
size_t gcm_dense_rgcnconv_fwd_workspace_bytes(int B, int N, int Fi, int Fo, int R);
int gcm_dense_rgcnconv_fwd(const float* x, const float* adj, const float* rel, const float* weight, const float* root,
                           const float* bias, float* out, float* scale, void* workspace, size_t workspace_bytes, int B,
                           int N, int Fi, int Fo, int R, int mean, gcm_stream_t stream);

/* Dense backward.  scale: what the forward wrote (NULL for the sum).  Outputs, each may be NULL to skip, all
 * overwritten: g_x [B,N,Fi], g_adj [B,N,N] (0 where no bit is set), g_weight [R,Fi,Fo], g_root [Fi,Fo], g_bias [Fo].
 * There is no gradient to rel. */
size_t gcm_dense_rgcnconv_bwd_workspace_bytes(int B, int N, int Fi, int Fo, int R);
int gcm_dense_rgcnconv_bwd(const float* g_out, const float* x, const float* adj, const float* rel, const float* weight,
                           const float* root, const float* scale, float* g_x, float* g_adj, float* g_weight,
                           float* g_root, float* g_bias, void* workspace, size_t workspace_bytes, int B, int N, int Fi,
                           int Fo, int R, gcm_stream_t stream);

/* Sparse forward over the destination CSR (row_ptr [M+1], col [E] = sources; col and edge_type may be NULL when
 * E == 0).  edge_type [E] int64 in CSR order: a relation id (an id outside [0, R) contributes nothing), or with
 * mask_mode the bit code.  Every entry counts (duplicates too) and has the value 1.  x [M,Fi], out [M,Fo],
 * scale [M,R] written when `mean`. */
size_t gcm_csr_rgcnconv_fwd_workspace_bytes(int64_t M, int64_t E, int Fi, int Fo, int R);
int gcm_csr_rgcnconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const int64_t* edge_type,
                         const float* weight, const float* root, const float* bias, float* out, float* scale,
                         void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int Fi, int Fo, int R, int mean,
                         int mask_mode, gcm_stream_t stream);

/* Sparse backward.  col_ptr [M+1] / rows [E] / perm [E]: the CSC by source (sink of each entry, and the CSR position
 * of each CSC entry: edge_type stays in CSR order); they may be NULL when E == 0 or neither g_x nor g_weight is
 * asked for.  Outputs as in the dense backward, without g_adj. */
size_t gcm_csr_rgcnconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int Fo, int R);
int gcm_csr_rgcnconv_bwd(const float* g_out, const float* x, const int64_t* edge_type, const int64_t* col_ptr,
                         const int64_t* rows, const int64_t* perm, const float* weight, const float* root,
                         const float* scale, float* g_x, float* g_weight, float* g_root, float* g_bias, void* workspace,
                         size_t workspace_bytes, int64_t M, int64_t E, int Fi, int Fo, int R, int mask_mode,
                         gcm_stream_t stream);

/* TypedEdge: one launch over L elements.  children: a HOST array of n_children device pointers, each a plane of L
 * floats; bits: a HOST array of n_children relation indices in [0, 16) (both are read during the call only).
 *   rel_out = rel | sum_k 2^bits[k] [children[k] > 0]   (an element no child selects keeps rel's value as it is)
 *   adj_out = diff_or(adj, children[0], ...): res + t - res t, left to right; NULL: not produced (adj is not read).
 * The outputs are fresh buffers: not in place. */
int gcm_typed_merge(const float* adj, const float* rel, const float* const* children, const int* bits, int n_children,
                    float* adj_out, float* rel_out, int64_t L, gcm_stream_t stream);

#endif /* GCM_HIP_RGCN_H */
