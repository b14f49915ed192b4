/* gcm_hip_gin.h - the GIN section of the C ABI (csrc/ginconv.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GCN section there: device pointers only, int return (GCM_EINVAL on
 * null / invalid arguments, GCM_EUNSUPPORTED when F > 128), launches on `stream`, no allocation, no host
 * synchronisation and no float atomics: results are bitwise reproducible.  Additive: GCM_ABI_VERSION is unchanged.
 * The Python binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * The kernels are the AGGREGATION of PyG's GINConv / DenseGINConv and its three gradients; the layer's `nn` is an
 * arbitrary module and stays with the caller:
 *   dense : h[b,i,:] = s x[b,i,:] + sum_j adj[b,i,j] x[b,j,:],  s = add_loop ? 1 + eps : 0
 *   sparse: h[i,:]   = (1 + eps) x[i,:] + sum over the CSR row i of x[col[e],:]
 * eps [1] is a DEVICE pointer read inside the kernels (never on the host: the calls stay HIP-graph capturable). */
#ifndef GCM_HIP_GIN_H
#define GCM_HIP_GIN_H

/* Dense forward, one launch.  x [B,N,F], adj [B,N,N] (adj[b,i,j]: i aggregates from j; the VALUES are used and the
 * diagonal is an ordinary entry), h [B,N,F].  F <= 128, B <= 65535, any N. */
int gcm_dense_gin_fwd(const float* x, const float* adj, const float* eps, float* h, int B, int N, int F, int add_loop,
                      gcm_stream_t stream);

/* Dense backward.  Outputs (each may be NULL to skip, all overwritten):
 *   g_x [B,N,F] = adj^T g_h + s g_h;  g_adj [B,N,N]: g_adj[b,i,j] = <g_h[b,i,:], x[b,j,:]>;
 *   g_eps [1] = add_loop ? sum <g_h, x> : 0  (per-row dot products into the workspace, then summed in a fixed order).
 * workspace: gcm_dense_gin_bwd_workspace_bytes (0 for an empty batch). */
size_t gcm_dense_gin_bwd_workspace_bytes(int B, int N, int F);
int gcm_dense_gin_bwd(const float* g_h, const float* x, const float* adj, const float* eps, float* g_x, float* g_adj,
                      float* g_eps, void* workspace, size_t workspace_bytes, int B, int N, int F, int add_loop,
                      gcm_stream_t stream);

/* Sparse forward over the destination CSR (row_ptr [M+1], col [E] = sources; col may be NULL when E == 0).  The
 * entries are used as given: no loop is added or removed, duplicates count once each.  x, h [M,F].  F <= 128. */
int gcm_csr_gin_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* eps, float* h, int64_t M,
                    int64_t E, int F, gcm_stream_t stream);

/* Sparse backward.  col_ptr [M+1] / rows [E]: the CSC by source (sink of each entry), may be NULL when E == 0.
 *   g_x [M,F] = (1 + eps) g_h + sum over the CSC column j of g_h[rows[k],:];  g_eps [1] = sum <g_h, x>.
 * Either output may be NULL to skip; x may be NULL without g_eps. */
size_t gcm_csr_gin_bwd_workspace_bytes(int64_t M, int64_t E, int F);
int gcm_csr_gin_bwd(const float* g_h, const float* x, const float* eps, const int64_t* col_ptr, const int64_t* rows,
                    float* g_x, float* g_eps, void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int F,
                    gcm_stream_t stream);

#endif /* GCM_HIP_GIN_H */
