/* gcm_hip_gen.h - the GEN section of the C ABI (csrc/genconv.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GIN section: device pointers only, int return (GCM_EINVAL on
 * null / invalid arguments, GCM_EUNSUPPORTED when C > 128), launches on `stream`, no allocation, no host
 * synchronisation and no float atomics: results are bitwise reproducible.  Additive: GCM_ABI_VERSION is unchanged.
 * The Python binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * The kernels are the softmax AGGREGATION of PyG's GENConv (DeeperGCN) and its gradients; lin_src / lin_dst, the
 * message norm and the mlp stay with the caller:
 *   m[j,c]   = relu(xs[j,c]) + eps
 *   agg[i,c] = sum over the set entries j of row i of a[i,j,c] m[j,c],  a[i,:,c] = softmax over those j of t m[j,c]
 * A row without entries aggregates 0.  t [1] is a DEVICE pointer read inside the kernels (never on the host: the
 * calls stay HIP-graph capturable); eps is the layer's constant.  The forward shifts every (row, channel) by its own
 * maximum in one pass (online softmax): logits of any size are exact.  It saves agg and lse [2, rows, C]: plane 0 the
 * maximum of t m over the row's entries, plane 1 the sum of exp(t m - maximum) (the log-sum-exp is plane 0 + log of
 * plane 1; 0 and 1 for a row without entries).  No per-edge weight is stored. */
#ifndef GCM_HIP_GEN_H
#define GCM_HIP_GEN_H

/* Dense forward, one launch, one wave per row.  xs [B,N,C], adj [B,N,N] (adj[b,i,j] != 0: i aggregates from j; only
 * the PATTERN is read, the diagonal is an ordinary entry), agg [B,N,C], lse [2,B,N,C].  bits [B*N, ceil(N/64)]
 * (written): bit j % 64 of word j / 64 of row i is set where adj[b,i,j] != 0 - the pattern as the backward reads it,
 * 1/32 of the adjacency.  C <= 128, any N. */
int gcm_dense_gen_fwd(const float* xs, const float* adj, const float* t, float eps, float* agg, float* lse,
                      int64_t* bits, int B, int N, int C, gcm_stream_t stream);

/* Dense backward; bits, agg, lse as the forward wrote them.  Outputs (each may be NULL to skip, both overwritten):
 *   g_xs [B,N,C]: g_m[j,c] = sum over the rows i with adj[b,i,j] != 0 of g_agg[i,c] a[i,j,c] (1 + t (m[j,c] -
 *                 agg[i,c])), g_xs = g_m where xs > 0, else 0  (a column sweep over the bit masks: no atomics);
 *   g_t [1] = sum over (i,c) of g_agg[i,c] (sum_j a[i,j,c] m[j,c]^2 - agg[i,c]^2)  (each row's moments in fp64, fp64
 *             partial sums of fixed row ranges into the workspace, then summed in a fixed order).
 * workspace: gcm_dense_gen_bwd_workspace_bytes (0 for an empty batch); needed only with g_t. */
size_t gcm_dense_gen_bwd_workspace_bytes(int B, int N, int C);
int gcm_dense_gen_bwd(const float* g_agg, const float* xs, const int64_t* bits, const float* t, float eps,
                      const float* agg, const float* lse, float* g_xs, float* g_t, void* workspace,
                      size_t workspace_bytes, int B, int N, int C, gcm_stream_t stream);

/* Sparse forward over the destination CSR (row_ptr [M+1], col [E] = sources; col may be NULL when E == 0).  The
 * entries are used as given: no loop is added or removed, duplicates count once each.  xs, agg [M,C], lse [2,M,C]. */
int gcm_csr_gen_fwd(const float* xs, const int64_t* row_ptr, const int64_t* col, const float* t, float eps, float* agg,
                    float* lse, int64_t M, int64_t E, int C, gcm_stream_t stream);

/* Sparse backward.  col_ptr [M+1] / rows [E]: the CSC by source (sink of each entry), needed for g_xs; row_ptr / col:
 * the CSR again, needed for g_t; each pair may be NULL when E == 0 or its output is skipped.  g_xs [M,C] and g_t [1]
 * as in the dense backward; either may be NULL to skip. */
size_t gcm_csr_gen_bwd_workspace_bytes(int64_t M, int64_t E, int C);
int gcm_csr_gen_bwd(const float* g_agg, const float* xs, const float* t, float eps, const float* agg, const float* lse,
                    const int64_t* row_ptr, const int64_t* col, const int64_t* col_ptr, const int64_t* rows,
                    float* g_xs, float* g_t, void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int C,
                    gcm_stream_t stream);

#endif /* GCM_HIP_GEN_H */
