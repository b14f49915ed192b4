/* gcm_hip_edgeconv.h - the EdgeConv section of the C ABI (csrc/edgeconv.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GEN section: device pointers only, int return (GCM_EINVAL on
 * null / invalid arguments, GCM_EUNSUPPORTED when H or C > 128, GCM_EWORKSPACE), launches on `stream`, no allocation,
 * no host synchronisation and no float atomics: results are bitwise reproducible.  Additive: GCM_ABI_VERSION is
 * unchanged.  The Python binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * The kernels are the per-edge stage of PyG's EdgeConv (Dynamic Graph CNN), x_i' = max_j nn([x_i, x_j - x_i]), for
 * nn = Linear(2F -> H), leaky_relu(slope), Linear(H -> C).  With the first weight W1 = [A | Bm] the caller forms the
 * two per-node products P = x (A - Bm)^T + b1 and Q = x Bm^T; then
 *   h[i,j]   = leaky_relu(P[i] + Q[j], slope)                   (slope = 0: ReLU)
 *   m[i,j]   = W2 h[i,j] + b2
 *   out[i,c] = max over the set entries j of row i of m[i,j,c]   (0 for a row without entries)
 * and winner[i,c] names the entry that attains it (-1 for none).  Of bitwise equal messages the first entry in row
 * order wins.  Neither h nor m is written to memory; the winner table is what the backward needs.  w2 [C,H] row major
 * (torch.nn.Linear.weight), b2 [C] or NULL.  H, C <= 128. */
#ifndef GCM_HIP_EDGECONV_H
#define GCM_HIP_EDGECONV_H

/* Dense forward, one launch.  P, Q [B,N,H], adj [B,N,N] (adj[b,i,j] != 0: i receives from j; only the PATTERN is read,
 * the diagonal is an ordinary entry), out [B,N,C], winner [B,N,C] int32: the source index j within the graph (ties:
 * the lowest j).  Cost follows the number of set entries (rounded up to 8 per wave of 2 rows) plus one read of adj. */
int gcm_dense_edgemax_fwd(const float* P, const float* Q, const float* adj, const float* w2, const float* b2,
                          float slope, float* out, int32_t* winner, int B, int N, int H, int C, gcm_stream_t stream);

/* Dense backward; winner as the forward wrote it.  With pre = P[i] + Q[j] of the winner j of (i, c) and
 * d = g_out[i,c] w2[c,:] leaky_relu'(pre):  g_P[i] = sum over c of d,  g_Q[j] = sum over the (i, c) that j won of d,
 * g_w2[c,:] = sum over i of g_out[i,c] leaky_relu(pre),  g_b2[c] = sum over the i with a winner of g_out[i,c].
 * Outputs g_P, g_Q [B,N,H], g_w2 [C,H], g_b2 [C]: each may be NULL to skip (its work is not done), all overwritten.
 * workspace: gcm_dense_edgemax_bwd_workspace_bytes; needed only with g_w2 or g_b2. */
size_t gcm_dense_edgemax_bwd_workspace_bytes(int B, int N, int H, int C);
int gcm_dense_edgemax_bwd(const float* g_out, const float* P, const float* Q, const int32_t* winner, const float* w2,
                          float slope, float* g_P, float* g_Q, float* g_w2, float* g_b2, void* workspace,
                          size_t workspace_bytes, int B, int N, int H, int C, gcm_stream_t stream);

/* Sparse forward over the destination CSR (row_ptr [M+1], col [E] = sources; col may be NULL when E == 0).  The
 * entries are used as given: no loop is added or removed (an i -> i entry has x_j - x_i = 0), duplicates compete
 * separately.  P, Q [M,H], out [M,C], winner [M,C] int32: the CSR position of the winning entry (ties: the first
 * entry in CSR order).  E < 2^31. */
int gcm_csr_edgemax_fwd(const float* P, const float* Q, const int64_t* row_ptr, const int64_t* col, const float* w2,
                        const float* b2, float slope, float* out, int32_t* winner, int64_t M, int64_t E, int H, int C,
                        gcm_stream_t stream);

/* Sparse backward.  col [E]: the CSR's sources again; col_ptr [M+1] / rows [E] / perm [E]: the CSC by source (sink and
 * CSR position of each entry), needed for g_Q only; each may be NULL when E == 0 or its output is skipped.  Outputs
 * as the dense backward's with rows M. */
size_t gcm_csr_edgemax_bwd_workspace_bytes(int64_t M, int64_t E, int H, int C);
int gcm_csr_edgemax_bwd(const float* g_out, const float* P, const float* Q, const int32_t* winner, const int64_t* col,
                        const int64_t* col_ptr, const int64_t* rows, const int64_t* perm, const float* w2, float slope,
                        float* g_P, float* g_Q, float* g_w2, float* g_b2, void* workspace, size_t workspace_bytes,
                        int64_t M, int64_t E, int H, int C, gcm_stream_t stream);

#endif /* GCM_HIP_EDGECONV_H */
