/* gcm_hip_learned_det.h - the deterministic LearnedEdge section of the C ABI (csrc/learned_sparsemax.hip, in
 * libgcm_hip.so).  Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status
 * codes: include gcm_hip.h, not this file.  Same conventions as gcm_learned_select_fwd / _bwd there: device pointers
 * only, int return (GCM_EINVAL on null / invalid arguments, GCM_EUNSUPPORTED when N > 1024), launches on `stream`, no
 * allocation, no host synchronisation, no float atomics and no random numbers: results are bitwise reproducible.
 * Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as gcm_hip.h
 * (gcm/_abi.py, gcm/_hip.py). */
#ifndef GCM_HIP_LEARNED_DET_H
#define GCM_HIP_LEARNED_DET_H

/* learned.py:78-111 with the `deterministic` branch taken: edges = Spardmax(logits) (util.py:29-42), the published
 * sparsemax (Martins & Astudillo 2016) made binary with a straight-through estimator, cutoff 0.  The reference's own
 * import of the `sparsemax` package is commented out, so parity is pinned to the published algorithm only.
 * Per graph b, cur = cur_idx[b] clamped to [0, N-1], n = cur candidates j < n with logits z_j:
 *   p = sparsemax(z[:n]): tau with sum_j max(z_j - tau, 0) = 1, support S = {j : z_j > tau}
 *   adj[b, cur, j] = (1[j in S] + adj[b, cur, j] > 0) for j < n, IN PLACE; nothing else of adj is touched
 *   soft [B,N] = p, 0 for j >= n: kept for the backward, which reads the support from it (soft > 0)
 * n = 0: no entry of adj is written and soft[b] = 0.  Equal logits are all in S or all out, whichever column holds
 * them.  logits [B,N] (entries j >= n are not read), adj [B,N,N].  No sample count and no cutoff take part. */
int gcm_learned_sparsemax_fwd(const float* logits, const int64_t* cur_idx, float* adj, float* soft, int B, int N,
                              gcm_stream_t stream);
/* Both straight-through estimators are identities, so d p_j = g_adj[b, cur, j] and g_logits [B,N] (overwritten) is the
 * sparsemax Jacobian applied to it: g_j - (sum_{k in S} g_k) / |S| for j in S, 0 elsewhere (all j >= n; n = 0: the
 * whole row).  The gradient of the incoming adjacency is g_adj itself and is not computed here. */
int gcm_learned_sparsemax_bwd(const float* g_adj, const float* soft, const int64_t* cur_idx, float* g_logits, int B,
                              int N, gcm_stream_t stream);

#endif /* GCM_HIP_LEARNED_DET_H */
