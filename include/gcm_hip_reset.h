/* gcm_hip_reset.h - the episode-reset section of the C ABI (csrc/rollout_reset.hip, csrc/state.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs, status codes and
 * gcm_selector_desc: include gcm_hip.h, not this file.  Same conventions as the entries around it: device pointers
 * only, int return (GCM_EINVAL on null / invalid arguments, GCM_EUNSUPPORTED for shapes without a kernel), launches on
 * `stream`, no allocation, no host synchronisation, no float atomics: results are bitwise reproducible.
 * Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as gcm_hip.h
 * (gcm/_abi.py, gcm/_hip.py). */
#ifndef GCM_HIP_RESET_H
#define GCM_HIP_RESET_H

/* The masked clear of whole graphs - what a caller does at an episode's end (`nodes[done] = 0; adj[done] = 0;
 * num_nodes[done] = 0`) as ONE launch: for every graph b, out[b] = mask[b] ? 0 : in[b] for nodes [B,N,F], adj [B,N,N],
 * weights [B,N,N] (both NULL: no edge weights) and count [B] (both NULL: skipped).  mask [B]: one byte per graph
 * (a torch.bool tensor).  in == out is allowed for any of the pairs, and then only the masked graphs are written.
 * Applied to gradient tensors (count NULL) it is its own backward: the gradient w.r.t. a cleared graph's incoming
 * state is zero, the others' is the identity.  B <= 65535. */
int gcm_state_reset(const float* nodes_in, float* nodes_out, const float* adj_in, float* adj_out,
                    const float* weights_in, float* weights_out, const int64_t* count_in, int64_t* count_out,
                    const uint8_t* mask, int B, int N, int F, gcm_stream_t stream);

/* start [T,B] int32 from reset [T,B] (one byte per entry, a torch.bool tensor): start[t,b] = the latest s <= t with
 * reset[s,b] != 0, else 0 - the step at which the episode that step t of graph b belongs to began (reset[t,b] empties
 * graph b BEFORE step t inserts its observation).  One thread per graph walking t.  T <= 65535. */
int gcm_episode_start(const uint8_t* reset, int32_t* start, int T, int B, gcm_stream_t stream);

/* gcm_dense_rollout_tp_fwd with per-graph episode resets: the same two launches, caches, records and preconditions
 * (gcm_dense_rollout_tp_supported, whose rule "T > N needs N > 2 max(hop)" stays as it is: episode lengths are not
 * known on the host), with start [T,B] as written by gcm_episode_start.  With age[t,b] = t - start[t,b], hop h of
 * step t is valid in graph b iff h <= min(age, N-1); the record of (t, b) carries that graph's live list and header
 * (hdr = {valid hops + 1, valid hops, min(age, N-1), age >= N}), read by gcm_dense_rows_bptt_cached(..., N := Tc)
 * unchanged.  Final state per graph, t0_b = max(start[T-1,b], T-N): rows t - t0_b (t >= t0_b) of nodes / adj hold
 * obs[t] / the band row, count[b] = T - t0_b; nodes [B,N,F] and adj [B,N,N] must be ZERO on entry (rows at or beyond
 * count[b] stay zero).  ORs GCM_FLAG_WRAPPED into *flags when some graph receives a node at age >= N (the overflow
 * roll of gcm.py:263-271), GCM_FLAG_NONFINITE as gcm_dense_rollout_tp_fwd.  Every access stays in bounds for any
 * contents of start. */
int gcm_dense_rollout_tp_reset_fwd(const float* obs, const int32_t* start, const gcm_selector_desc* selectors,
                                   int n_selectors, const float* params, int has_bias, int act1, int act2,
                                   float* nodes, float* adj, int64_t* count, float* cache_h1, float* cache_agg1,
                                   float* cache_nodes, float* records, size_t rec_stride, int record, float* mx_all,
                                   uint32_t* flags, int T, int B, int N, int Tc, int F, int H1, int H2,
                                   gcm_stream_t stream);

#endif /* GCM_HIP_RESET_H */
