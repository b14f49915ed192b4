/* gcm_hip_window.h - the sliding-window section of the C ABI (csrc/sparse_window.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the entries around it: device pointers only, int return (GCM_EINVAL
 * on null / invalid arguments, GCM_EUNSUPPORTED for sizes without a kernel), launches on `stream`, no allocation, no
 * host synchronisation, no float atomics, and no atomic decides where an entry lands: results are bitwise
 * reproducible.  Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as
 * gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * "Drop the oldest k_b nodes of every graph" of a SparseGCM hidden state (nodes [B,N,F], COO indices idx [3,E] =
 * (batch, sink, source) sorted by (batch, sink, source), values [E], T [B]): SparseGCM.drop_oldest / reset_hidden /
 * overflow="wrap".  With t_b = min(max(T_b, 0), N) and kc_b = min(max(k_b, 0), t_b), both taken on the device (every
 * access stays in bounds for any contents of k and T):
 *   nodes'[b, i] = nodes[b, i + kc_b] for i < t_b - kc_b, zero otherwise;
 *   an entry (b, sink, source) survives iff source >= kc_b and becomes (b, sink - kc_b, source - kc_b) with its value;
 *   survivors keep their order, so the list stays sorted and duplicate free;  T' = T - kc.
 * Three steps, because the host sizes the exact output from E' between the first and the last: */
#ifndef GCM_HIP_WINDOW_H
#define GCM_HIP_WINDOW_H

/* entries per chunk of the list (one workgroup's share); chunk_off has E / CHUNK rounded up, plus one, elements */
#define GCM_SPARSE_DROP_CHUNK 1024

/* Survivors per chunk, then their exclusive scan (one workgroup): chunk_off[c] = survivors ahead of chunk c,
 * chunk_off[n_chunks] = E' (what the host reads back).  T_out [B] = T - kc.  E == 0: idx may be NULL, chunk_off[0] = 0.
 * Two launches (one for E == 0). */
int gcm_sparse_drop_plan(const int64_t* idx, const int64_t* k, const int64_t* T, int64_t* T_out, int64_t* chunk_off,
                         int64_t E, int B, int N, gcm_stream_t stream);

/* backward == 0: out[b, i] = in[b, i + kc_b] for i < t_b - kc_b, else 0.  backward != 0, the adjoint on gradients:
 * out[b, j] = in[b, j - kc_b] for kc_b <= j < t_b, else 0.  in != out.  16-byte accesses when F % 4 == 0 and both
 * pointers are 16-byte aligned.  B <= 65535.  One launch. */
int gcm_sparse_drop_nodes(const float* in, const int64_t* k, const int64_t* T, float* out, int B, int N, int F,
                          int backward, gcm_stream_t stream);

/* The compaction, from the plan of the same (idx, k, T): out_idx [3,E_new], out_vals [E_new] (vals and out_vals both
 * NULL: indices only), src_pos [E_new] = position of every survivor in the old list, bptr [B+1] = per-graph pointer
 * of the new list (what gcm_ptr_from_sorted over its batch row gives; written from the first entry of every graph of
 * the old list, which must be sorted by batch).  E_new = chunk_off[n_chunks]; a survivor beyond E_new is not
 * written.  One launch (E == 0: a memset of bptr). */
int gcm_sparse_drop_edges(const int64_t* idx, const float* vals, const int64_t* k, const int64_t* T,
                          const int64_t* chunk_off, int64_t* out_idx, float* out_vals, int64_t* src_pos,
                          int64_t* bptr, int64_t E, int64_t E_new, int B, int N, gcm_stream_t stream);

/* Gradient of the values: g_in [E] = 0, then g_in[src_pos[i]] = g_out[i] (src_pos is injective: plain stores). */
int gcm_sparse_drop_values_bwd(const float* g_out, const int64_t* src_pos, float* g_in, int64_t E, int64_t E_new,
                               gcm_stream_t stream);

#endif /* GCM_HIP_WINDOW_H */
