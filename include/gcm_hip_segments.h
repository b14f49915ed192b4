/* gcm_hip_segments.h - the episode-segment section of the C ABI (csrc/sparse_segments.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the entries around it: device pointers only, int return (GCM_EINVAL
 * on null / invalid arguments, GCM_EUNSUPPORTED for sizes without a kernel), launches on `stream`, no allocation, no
 * host synchronisation, no float atomics, and no atomic decides where an entry lands: results are bitwise
 * reproducible.  Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as
 * gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * SparseGCM.rollout(x, reset=mask): mask u8 [B,t], mask[b,s] != 0 empties graph b before x[b,s] is inserted.  With
 * tau_b = min(max(taus_b, 0), t), the VALID resets of graph b are the columns s < tau_b with mask[b,s] != 0,
 * r_1 < ... < r_m.  Graph b becomes m + 1 virtual graphs (segments) v = vbase[b] + j, j = 0..m:
 *   j = 0: columns [0, r_1) (m = 0: [0, tau_b)), entering with the stored state - unless r_1 == 0: then it is empty,
 *          takes no column, and the stored rows and edges of graph b are dropped;
 *   j > 0: columns [r_j, r_{j+1}) (the last one to tau_b), entering empty.
 * vbase [B+1] is the exclusive scan of m_b + 1, so v is monotone in b and a list sorted by batch stays sorted under
 * b -> vbase[b].  The ordinary call then runs over the B' = vbase[B] virtual graphs, and the last virtual graph of
 * every b (v = vbase[b+1] - 1) is the state the call returns.  Every index read from the mask, taus, the table or an
 * edge list is clamped on the device: any contents stay in bounds.  DESIGN 3.28. */
#ifndef GCM_HIP_SEGMENTS_H
#define GCM_HIP_SEGMENTS_H

/* entries per chunk of an edge list (one workgroup's share); chunk_off has E / CHUNK rounded up, plus one, elements */
#define GCM_SPARSE_SEG_CHUNK 1024
/* rows of the segment table (each `cap` = B * (t + 1) long, the worst case; the first B' entries are written):
 * owner b, first column, length, enters_empty (0 only for a j = 0 segment that keeps the stored state), T the segment
 * enters with (T_b or 0), and its batch in the returned state (owner for the last segment of b, else -1) */
#define GCM_SPARSE_SEG_OWNER 0
#define GCM_SPARSE_SEG_START 1
#define GCM_SPARSE_SEG_LEN 2
#define GCM_SPARSE_SEG_EMPTY 3
#define GCM_SPARSE_SEG_T 4
#define GCM_SPARSE_SEG_FINAL 5
#define GCM_SPARSE_SEG_ROWS 6
/* totals [4], what the host reads back: B', t' (longest segment, at least 1), valid resets, surviving stored edges */
#define GCM_SPARSE_SEG_TOTALS 4

/* The plan.  vbase [B+1]; table [GCM_SPARSE_SEG_ROWS, cap], cap >= B * (t + 1); relabel [B] = vbase[b], or -1 when
 * the stored state of b is dropped (what gcm_sparse_seg_edges takes for the stored list); idx [3,E] the stored list
 * (NULL with E == 0); chunk_off [n_chunks + 1] = survivors of the stored list ahead of every chunk, the last their
 * count; totals [GCM_SPARSE_SEG_TOTALS].  cap must fit an int.  Four launches (three for E == 0): a ballot over 64
 * columns of a mask row at a time counts and places the resets of a graph (one wave per graph), a wave-shuffle scan
 * over the graphs gives vbase. */
int gcm_sparse_seg_plan(const uint8_t* mask, const int64_t* taus, const int64_t* T, const int64_t* idx,
                        int64_t* vbase, int64_t* table, int64_t cap, int64_t* relabel, int64_t* chunk_off,
                        int64_t* totals, int64_t E, int B, int t, gcm_stream_t stream);

/* Rows between the batch layout [B,t,F] and the segment layout [Bp,tp,F].
 * backward == 0 (gather): out [Bp,tp,F], out[v,i] = in[owner_v, start_v + i] for i < len_v, else 0.
 * backward != 0 (the adjoint, and the collection of the call's outputs): out [B,t,F] = 0, then
 * out[owner_v, start_v + i] = in[v,i] for i < len_v (segments do not overlap: plain stores).
 * 16-byte accesses when F % 4 == 0 and both pointers are 16-byte aligned.  One launch (backward: a memset first). */
int gcm_sparse_seg_rows(const float* in, const int64_t* table, int64_t cap, float* out, int Bp, int tp, int B, int t,
                        int F, int backward, gcm_stream_t stream);

/* Node matrices between [B,N,F] and [Bp,N,F].  final == 0 pairs b with v = vbase[b] unless that segment enters empty
 * (the expansion of the stored state); final != 0 pairs b with v = vbase[b+1] - 1 (the state the call returns).
 * to_segments != 0: out [Bp,N,F], out[v] = in[b] for a paired v, 0 otherwise.
 * to_segments == 0: out [B,N,F],  out[b] = in[v] for a paired b, 0 otherwise.
 * Each is the adjoint of the other.  in != out.  One launch. */
int gcm_sparse_seg_nodes(const float* in, const int64_t* vbase, const int64_t* table, int64_t cap, float* out, int Bp,
                         int B, int N, int F, int final, int to_segments, gcm_stream_t stream);

/* Survivors of a list under a relabelling of its batches: relabel [B_old] >= 0 the new batch (non-decreasing over the
 * kept batches), < 0 the entries of that batch go.  chunk_off [n_chunks + 1] as above.  Two launches (one for
 * E == 0). */
int gcm_sparse_seg_edges_plan(const int64_t* idx, const int64_t* relabel, int64_t* chunk_off, int64_t E, int B_old,
                              gcm_stream_t stream);

/* The order-preserving compaction, from chunk_off of the same (idx, relabel): out_idx [3,E_new] = (relabel[batch],
 * sink, source), out_vals [E_new] (vals and out_vals both NULL: indices only), src_pos [E_new] = the position of every
 * survivor in the old list (gcm_sparse_drop_values_bwd is the values' adjoint).  A survivor beyond E_new is not
 * written, a new batch is clamped into [0, B_new).  One launch (none for E == 0). */
int gcm_sparse_seg_edges(const int64_t* idx, const float* vals, const int64_t* relabel, const int64_t* chunk_off,
                         int64_t* out_idx, float* out_vals, int64_t* src_pos, int64_t E, int64_t E_new, int B_old,
                         int B_new, gcm_stream_t stream);

/* T_out [B] = T_seg[vbase[b+1] - 1]: the node counts of the returned state.  One launch. */
int gcm_sparse_seg_final_T(const int64_t* T_seg, const int64_t* vbase, int64_t* T_out, int Bp, int B,
                           gcm_stream_t stream);

#endif /* GCM_HIP_SEGMENTS_H */
