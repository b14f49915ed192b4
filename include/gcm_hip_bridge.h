/* gcm_hip_bridge.h - the dense <-> sparse bridge section of the C ABI (csrc/dense_sparse.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the message-passing section: device pointers only, int return
 * (GCM_EINVAL on null / invalid arguments, before anything is launched), launches on `stream`, no allocation, no host
 * synchronisation and no float atomics: every sum runs in one fixed order and results are bitwise reproducible.
 * Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as gcm_hip.h
 * (gcm/_abi.py, gcm/_hip.py).
 *
 * gcm.gcm.DenseToSparse turns adj [B,N,N] into the flat edge list of its entries > 0 in (b, r, c) order - the order of
 * torch.nonzero - together with the index the sparse layers share (GraphIndex: CSR by sink, CSC by source), without a
 * sort: the row-major order of the entries is the list order, their column-major order is the other view, and one
 * walk over a bit image of adj > 0 numbers every entry in both.  Three launches and one host read of E between the
 * second and the third (the caller allocates the [E] arrays):
 *
 *     gcm_bridge_image   adj -> image, row_cnt, col_cnt, total
 *     gcm_bridge_scan    total -> graph_off            (the caller reads graph_off[B] = E)
 *     gcm_bridge_fill    image, counts, graph_off -> edge_index, both pointer arrays, both permutations, values
 *
 * gcm.gcm.SparseToDense is the way back (PyG's to_dense_batch / to_dense_adj with max_num_nodes = N).
 * Node m = b*N + n throughout the first group; in the second group the graphs are the runs of a non-decreasing
 * batch_idx and node_ptr [B+1] holds the first node of each (gcm_ptr_from_sorted over batch_idx). */
#ifndef GCM_HIP_BRIDGE_H
#define GCM_HIP_BRIDGE_H

/* the largest N of the bridge kernels: one thread per column of a graph, one workgroup per graph */
#define GCM_BRIDGE_MAX_N 512

/* image[(b*N + r) * W + k], W = (N + 63) / 64: bit j of the word is adj[b, r, 64k + j] > 0 (strict: negative entries
 * and NaN are no edges; bits of columns >= N are 0).  row_cnt [B*N], col_cnt [B*N]: the entries of each row / column of
 * each graph; total [B]: the entries of each graph.  adj is float32, or int64 when adj_i64 != 0.
 * 1 <= N <= GCM_BRIDGE_MAX_N, else GCM_EUNSUPPORTED. */
int gcm_bridge_image(const void* adj, int adj_i64, uint64_t* image, int32_t* row_cnt, int32_t* col_cnt,
                     int32_t* total, int B, int N, gcm_stream_t stream);

/* graph_off [B+1]: the exclusive prefix of total, graph_off[B] = E.  One workgroup, any B. */
int gcm_bridge_scan(const int32_t* total, int64_t* graph_off, int B, gcm_stream_t stream);

/* Entry (b, r, c) is number p of the row-major order (b, r, c) and number q of the column-major order (b, c, r).
 *   edge_index [2,E]  at p: (b*N + r, b*N + c), or (b*N + c, b*N + r) with transpose != 0
 *   row_ptr [B*N+1]   exclusive prefix of row_cnt (first p of each row),  row_ptr[B*N] = E
 *   col_ptr [B*N+1]   exclusive prefix of col_cnt (first q of each column), col_ptr[B*N] = E
 *   by_col [E]        by_col[q] = p          col_pos [E]  col_pos[p] = q  (NULL: not written)
 *   col_rows [E]      col_rows[q] = b*N + r
 *   values [E] | NULL values[p] = (float)adj[b, r, c]
 * E must be graph_off[B] as gcm_bridge_scan wrote it from the counts of the same image; every store is checked against
 * E all the same.  E == 0 writes the two pointer arrays only. */
int gcm_bridge_fill(const void* adj, int adj_i64, const uint64_t* image, const int32_t* row_cnt,
                    const int32_t* col_cnt, const int64_t* graph_off, int64_t* edge_index, int64_t* row_ptr,
                    int64_t* col_ptr, int64_t* by_col, int64_t* col_pos, int64_t* col_rows, float* values, int B,
                    int N, int64_t E, int transpose, gcm_stream_t stream);

/* The gradient of `values`: g_adj [B,N,N] = 0, then g_adj[b, r, c] = g_values[p] for every entry of edge_index as
 * gcm_bridge_fill wrote it (every entry has its own element: plain stores).  Entries outside [0, B*N) or whose two
 * ends lie in different graphs are skipped. */
int gcm_bridge_values_bwd(const float* g_values, const int64_t* edge_index, float* g_adj, int B, int N, int64_t E,
                          int transpose, gcm_stream_t stream);

/* x [B,N,F]: x[b, n, :] = x_sp[node_ptr[b] + n, :] for n < min(N, nodes of graph b), else 0.  x_sp [M,F]. */
int gcm_bridge_dense_nodes(const float* x_sp, const int64_t* node_ptr, float* x, int64_t M, int B, int N, int F,
                           gcm_stream_t stream);

/* g_x_sp [M,F]: g_x_sp[m, :] = g_x[batch_idx[m], m - node_ptr[batch_idx[m]], :] when that position is < N, else 0. */
int gcm_bridge_dense_nodes_bwd(const float* g_x, const int64_t* batch_idx, const int64_t* node_ptr, float* g_x_sp,
                               int64_t M, int B, int N, int F, gcm_stream_t stream);

/* adj [B,N,N] = 0, then for every edge e = (s, d) with batch_idx[s] == batch_idx[d] = b and both positions in the
 * graph < N:  adj[b, s - node_ptr[b], d - node_ptr[b]] += edge_weight ? edge_weight[e] : 1.  (row_ptr [M+1],
 * csr_perm [E] | NULL) is the list by sink (GraphIndex): one thread per sink walks its entries in order, so the sum
 * of duplicates has one order and no atomics are used.  edge_index [2,E] (source, sink). */
int gcm_bridge_dense_adj(const int64_t* row_ptr, const int64_t* csr_perm, const int64_t* edge_index,
                         const float* edge_weight, const int64_t* batch_idx, const int64_t* node_ptr, float* adj,
                         int64_t M, int64_t E, int B, int N, gcm_stream_t stream);

/* g_weight [E]: g_weight[e] = g_adj[b, s_local, d_local] of the element edge e was added to, 0 for a dropped edge. */
int gcm_bridge_dense_adj_bwd(const float* g_adj, const int64_t* edge_index, const int64_t* batch_idx,
                             const int64_t* node_ptr, float* g_weight, int64_t M, int64_t E, int B, int N,
                             gcm_stream_t stream);

#endif /* GCM_HIP_BRIDGE_H */
