/* gcm_hip_knn.h - the k-nearest section of the distance selectors of the C ABI (csrc/knn.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Additive: GCM_ABI_VERSION is unchanged, no struct and no existing prototype changes.  The
 * Python binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * KNNEdge (gcm/edge_selectors/knn.py): the `mode` of gcm_edge_distance / _ex / _pre / _pre_ex and of a
 * gcm_selector_desc of kind GCM_SEL_DISTANCE carries k beside the metric:
 *   mode = metric | k << GCM_DIST_KNN_SHIFT      metric: GCM_DIST_L2_PERGRAPH or GCM_DIST_COSINE_SIM (the low byte)
 *                                                k:      1 .. GCM_DIST_KNN_MAX;  k = 0 is the threshold selector
 * With k bits set, the candidates of graph b are its image rows j < cur_b (as for the threshold modes: after the
 * overflow roll in the "pre" form) and their distance is
 *   L2_PERGRAPH   || cur[b, a0:a1] - nodes[b, j, b0:b1] ||      (the threshold mode's value, bit for bit)
 *   COSINE_SIM    1 - similarity                                (similarity: the threshold mode's value)
 * which is also what dist_out receives.  The candidates are ranked by (distance, j) ascending - equal distances go
 * to the lower index, a NaN distance ranks behind everything and is never selected - and the first min(k, cur_b) of
 * them are selected, of those only the ones with distance < max_distance when max_distance is finite (+inf: no cap).
 * The decisions are written like the threshold modes': adj[b, cur_b, j] = 1 (and adj[b, j, cur_b] = 1 when
 * bidirectional) for the selected j, or sel_row[b, j] = 1 / 0 for every j < cur_b in the "pre" form.
 * GCM_EINVAL: GCM_DIST_EUCLID_CROSSBATCH (or an unknown metric) with k bits, bits above the k field, cur_rows !=
 * NULL.  No workspace: gcm_edge_distance_workspace_bytes is 0 for these modes. */
#ifndef GCM_HIP_KNN_H
#define GCM_HIP_KNN_H

#define GCM_DIST_KNN_SHIFT 8
#define GCM_DIST_KNN_MAX 255

/* 1 when gcm_edge_distance* runs `mode` (k bits set) at these sizes, else 0: a valid metric and k, B, N, F > 0 and
 * N <= 8192 (one workgroup per graph keeps the ranking keys of its candidates in LDS). */
int gcm_edge_knn_supported(int mode, int B, int N, int F);

#endif /* GCM_HIP_KNN_H */
