// Where the distance selector kernels find the graph, and how they hand over a decision: shared by
// distance.hip (threshold selectors) and knn.hip (k-nearest selection).
#pragma once
#include "gcm_common.h"

// Where a kernel finds the graph.  Either the ADVANCED state (count == nullptr): cur_idx[b] is the row
// that holds the current node.  Or the state BEFORE the step (count = num_nodes going in, obs = the
// new nodes): the current node is obs[b], it will land in row cur = min(count, N-1), and after the
// overflow roll (count + 1 > N) image row j is stored row j + 1.  Same arithmetic either way: the
// second form lets the live-row step (rows_step.hip) run the distance selectors ahead of its own
// state advance, with the decisions handed over as a row [B, N] instead of adjacency writes.
//
// cur_rows != nullptr: the "current nodes" the distances are taken against come from outside - n_cur rows
// [n_cur, F], the all-gathered current nodes of EVERY rank of a batch-sharded run (EuclideanEdge's
// mean runs over all graphs b' of the GLOBAL batch, distance.py:48-49) - instead of the B local ones.
struct View {
  const float* nodes;
  const int64_t* cur_idx;
  const int64_t* count;
  const float* obs;
  const float* cur_rows;
  int n_cur;
};
__device__ __forceinline__ int view_cur(const View& v, int b, int N, int& sh) {
  sh = 0;
  int64_t c;
  if (v.count) {
    const int64_t n = v.count[b];
    sh = n + 1 > N ? 1 : 0;
    c = sh ? n - 1 : n;
  } else {
    c = v.cur_idx[b];
  }
  return (int)(c < 0 ? 0 : (c > N - 1 ? N - 1 : c));
}
__device__ __forceinline__ const float* view_cur_row(const View& v, int b, int cur, int N, int F) {
  return v.count ? v.obs + (size_t)b * F : v.nodes + ((size_t)b * N + cur) * F;
}
// decision for image row j: adjacency entry (advanced state) or the row handed to the step kernel
__device__ __forceinline__ void view_emit(float* adj, float* sel_row, int b, int cur, int j, int N,
                                          bool hit, int bidirectional) {
  if (sel_row) {
    sel_row[(size_t)b * N + j] = hit ? 1.f : 0.f;
  } else if (hit) {
    adj[((size_t)b * N + cur) * N + j] = 1.f;
    if (bidirectional) adj[((size_t)b * N + j) * N + cur] = 1.f;
  }
}

// knn.hip: the modes with k bits (include/gcm_hip_knn.h), called by run_distance() of distance.hip with its own
// arguments.  GCM_EINVAL for a metric other than L2_PERGRAPH / COSINE_SIM, gathered current rows or a bad slice;
// GCM_EUNSUPPORTED beyond gcm_edge_knn_supported.
int gcm_knn_run(const View& vw, float* adj, float* sel_row, int mode, float max_distance, const float* dist_param,
                int a0, int a1, int b0, int b1, int bidirectional, float* dist_out, int B, int N, int F,
                hipStream_t stream);
