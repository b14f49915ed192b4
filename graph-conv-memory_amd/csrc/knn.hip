// k-nearest selection for the Distance edge selectors (KNNEdge, include/gcm_hip_knn.h): the distance modes whose
// `mode` carries k bits.  Candidates of graph b: its image rows j < cur_b.
//
//   L2_PERGRAPH   d[b,j] = || cur[b, a0:a1] - nodes[b, j, b0:b1] ||      (k_pergraph's value, distance.hip)
//   COSINE_SIM    d[b,j] = 1 - <cur[b]/max(|cur[b]|,eps), nodes[b,j]/max(|nodes[b,j]|,eps)>
//
// then adj[b, cur_b, j] = 1 for the first min(k, cur_b) candidates in (d, j) order that also have d < max_distance.
//
// One workgroup of four wavefronts per graph.  Thread t computes the distances of candidates t, t + 256, ... (the
// same fmaf chain in column order as k_pergraph, then sqrtf) and leaves each as an ORDER-PRESERVING 32-bit key in LDS
// (key(a) < key(b) <=> a < b; NaN -> the largest key).  Behind one barrier every candidate's RANK is the number of
// candidates that precede it in (d, j) order: with the index as the low word that is ONE 64-bit compare per pair,
// counted over broadcast LDS reads (four candidates per 16-byte read, every lane the same address) - no sort, no
// branch, no serial dependence on k; cur compares per candidate, one candidate per thread up to 256 nodes.  A
// candidate is selected when its rank is below k; a NaN distance holds the largest key, so it precedes nothing
// (ranks behind every number), and is excluded explicitly.
#include "dist_view.h"

namespace {

constexpr int KNN_MAX_N = 8192;   // the graph's keys in LDS: 32 KB
constexpr int KNN_THREADS = 256;

// a < b <=> knn_key(a) < knn_key(b) for numbers (-0 counts as +0, as in a float compare); NaN -> above every number
__device__ __forceinline__ uint32_t knn_key(float d) {
  if (d != d) return 0xFFFFFFFFu;
  const uint32_t u = __float_as_uint(d + 0.f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool COSINE>
__global__ __launch_bounds__(KNN_THREADS) void k_knn(View vw, const float* __restrict__ dist_param,
                                                     float* __restrict__ adj, float* __restrict__ sel_row,
                                                     float* __restrict__ dist_out, int k, float max_distance, int a0,
                                                     int a1, int b0, int bidirectional, int N, int F) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sK[];   // [N rounded up to 4] keys of the candidates
  const int b = blockIdx.x, tid = threadIdx.x;
  int sh;
  const int cur = view_cur(vw, b, N, sh);
  const int nd = dist_out ? N : cur;   // rows whose distance is wanted (dist_out: all of them, as k_pergraph)
  const float* c = view_cur_row(vw, b, cur, N, F);
  const float sc = dist_param ? dist_param[0] : 1.f;
  float ic = 0.f;
  if (COSINE) {
    float cc = 0.f;
    for (int f = 0; f < F; ++f) {
      const float cv = c[f] / sc;
      cc = fmaf(cv, cv, cc);
    }
    ic = 1.f / fmaxf(sqrtf(cc), 1e-8f);
  }
  for (int j = tid; j < nd; j += KNN_THREADS) {
    const float* n = vw.nodes + ((size_t)b * N + (j + sh < N ? j + sh : N - 1)) * F;
    float d;
    if (!COSINE) {
      float s = 0.f;
      for (int f = 0; f < a1 - a0; ++f) {
        const float t = c[a0 + f] / sc - n[b0 + f] / sc;
        s = fmaf(t, t, s);
      }
      d = sqrtf(s);
    } else {   // torch semantics: normalise each side by max(norm, eps) first
      float nn = 0.f;
      for (int f = 0; f < F; ++f) {
        const float nv = n[f] / sc;
        nn = fmaf(nv, nv, nn);
      }
      const float in = 1.f / fmaxf(sqrtf(nn), 1e-8f);
      float s = 0.f;
      for (int f = 0; f < F; ++f) s = fmaf((c[f] / sc) * ic, (n[f] / sc) * in, s);
      d = 1.f - s;
    }
    if (j < cur) sK[j] = knn_key(d);
    if (dist_out) dist_out[(size_t)b * N + j] = d;
  }
  if (tid < 4 && cur + tid < ((cur + 3) & ~3)) sK[cur + tid] = 0xFFFFFFFFu;   // the last 16-byte read: precede nothing
  __syncthreads();
  const bool capped = !(max_distance == INFINITY);
  const uint32_t kcap = max_distance != max_distance ? 0u : knn_key(max_distance);   // (d < NaN: never)
  for (int j = tid; j < cur; j += KNN_THREADS) {
    const uint32_t kd = sK[j];
    const uint64_t kj = ((uint64_t)kd << 32) | (uint32_t)j;   // (distance, index): ties go to the lower index
    int rank = 0;
    for (int i0 = 0; i0 < cur; i0 += 4) {
      const uint4 q = *reinterpret_cast<const uint4*>(sK + i0);
      rank += ((((uint64_t)q.x << 32) | (uint32_t)i0) < kj) ? 1 : 0;
      rank += ((((uint64_t)q.y << 32) | (uint32_t)(i0 + 1)) < kj) ? 1 : 0;
      rank += ((((uint64_t)q.z << 32) | (uint32_t)(i0 + 2)) < kj) ? 1 : 0;
      rank += ((((uint64_t)q.w << 32) | (uint32_t)(i0 + 3)) < kj) ? 1 : 0;
    }
    const bool hit = kd != 0xFFFFFFFFu && rank < k && (!capped || kd < kcap);
    view_emit(adj, sel_row, b, cur, j, N, hit, bidirectional);
  }
}

}  // namespace

extern "C" int gcm_edge_knn_supported(int mode, int B, int N, int F) {
  const int metric = mode & ((1 << GCM_DIST_KNN_SHIFT) - 1), k = mode >> GCM_DIST_KNN_SHIFT;
  return (metric == GCM_DIST_L2_PERGRAPH || metric == GCM_DIST_COSINE_SIM) && k >= 1 && k <= GCM_DIST_KNN_MAX &&
         B > 0 && N > 0 && F > 0 && N <= KNN_MAX_N;
}

int gcm_knn_run(const View& vw, float* adj, float* sel_row, int mode, float max_distance, const float* dist_param,
                int a0, int a1, int b0, int b1, int bidirectional, float* dist_out, int B, int N, int F,
                hipStream_t stream) {
  const int metric = mode & ((1 << GCM_DIST_KNN_SHIFT) - 1), k = mode >> GCM_DIST_KNN_SHIFT;
  GCM_REQUIRE(!vw.cur_rows && k >= 1 && k <= GCM_DIST_KNN_MAX && B > 0 && N > 0 && F > 0);
  if (metric == GCM_DIST_L2_PERGRAPH) {
    GCM_REQUIRE(a0 >= 0 && a1 > a0 && a1 <= F && b0 >= 0 && b1 <= F && (b1 - b0) == (a1 - a0));
  } else if (metric != GCM_DIST_COSINE_SIM) {
    return GCM_EINVAL;   // the cross-batch mean has no k-nearest form
  }
  if (!gcm_edge_knn_supported(mode, B, N, F)) return GCM_EUNSUPPORTED;
  const size_t lds = sizeof(float) * (size_t)((N + 3) & ~3);
  if (metric == GCM_DIST_L2_PERGRAPH)
    hipLaunchKernelGGL(k_knn<false>, dim3(B), dim3(KNN_THREADS), lds, stream, vw, dist_param, adj, sel_row, dist_out, k,
                       max_distance, a0, a1, b0, bidirectional, N, F);
  else
    hipLaunchKernelGGL(k_knn<true>, dim3(B), dim3(KNN_THREADS), lds, stream, vw, dist_param, adj, sel_row, dist_out, k,
                       max_distance, a0, a1, b0, bidirectional, N, F);
  return gcm_launch_status();
}
