// Back-to-back lean cached steps as ONE graph node: the multi-step form of k_step_rows_cached_img4_lean and
// the capture-time merging that puts steps into it.
//
// A replayed chain of dependent kernel nodes pays ~1.6 us per node that no kernel work buys back.  While a
// stream is being captured the library sees whether step t + 1 follows step t with nothing in between: the stream's only
// pending dependency is then the node step t became.  No captured work can observe the state between the two steps, so
// step t + 1 is appended to that node's argument table (n -> n + 1) instead of being launched; the node runs
// k_step_rows_cached_img4_lean_run, which makes the n steps inside one workgroup per graph.
//
// The kernel's step is the lean kernel's, operation for operation (lean_half_matvec from rows_lean.h, the same source
// order and association, gcm_tanh), so beliefs, records, caches, state and flags are the bits the per-step launches write.
// What changes is where its inputs come from and who makes which step:
//   * in a chain of cached steps a step's layer 1 reads observations alone (its own and those of the rows cur - hop) and
//     its layer 2 the h1 rows of those same rows (a layer-1 row is final once written), so inside one launch
//     the steps do not wait for one another: the workgroup's eight waves take the steps t = w, w + 8, ... each, in three
//     phases with a workgroup barrier between them - observations into LDS; layer 1 of every step; layer 2 of every step;
//   * the graph's x and h1 rows live in LDS by row (2 x N x 32 floats <= 32 KB): the rows from before the run's first
//     step - at most max(hop) of them - are loaded from nodes / cH up front, a step's own rows are written there by the
//     wave that makes it, and the source rows are read from there behind the barrier.  Nothing this launch stored to
//     global memory is read back (the vector L1 may still hold the old line);
//   * weights and biases are loaded once per wave and stay in registers; every global load of the launch - observations
//     (two steps per instruction: half-waves), earlier rows, weights - is issued before the first wait, and every store
//     is fire and forget: loads and stores share one in-order vmcnt on this ISA (rollout_persist.hip), so a load behind
//     stores would drain them;
//   * what follows from cur and the hops alone (adjacency entries, the record's live list / coefficients / header) is
//     written by the step's wave at the end, the count once with the run's last value.
#include <atomic>
#include <new>

#include "fused_common.h"
#include "gcm_common.h"
#include "rows_common.h"
#include "rows_lean.h"

namespace gcm_rows {

constexpr int RUN_CAP = GCM_ROWS_MAX_STEPS;   // two tables of 128 pointers: 2 KB of the 4 KB of kernel arguments
constexpr int RUN_WAVES = 8;
constexpr int RUN_PAIRS = RUN_CAP / 2 / RUN_WAVES;   // observation loads per wave (two steps each)

struct RunTable {
  const float* obs[RUN_CAP];
  float* rec[RUN_CAP];
};

// hops4: the distinct hops 0 < h < 128 ASCENDING, one byte each, 0xff in the unused slots.  nhs: N | H2 << 8 | self << 16.
// Steps t < n <= RUN_CAP: row cur0 + t < N, observation tab.obs[t] [B, 32], record tab.rec[t] (o_*: CachedLayout;
// rec = 0: mx alone).
__global__ __launch_bounds__(64 * RUN_WAVES) void k_step_rows_cached_img4_lean_run(
    const float* __restrict__ image, float* __restrict__ nodes, float* __restrict__ cH, const float* __restrict__ params,
    int cur0, int n, unsigned hops4, unsigned nhs, float* __restrict__ adj, int64_t* __restrict__ count,
    float* __restrict__ cA, float* __restrict__ cX, uint32_t* __restrict__ flags, unsigned o_v, unsigned o_hdr,
    unsigned o_coef, unsigned o_live, int rec, RunTable tab) {
  constexpr int F = 32, H1 = 32, ROWS = 128 * 32;
  __shared__ __attribute__((aligned(16))) float sXH[2 * ROWS];            // x rows [128][32] | h1 rows [128][32]
  __shared__ __attribute__((aligned(16))) float svw[RUN_WAVES * 128];     // each wave's lane exchange
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float* sv = svw + 128 * wv;
  const unsigned gb = blockIdx.x;
  const unsigned N = nhs & 0xffu;
  const int H2 = (int)((nhs >> 8) & 0xffu);
  const bool self = (nhs >> 16) & 1u;
  const unsigned g0 = gb * N;
  const int fl = lane & 31, kh = lane >> 5;
  const int ol = lane < H2 ? lane : H2 - 1;
  // ---- phase A: every global load of the launch ------------------------------------------------------------------
  // the observations, pair p = steps 2 p (lanes 0 - 31) and 2 p + 1 (lanes 32 - 63): this wave's are p = w, w + 8, ...
  float xo[RUN_PAIRS];
#pragma unroll
  for (int j = 0; j < RUN_PAIRS; ++j) {
    const int p = wv + RUN_WAVES * j;
    const int ta = 2 * p < n ? 2 * p : n - 1, tb = 2 * p + 1 < n ? 2 * p + 1 : n - 1;
    const float* pa = tab.obs[ta];
    const float* pb = tab.obs[tb];
    xo[j] = (kh ? pb : pa)[gb * F + fl];
  }
  const f32x2* i3 = reinterpret_cast<const f32x2*>(image + 2 * 4 * 64 * 64);   // image3 (k_cached_weight_image)
  f32x2 w1[16], w2[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) w1[k] = i3[k * 64 + lane];
  const float* b1 = params + 2 * H1 * F;
  const float bias1 = b1[fl];
#pragma unroll
  for (int k = 0; k < 16; ++k) w2[k] = i3[(16 + k) * 64 + lane];
  const float bias2 = b1[H1 + 2 * H2 * H1 + ol];
  // the rows from before the run that a step of it can read: [cur0 - max(hop), cur0), x (lanes 0 - 31) and h1 (32 - 63)
  {
    int hmax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int h = (int)((hops4 >> (8 * i)) & 0xffu);
      if (h != 0xff && h > hmax) hmax = h;
    }
    const int lo = cur0 - hmax > 0 ? cur0 - hmax : 0;
    const float* src = kh ? cH : nodes;
    for (int r = lo + wv; r < cur0; r += RUN_WAVES) sXH[kh * ROWS + r * 32 + fl] = src[(g0 + (unsigned)r) * 32 + fl];
  }
#pragma unroll
  for (int j = 0; j < RUN_PAIRS; ++j) {   // the observations: x rows in LDS, rows of the node matrix and of its cache
    const int t = 2 * (wv + RUN_WAVES * j) + kh;   // (rows cur and cur + 1 are 64 consecutive floats)
    if (t < n) {
      sXH[(cur0 + t) * 32 + fl] = xo[j];
      const unsigned at = (g0 + (unsigned)(cur0 + t)) * F + fl;
      nodes[at] = xo[j];
      cX[at] = xo[j];
    }
  }
  __syncthreads();
  // the source rows of row cur, ascending and compacted as the lean kernel's host resolves them: the k hops <= cur are
  // the first k of the ascending list, slot q holds row cur - hop[k - 1 - q]; an empty slot reads row 0 and adds nothing
  auto sources = [&](int cur, const float* rows, float (&va)[4]) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) k += (int)(((hops4 >> (8 * i)) & 0xffu) <= (unsigned)cur);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = k - 1 - q;
      const bool any = idx >= 0;
      const int s = any ? cur - (int)((hops4 >> (8 * (idx & 3))) & 0xffu) : 0;
      const float v = rows[s * 32 + fl];
      va[q] = any ? v : 0.f;
    }
  };
  // ---- phase B: layer 1 of this wave's steps (reads x rows, writes h1 rows) ------------------------------------------
  for (int t = wv; t < n; t += RUN_WAVES) {
    const int cur = cur0 + t;
    const unsigned rc = g0 + (unsigned)cur;
    float xa[4];
    sources(cur, sXH, xa);
    const float xc = sXH[cur * 32 + fl];
    asm volatile("" ::: "memory");
    // (the sums img4b's mask walk makes: sources ascending, (v0 + v1) + (v2 + v3))
    float agg1 = (xa[0] + xa[1]) + (xa[2] + xa[3]);
    agg1 = lane < F ? agg1 + (self ? xc : 0.f) : 0.f;
    if (lane < F) *reinterpret_cast<f32x2*>(sv + 2 * lane) = f32x2{agg1, xc};
    asm volatile("" ::: "memory");   // (lanes exchange through LDS; one wave: its LDS operations execute in order)
    const float p1 = bias1 + lean_half_matvec(w1, sv, kh);   // (all 64 lanes: the halves meet across lanes 0 - 63)
    const float h1c = lane < H1 ? gcm_tanh(p1) : 0.f;
    asm volatile("" ::: "memory");
    if (lane < H1) sXH[ROWS + cur * 32 + lane] = h1c;
    if (lane < F) cA[rc * F + lane] = agg1;
    if (lane < H1) cH[rc * H1 + lane] = h1c;
  }
  __syncthreads();
  // ---- phase C: layer 2 of this wave's steps (reads h1 rows) --------------------------------------------------------
  bool bad = false;
  for (int t = wv; t < n; t += RUN_WAVES) {
    const int cur = cur0 + t;
    float* saved = tab.rec[t];
    float ha[4];
    sources(cur, sXH + ROWS, ha);
    const float h1r = sXH[ROWS + cur * 32 + fl];
    asm volatile("" ::: "memory");
    const float h1c = lane < H1 ? h1r : 0.f;
    float agg2 = (ha[0] + ha[1]) + (ha[2] + ha[3]);
    agg2 = lane < H1 ? agg2 + (self ? h1c : 0.f) : 0.f;
    if (lane < H1) *reinterpret_cast<f32x2*>(sv + 2 * lane) = f32x2{agg2, h1c};
    asm volatile("" ::: "memory");
    const float p2 = bias2 + lean_half_matvec(w2, sv, kh);
    const float v = gcm_tanh(p2);
    asm volatile("" ::: "memory");
    if (lane < H2) saved[gb * H2 + lane] = v;
    if (rec && lane < H1) {
      saved[o_v + gb * 2 * H1 + lane] = agg2;
      saved[o_v + gb * 2 * H1 + H1 + lane] = h1c;
    }
    bad = bad || (lane < H2 && !isfinite(v));
  }
  // ---- phase D: what follows from cur and the hops alone, for this wave's steps -------------------------------------
  for (int t = wv; t < n; t += RUN_WAVES) {
    const int cur = cur0 + t;
    const unsigned rc = g0 + (unsigned)cur;
    float* saved = tab.rec[t];
    unsigned long long m0 = 0ull, m1 = 0ull;   // the sources of row cur: j = cur - h >= 0
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int h = (int)((hops4 >> (8 * i)) & 0xffu);
      if (h <= cur) {
        const int j = cur - h;
        if (j < 64) m0 |= 1ull << j;
        else m1 |= 1ull << (j - 64);
      }
    }
    float* arow = adj + (size_t)rc * N;
    const unsigned long long s0 = m0 | ((self && cur < 64) ? 1ull << cur : 0ull);
    const unsigned long long s1 = m1 | ((self && cur >= 64) ? 1ull << (cur - 64) : 0ull);
    if (lane < (int)N && ((s0 >> lane) & 1ull)) arow[lane] = 1.f;
    if (lane + 64 < (int)N && ((s1 >> lane) & 1ull)) arow[lane + 64] = 1.f;
    if (rec) {
      const unsigned long long l0 = m0 | (cur < 64 ? 1ull << cur : 0ull), l1 = m1 | (cur >= 64 ? 1ull << (cur - 64) : 0ull);
      int* live = reinterpret_cast<int*>(saved + o_live) + gb * N;
      float* coef = saved + o_coef + gb * N;
      const int j0 = lane, j1 = lane + 64;
      const bool in0 = (l0 >> lane) & 1ull, in1 = (l1 >> lane) & 1ull;
      const int pos0 = __popcll(l0 & ((1ull << lane) - 1ull));
      const int pos1 = __popcll(l0) + __popcll(l1 & ((1ull << lane) - 1ull));
      if (in0) { live[pos0] = j0; coef[pos0] = (j0 == cur && !self) ? 0.f : 1.f; }
      if (in1) { live[pos1] = j1; coef[pos1] = (j1 == cur && !self) ? 0.f : 1.f; }
      if (lane == 0) {
        int* hdr = reinterpret_cast<int*>(saved + o_hdr) + 4 * gb;
        const int L = __popcll(l0) + __popcll(l1);
        const int l_cur = cur < 64 ? __popcll(l0 & ((1ull << cur) - 1ull)) : __popcll(l0) + __popcll(l1 & ((1ull << (cur - 64)) - 1ull));
        hdr[0] = L; hdr[1] = l_cur; hdr[2] = cur; hdr[3] = 0;
      }
    }
  }
  if (threadIdx.x == 0) count[gb] = cur0 + n;   // (nothing can observe the values in between)
  const bool nonfinite = __any(bad);
  if (nonfinite && lane == 0) atomicOr(flags, GCM_FLAG_NONFINITE);
}

// ---- the host side: one run object per chain --------------------------------------------------------------------
struct Run {
  // the remembered node: valid only while the stream's capture is `cid`
  hipGraphNode_t node = nullptr;
  unsigned long long cid = 0;
  hipStream_t stream = nullptr;
  int n = 0, cur0 = 0;
  // what a step must share with the node to continue it
  float *nodes = nullptr, *adj = nullptr, *cH = nullptr, *cA = nullptr, *cX = nullptr;
  int64_t* count = nullptr;
  const float *params = nullptr, *image = nullptr;
  uint32_t* flags = nullptr;
  int B = 0, N = 0, H2 = 0, self = 0, rec = 0;
  unsigned hops4 = 0xffffffffu;
  RunTable tab;
  int cap = RUN_CAP;
  // counters of the capture seen last
  unsigned long long stat_cid = 0;
  int stat_nodes = 0, stat_merged = 0;
};

// a graph call failed once: every later step of the process is a launch of its own
static std::atomic<bool> g_merge_ok{true};
static std::atomic<int> g_route{0}, g_last_error{0};   // 1: node edited in place, 2: node replaced; the last graph error

static void merge_off(hipError_t e) {
  g_last_error = (int)e;
  g_merge_ok = false;
  (void)hipGetLastError();
}

// n steps of R (tab filled up to n) as the parameters of a kernel node
struct RunArgs {
  int cur0, n, rec;
  unsigned hops4, nhs, o_v, o_hdr, o_coef, o_live;
  void* ptr[19];
  hipKernelNodeParams p;
};
static void fill_args(Run& R, int n, RunArgs& a) {
  const CachedLayout lay = make_cached_layout(R.B, R.N, 32, R.H2);
  a.cur0 = R.cur0;
  a.n = n;
  a.rec = R.rec;
  a.hops4 = R.hops4;
  a.nhs = (unsigned)R.N | (unsigned)R.H2 << 8 | (R.self ? 1u << 16 : 0u);
  a.o_v = (unsigned)lay.o_v; a.o_hdr = (unsigned)lay.o_hdr; a.o_coef = (unsigned)lay.o_coef; a.o_live = (unsigned)lay.o_live;
  void* ptr[19] = {&R.image, &R.nodes, &R.cH, &R.params, &a.cur0, &a.n, &a.hops4, &a.nhs, &R.adj, &R.count,
                   &R.cA,    &R.cX,    &R.flags, &a.o_v, &a.o_hdr, &a.o_coef, &a.o_live, &a.rec, &R.tab};
  for (int i = 0; i < 19; ++i) a.ptr[i] = ptr[i];
  a.p = hipKernelNodeParams{};
  a.p.func = (void*)k_step_rows_cached_img4_lean_run;
  a.p.gridDim = dim3(R.B);
  a.p.blockDim = dim3(64 * RUN_WAVES);
  a.p.sharedMemBytes = 0;
  a.p.kernelParams = a.ptr;
  a.p.extra = nullptr;
}

// The remembered node now runs n steps.  First by editing it in place (hipGraphKernelNodeSetParams); if the runtime
// refuses that, by a new node on the old one's dependencies that takes its place as the stream's pending dependency.
// ROCm 7.2 accepts the edit of a node under capture while function and block size stay as they are, and refuses it with
// hipErrorLaunchFailure (719) when the node goes from the lean kernel's 128 threads to this kernel's 512: the second
// route is the one that runs there, and once it has, it is taken straight away.  The old node is replaced only while
// nothing depends on it (a fork recorded behind step t on another stream would): else the step starts a new run.
// false: nothing changed; the step is then a launch of its own (and after a failed graph call merging is off)
static bool grow_node(Run& R, int n, hipGraph_t graph) {
  RunArgs a;
  fill_args(R, n, a);
  if (g_route.load() != 2) {
    const hipError_t e = hipGraphKernelNodeSetParams(R.node, &a.p);
    if (e == hipSuccess) {
      g_route = 1;
      return true;
    }
    g_last_error = (int)e;
    (void)hipGetLastError();
    if (g_route.load() == 1) {   // (it worked before: not a question of the route)
      merge_off(e);
      return false;
    }
  }
  size_t nd = 0, n_dependent = 0;
  hipError_t e = hipGraphNodeGetDependentNodes(R.node, nullptr, &n_dependent);
  if (e == hipSuccess && n_dependent) return false;
  if (e == hipSuccess) e = hipGraphNodeGetDependencies(R.node, nullptr, &nd);
  hipGraphNode_t deps[8];
  if (e == hipSuccess && nd > 8) e = hipErrorInvalidValue;
  if (e == hipSuccess && nd) e = hipGraphNodeGetDependencies(R.node, deps, &nd);
  hipGraphNode_t fresh = nullptr;
  if (e == hipSuccess) e = hipGraphAddKernelNode(&fresh, graph, nd ? deps : nullptr, nd, &a.p);
  if (e != hipSuccess) {
    merge_off(e);
    return false;
  }
  e = hipStreamUpdateCaptureDependencies(R.stream, &fresh, 1, hipStreamSetCaptureDependencies);
  if (e != hipSuccess) {
    (void)hipGraphDestroyNode(fresh);
    merge_off(e);
    return false;
  }
  e = hipGraphDestroyNode(R.node);
  if (e != hipSuccess) {   // put the stream back on the old node
    hipGraphNode_t old = R.node;
    (void)hipStreamUpdateCaptureDependencies(R.stream, &old, 1, hipStreamSetCaptureDependencies);
    (void)hipGraphDestroyNode(fresh);
    merge_off(e);
    return false;
  }
  R.node = fresh;
  g_route = 2;
  return true;
}

// [p, p + floats) and [q, q + floats2) share an address
static bool overlap(const float* p, size_t floats, const float* q, size_t floats2) {
  return p < q + floats2 && q < p + floats;
}

// Inside one launch the steps are not ordered against one another (each wave makes every eighth step, the
// observations are all read up front), so a step may join a run only if it shares no memory with the run's earlier
// steps in a way the order of the per-step launches would have resolved: its record must not lie on an earlier step's
// record (the later write must win) or observation (read before it is overwritten), and its observation must not lie
// on an earlier step's record (a belief fed back as the next observation).  The caching allocator hands a block freed
// during a capture out again without a node of its own, so this does happen: records of a no_grad loop that keeps
// only its last belief alternate between two addresses.
static bool shares_memory(const Run& R, const float* obs, const float* saved, size_t obs_floats, size_t rec_floats) {
  for (int t = 0; t < R.n; ++t)
    if (overlap(saved, rec_floats, R.tab.rec[t], rec_floats) || overlap(saved, rec_floats, R.tab.obs[t], obs_floats) ||
        overlap(obs, obs_floats, R.tab.rec[t], rec_floats))
      return true;
  return false;
}

}  // namespace gcm_rows

extern "C" int gcm_rows_run_steps_cap(void) { return gcm_rows::RUN_CAP; }
extern "C" void* gcm_rows_run_create(void) { return new (std::nothrow) gcm_rows::Run(); }
extern "C" int gcm_rows_run_destroy(void* run) {
  delete static_cast<gcm_rows::Run*>(run);
  return GCM_OK;
}
extern "C" int gcm_rows_run_reset(void* run) {
  GCM_REQUIRE(run);
  static_cast<gcm_rows::Run*>(run)->node = nullptr;
  return GCM_OK;
}
extern "C" int gcm_rows_run_set_cap(void* run, int cap) {
  GCM_REQUIRE(run && cap >= 1 && cap <= gcm_rows::RUN_CAP);
  static_cast<gcm_rows::Run*>(run)->cap = cap;
  return GCM_OK;
}
extern "C" int gcm_rows_run_stats(const void* run, int* out2) {
  GCM_REQUIRE(run && out2);
  const gcm_rows::Run* R = static_cast<const gcm_rows::Run*>(run);
  out2[0] = R->stat_nodes;
  out2[1] = R->stat_merged;
  return GCM_OK;
}
extern "C" int gcm_rows_run_enabled(void) { return gcm_rows::g_merge_ok.load() ? 1 : 0; }
extern "C" int gcm_rows_run_route(int* out2) {
  GCM_REQUIRE(out2);
  out2[0] = gcm_rows::g_route.load();
  out2[1] = gcm_rows::g_last_error.load();
  return GCM_OK;
}

extern "C" int gcm_dense_rows_step_cached_run(void* run, const float* obs, float* nodes, float* adj, int64_t* count,
                                              const gcm_selector_desc* selectors, int n_selectors, const float* params,
                                              const float* weight_image, int has_bias, int act1, int act2,
                                              float* cache_h1, float* cache_agg1, float* cache_nodes, float* saved,
                                              int record, int cur_host, uint32_t* flags, void* workspace,
                                              size_t workspace_bytes, int B, int N, int F, int H1, int H2,
                                              gcm_stream_t stream) {
  using namespace gcm_rows;
  auto plain = [&]() {
    return gcm_dense_rows_step_cached_ws(obs, nodes, adj, count, selectors, n_selectors, params, weight_image, has_bias,
                                         act1, act2, cache_h1, cache_agg1, cache_nodes, saved, record, cur_host, flags,
                                         workspace, workspace_bytes, B, N, F, H1, H2, stream);
  };
  Run* R = static_cast<Run*>(run);
  if (!R || !g_merge_ok.load()) return plain();
  hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long cid = 0;
  hipGraph_t graph = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  hipError_t e = hipStreamGetCaptureInfo_v2(st, &cs, &cid, &graph, &deps, &nd);
  if (e != hipSuccess) {
    merge_off(e);
    return plain();
  }
  if (cs != hipStreamCaptureStatusActive) {   // eager: exactly today's path
    R->node = nullptr;
    R->stat_cid = 0;
    R->stat_nodes = R->stat_merged = 0;
    return plain();
  }
  // the lean case, as gcm_dense_rows_step_cached_ws decides it
  GCM_REQUIRE(obs && nodes && adj && count && params && cache_h1 && cache_agg1 && cache_nodes && saved && flags);
  GCM_REQUIRE(B > 0 && (selectors || n_selectors == 0));
  LeanCase lc;
  CachedLayout lay = make_cached_layout(B, N, H1, H2);
  const bool lean = gcm_dense_rows_cached_supported_ws(selectors, n_selectors, has_bias, N, F, H1, H2) &&
                    (size_t)B * N * (size_t)(F > N ? F : N) < ((size_t)1 << 31) && lay.total < ((size_t)1 << 31) &&
                    lean_step_case(selectors, n_selectors, weight_image, has_bias, act1, act2, N, F, H1, H2, cur_host, lc);
  if (!lean) {
    R->node = nullptr;
    return plain();
  }
  const int self = lc.self;
  unsigned hops4 = 0xffffffffu;
  for (int a = 0; a < lc.nh; ++a) hops4 = (hops4 & ~(0xffu << (8 * a))) | (unsigned)lc.hops[a] << (8 * a);
  const size_t obs_floats = (size_t)B * F, rec_floats = record ? lay.total : (size_t)B * H2;
  // (an observation that is a view of the state or the caches this chain writes: a row an earlier step made)
  const size_t rows_floats = (size_t)B * N * 32;
  const bool obs_in_state = overlap(obs, obs_floats, nodes, rows_floats) || overlap(obs, obs_floats, cache_nodes, rows_floats) ||
                            overlap(obs, obs_floats, cache_h1, rows_floats) || overlap(obs, obs_floats, cache_agg1, rows_floats) ||
                            overlap(obs, obs_floats, adj, (size_t)B * N * N);
  if (R->stat_cid != cid) {
    R->stat_cid = cid;
    R->stat_nodes = R->stat_merged = 0;
  }
  // (a handle is looked at only while the stream's capture is the one it was made in)
  const bool follows = R->node && R->cid == cid && R->stream == st && nd == 1 && deps[0] == R->node &&
                       cur_host == R->cur0 + R->n && R->n < R->cap && R->n < RUN_CAP && R->nodes == nodes &&
                       R->adj == adj && R->count == count && R->cH == cache_h1 && R->cA == cache_agg1 &&
                       R->cX == cache_nodes && R->params == params && R->image == weight_image && R->flags == flags &&
                       R->B == B && R->N == N && R->H2 == H2 && R->self == self && R->hops4 == hops4 &&
                       R->rec == (record ? 1 : 0) && !obs_in_state &&
                       !shares_memory(*R, obs, saved, obs_floats, rec_floats);
  if (follows) {
    R->tab.obs[R->n] = obs;
    R->tab.rec[R->n] = saved;
    if (grow_node(*R, R->n + 1, graph)) {
      ++R->n;
      ++R->stat_merged;
      return GCM_OK;
    }
  }
  // a new run: the lean kernel, captured as gcm_dense_rows_step_cached_ws captures it, and its node remembered
  R->node = nullptr;
  if (!record) lay.total = 0;
  const int rc = launch_step_cached_lean(obs, nodes, adj, count, lc.m0, lc.m1, self, params, weight_image, cache_h1,
                                         cache_agg1, cache_nodes, saved, lay, flags, B, N, H2, cur_host, st);
  if (rc == GCM_EUNSUPPORTED) return plain();
  if (rc) return rc;
  ++R->stat_nodes;
  if (!g_merge_ok.load()) return GCM_OK;
  unsigned long long cid2 = 0;
  e = hipStreamGetCaptureInfo_v2(st, &cs, &cid2, &graph, &deps, &nd);
  if (e != hipSuccess) {
    merge_off(e);
    return GCM_OK;
  }
  if (cs != hipStreamCaptureStatusActive || cid2 != cid || nd != 1) return GCM_OK;
  hipGraphNode_t node = deps[0];
  hipGraphNodeType type;
  hipKernelNodeParams got;
  if ((e = hipGraphNodeGetType(node, &type)) != hipSuccess ||
      (type == hipGraphNodeTypeKernel && (e = hipGraphKernelNodeGetParams(node, &got)) != hipSuccess)) {
    merge_off(e);
    return GCM_OK;
  }
  if (type != hipGraphNodeTypeKernel || got.func != lean_step_kernel()) return GCM_OK;
  R->node = node;
  R->cid = cid;
  R->stream = st;
  R->n = 1;
  R->cur0 = cur_host;
  R->nodes = nodes; R->adj = adj; R->count = count; R->cH = cache_h1; R->cA = cache_agg1; R->cX = cache_nodes;
  R->params = params; R->image = weight_image; R->flags = flags;
  R->B = B; R->N = N; R->H2 = H2; R->self = self; R->rec = record ? 1 : 0;
  R->hops4 = hops4;
  R->tab.obs[0] = obs;
  R->tab.rec[0] = saved;
  return GCM_OK;
}
