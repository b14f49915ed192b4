// Sparse spatial selectors (src/gcm/sparse_edge_selectors/spatial.py: SpatialKNNEdge, SpatialRadiusEdge).
// The reference loops over graphs in Python around PyG's knn / a pairwise distance; here every graph is one
// workgroup that stages its positions in LDS and gives each of its rows (sink nodes) to one wave at a time:
//   count: the wave evaluates the row's candidates 64 at a time (ballot + popcount), keeps the row count in LDS,
//          wave 0 scans the rows -> row_off [B, N] (within the graph) and the graph's total; a one-workgroup
//          pass scans the totals over B -> edge_off [B+1] (+ max(T_b + tau_b) behind it, for the overflow check).
//          kNN: the wave also selects the row's k-th smallest key (d2 bits << 32 | j) over all candidates by a
//          bitwise radix search on the squared distances held in registers, and stores it in kth [B, N].
//   fill : the same predicate again, every edge written at base + (set lanes below it) (mbcnt): ascending
//          sources inside ascending sinks inside ascending graphs = coalesced COO order, no sort.
// The squared distance is d = x_i - x_j per column, squared and added in column order with contraction off
// (`#pragma clang fp contract(off)` in Row::d2): bit-identical to the reference's fp32 ((s - t) ** 2).sum(-1) for the
// P = 2 / 3 positions it is used with; the radius test takes the correctly rounded square root (see within()).
#include "gcm_common.h"

namespace {

constexpr int kWaves = 8;              // waves per workgroup (one workgroup per graph)
constexpr int kThreads = 64 * kWaves;

struct Cols {
  int32_t c[GCM_SPATIAL_MAX_COLS];
};

// (n, t0) of graph b, clamped to the node matrix (max(T + tau) > N is reported by the offsets pass instead)
__device__ __forceinline__ void graph_extent(const int64_t* T, const int64_t* taus, int b, int N, int& t0, int& n) {
  int64_t t = T[b], tau = taus[b];
  t = t < 0 ? 0 : (t > N ? N : t);
  tau = tau < 0 ? 0 : tau;
  const int64_t e = t + tau;
  n = (int)(e > N ? N : e);
  t0 = (int)t;
}

// stage pos[b, 0:n, cols] column-major: lds[p * npad + j]
__device__ __forceinline__ void stage_positions(float* lds, const float* __restrict__ nodes, const Cols& cols,
                                                int P, int b, int n, int N, int F, int npad) {
  const float* g = nodes + (size_t)b * N * F;
  for (int p = 0; p < P; ++p) {
    const int col = cols.c[p];
    for (int j = threadIdx.x; j < n; j += kThreads) lds[p * npad + j] = g[(size_t)j * F + col];
  }
}

// the sink row's coordinates in registers for PC = P in {2, 3}; read from LDS for any other P (PC = 0)
template <int PC>
struct Row {
  float x[PC > 0 ? PC : 1];
  int i;
  __device__ __forceinline__ void load(const float* lds, int npad, int i_) {
    i = i_;
#pragma unroll
    for (int p = 0; p < PC; ++p) x[p] = lds[p * npad + i_];
  }
  // sum over columns in order of (x_i - x_j)^2, every product rounded before the add.  The pragma is what keeps
  // it that way: hipcc's HIP default is -ffp-contract=fast-honor-pragmas, and __fmul_rn / __fadd_rn are plain
  // `*` / `+` in this toolchain's headers, so without it s + d * d becomes v_fma_f32 / v_pk_fma_f32 (the ISA of
  // every instantiation is free of them now; tests/test_spatial_sparse_gpu.py pins pairs where the two differ).
  __device__ __forceinline__ float d2(const float* lds, int npad, int P, int j) const {
#pragma clang fp contract(off)
    float s = 0.f;
    if constexpr (PC > 0) {
#pragma unroll
      for (int p = 0; p < PC; ++p) {
        const float d = x[p] - lds[p * npad + j];
        s = s + d * d;
      }
    } else {
      for (int p = 0; p < P; ++p) {
        const float d = lds[p * npad + i] - lds[p * npad + j];
        s = s + d * d;
      }
    }
    return s;
  }
};

// sqrtf, not __fsqrt_rn: on gfx950 the latter compiles to the bare v_sqrt_f32 (1 ulp), sqrtf to v_sqrt_f32 plus
// the two fma residual corrections (correctly rounded, like the reference's CPU sqrt)
__device__ __forceinline__ bool within(float d2, float radius) { return sqrtf(d2) < radius; }

__device__ __forceinline__ int lanes_below(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// kNN: the k-th smallest key (d2 bits << 32 | j) of row i over the candidates [0, n) (all of them when k >= n).
// d[r] = d2 bits of candidate r * 64 + lane (0xFFFFFFFF past n).  Wave-uniform result.
template <int M>
__device__ __forceinline__ uint64_t kth_key(const uint32_t (&d)[M], int n, int k, int lane) {
  if (k >= n) return ~0ull;
  // D = the k-th smallest d2 (with multiplicity): the largest D with #{d < D} < k.  Valid d2 are non-negative
  // floats (bit 31 clear), the padding sentinel never counts.
  uint32_t D = 0;
  for (int bit = 30; bit >= 0; --bit) {
    const uint32_t t = D | (1u << bit);
    int c = 0;
#pragma unroll
    for (int r = 0; r < M; ++r) c += __popcll(__ballot(d[r] < t));
    if (c < k) D = t;
  }
  int need = k;
#pragma unroll
  for (int r = 0; r < M; ++r) need -= __popcll(__ballot(d[r] < D));
  // ties at D: the need-th lowest index among them (1 <= need <= #{d == D})
  int jstar = 0;
  bool found = false;
#pragma unroll
  for (int r = 0; r < M; ++r) {
    const uint64_t m = __ballot(d[r] == D);
    const int pc = __popcll(m);
    if (!found) {
      if (need <= pc) {
        const uint64_t hit = __ballot(((m >> lane) & 1ull) && lanes_below(m) == need - 1);
        jstar = r * 64 + __ffsll((unsigned long long)hit) - 1;
        found = true;
      } else {
        need -= pc;
      }
    }
  }
  return ((uint64_t)D << 32) | (uint32_t)jstar;
}

// rows of graph b: the new nodes [t0, n) (causal modes) or every node [0, n) (radius, non-causal)
template <int MODE>
__device__ __forceinline__ int row_lo(int t0) { return MODE == GCM_SPATIAL_RADIUS_ALL ? 0 : t0; }

template <int MODE, int PC, int M>
__global__ __launch_bounds__(kThreads) void k_spatial_count(
    const float* __restrict__ nodes, const int64_t* __restrict__ T, const int64_t* __restrict__ taus, Cols cols,
    int P, float radius, int k, int32_t* __restrict__ row_off, uint64_t* __restrict__ kth,
    int64_t* __restrict__ edge_off, int N, int F, int npad) {
  extern __shared__ float lds[];           // [P][npad] positions, then [npad] row counts
  int* cnt = (int*)(lds + (size_t)P * npad);
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int t0, n;
  graph_extent(T, taus, b, N, t0, n);
  stage_positions(lds, nodes, cols, P, b, n, N, F, npad);
  __syncthreads();
  const int lo = row_lo<MODE>(t0);
  for (int r = lo + wave; r < n; r += kWaves) {
    Row<PC> row;
    row.load(lds, npad, r);
    int c = 0;
    if constexpr (MODE == GCM_SPATIAL_RADIUS_CAUSAL) {          // sources j < r
      for (int j0 = 0; j0 < r; j0 += 64) {
        const int j = j0 + lane;
        c += __popcll(__ballot(j < r && within(row.d2(lds, npad, P, j), radius)));
      }
    } else if constexpr (MODE == GCM_SPATIAL_RADIUS_ALL) {      // sources: the new nodes [t0, n)
      for (int j0 = t0; j0 < n; j0 += 64) {
        const int j = j0 + lane;
        c += __popcll(__ballot(j < n && within(row.d2(lds, npad, P, j), radius)));
      }
    } else {                                                    // kNN over [0, n), then sources j < r
      uint32_t d[M];
#pragma unroll
      for (int q = 0; q < M; ++q) {
        const int j = q * 64 + lane;
        d[q] = j < n ? __float_as_uint(row.d2(lds, npad, P, j)) : 0xFFFFFFFFu;
      }
      const uint64_t key = kth_key<M>(d, n, k, lane);
#pragma unroll
      for (int q = 0; q < M; ++q) {
        const int j = q * 64 + lane;
        c += __popcll(__ballot(j < r && ((((uint64_t)d[q]) << 32) | (uint32_t)j) <= key));
      }
      if (lane == 0) kth[(size_t)b * N + r] = key;
    }
    if (lane == 0) cnt[r] = c;
  }
  __syncthreads();
  if (wave != 0) return;
  // exclusive scan of the row counts, 64 rows at a time
  int carry = 0;
  for (int r0 = lo; r0 < n; r0 += 64) {
    const int r = r0 + lane;
    const int v = r < n ? cnt[r] : 0;
    int incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const int t = __shfl_up(incl, s);
      if (lane >= s) incl += t;
    }
    if (r < n) row_off[(size_t)b * N + r] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (lane == 0) edge_off[b] = carry;      // the graph's total (scanned over B by k_spatial_offsets)
}

// edge_off[0:B] holds the per-graph totals: exclusive scan in place, edge_off[B] = E, edge_off[B+1] = max(T + tau).
// max(T + tau) <= 1 is the reference's early return (spatial.py:30, 82): no edges at all, for every mode.
__global__ __launch_bounds__(256) void k_spatial_offsets(const int64_t* __restrict__ T,
                                                         const int64_t* __restrict__ taus,
                                                         int64_t* __restrict__ edge_off, int B) {
  __shared__ int64_t wsum[4], wmax[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (B + 255) / 256;
  const int b0 = min(B, (int)threadIdx.x * per), b1 = min(B, b0 + per);
  int64_t s = 0, mx = 0;
  for (int b = b0; b < b1; ++b) {
    s += edge_off[b];
    const int64_t e = T[b] + (taus[b] > 0 ? taus[b] : 0);
    mx = e > mx ? e : mx;
  }
  int64_t incl = s;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int lo = __shfl_up((int)(incl & 0xffffffffll), d), hi = __shfl_up((int)(incl >> 32), d);
    const int64_t t = ((int64_t)hi << 32) | (uint32_t)lo;
    if (lane >= d) incl += t;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int lo = __shfl_xor((int)(mx & 0xffffffffll), d), hi = __shfl_xor((int)(mx >> 32), d);
    const int64_t t = ((int64_t)hi << 32) | (uint32_t)lo;
    mx = t > mx ? t : mx;
  }
  if (lane == 63) wsum[wave] = incl;
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  int64_t before = 0, total = 0, gmax = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += wsum[w];
    total += wsum[w];
    gmax = wmax[w] > gmax ? wmax[w] : gmax;
  }
  const bool none = gmax <= 1;
  int64_t run = before + incl - s;
  for (int b = b0; b < b1; ++b) {
    const int64_t v = edge_off[b];
    edge_off[b] = none ? 0 : run;
    run += v;
  }
  if (threadIdx.x == 0) {
    edge_off[B] = none ? 0 : total;
    edge_off[B + 1] = gmax;
  }
}

template <int MODE, int PC>
__global__ __launch_bounds__(kThreads) void k_spatial_fill(
    const float* __restrict__ nodes, const int64_t* __restrict__ T, const int64_t* __restrict__ taus, Cols cols,
    int P, float radius, const int32_t* __restrict__ row_off, const uint64_t* __restrict__ kth,
    const int64_t* __restrict__ edge_off, int64_t* __restrict__ indices, int64_t E, int N, int F, int npad) {
  extern __shared__ float lds[];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t g0 = edge_off[b], g1 = edge_off[b + 1];
  if (g1 == g0) return;
  int t0, n;
  graph_extent(T, taus, b, N, t0, n);
  stage_positions(lds, nodes, cols, P, b, n, N, F, npad);
  __syncthreads();
  for (int r = row_lo<MODE>(t0) + wave; r < n; r += kWaves) {
    Row<PC> row;
    row.load(lds, npad, r);
    int64_t base = g0 + row_off[(size_t)b * N + r];
    const int j_lo = MODE == GCM_SPATIAL_RADIUS_ALL ? t0 : 0;
    const int j_hi = MODE == GCM_SPATIAL_RADIUS_ALL ? n : r;
    uint64_t key = 0;
    if constexpr (MODE == GCM_SPATIAL_KNN) key = kth[(size_t)b * N + r];
    for (int j0 = j_lo; j0 < j_hi; j0 += 64) {
      const int j = j0 + lane;
      bool hit = false;
      if (j < j_hi) {
        const float d2 = row.d2(lds, npad, P, j);
        if constexpr (MODE == GCM_SPATIAL_KNN)
          hit = ((((uint64_t)__float_as_uint(d2)) << 32) | (uint32_t)j) <= key;
        else
          hit = within(d2, radius);
      }
      const uint64_t m = __ballot(hit);
      const int64_t e = base + lanes_below(m);
      if (hit && e < g1) {      // (the count pass evaluated the same predicate: e < g1 always holds)
        indices[e] = b;
        indices[E + e] = r;
        indices[2 * E + e] = j;
      }
      base += __popcll(m);
    }
  }
}

template <int MODE, int PC>
int launch_count(int M, dim3 grid, size_t lds, hipStream_t st, const float* nodes, const int64_t* T,
                 const int64_t* taus, const Cols& cols, int P, float radius, int k, int32_t* row_off,
                 uint64_t* kth, int64_t* edge_off, int N, int F, int npad) {
  const void* kern = nullptr;
  if constexpr (MODE != GCM_SPATIAL_KNN) {
    kern = (const void*)k_spatial_count<MODE, PC, 1>;
  } else {
    const int rc = gcm_pick(
        [&](auto mm) {
          kern = (const void*)k_spatial_count<MODE, PC, mm()>;
          return GCM_OK;
        },
        OneOf<1, 2, 4, 8, 16, 32, 64>{M});
    if (rc) return rc;
  }
  gcm_allow_dynamic_lds(kern, lds);
  void* args[] = {(void*)&nodes, (void*)&T, (void*)&taus, (void*)&cols, (void*)&P, (void*)&radius, (void*)&k,
                  (void*)&row_off, (void*)&kth, (void*)&edge_off, (void*)&N, (void*)&F, (void*)&npad};
  const hipError_t e = hipLaunchKernel(kern, grid, dim3(kThreads), args, lds, st);
  return e == hipSuccess ? GCM_OK : (int)e;
}

template <int MODE>
int dispatch_count(int PCsel, int M, dim3 grid, size_t lds, hipStream_t st, const float* nodes, const int64_t* T,
                   const int64_t* taus, const Cols& cols, int P, float radius, int k, int32_t* row_off,
                   uint64_t* kth, int64_t* edge_off, int N, int F, int npad) {
  if (PCsel == 2)
    return launch_count<MODE, 2>(M, grid, lds, st, nodes, T, taus, cols, P, radius, k, row_off, kth, edge_off, N,
                                 F, npad);
  if (PCsel == 3)
    return launch_count<MODE, 3>(M, grid, lds, st, nodes, T, taus, cols, P, radius, k, row_off, kth, edge_off, N,
                                 F, npad);
  return launch_count<MODE, 0>(M, grid, lds, st, nodes, T, taus, cols, P, radius, k, row_off, kth, edge_off, N, F,
                               npad);
}

template <int MODE>
const void* fill_kernel(int PCsel) {
  if (PCsel == 2) return (const void*)k_spatial_fill<MODE, 2>;
  if (PCsel == 3) return (const void*)k_spatial_fill<MODE, 3>;
  return (const void*)k_spatial_fill<MODE, 0>;
}

// shared argument checks; -> npad (LDS column stride), or a negative status
int spatial_check(const float* nodes, const int64_t* T, const int64_t* taus, const int32_t* cols_host, int P,
                  int mode, int k, int B, int N, int F, Cols& cols, size_t& lds_bytes, int& M) {
  if (!(nodes && T && taus && B > 0 && N > 0 && F > 0 && P >= 0 && (cols_host || P == 0))) return GCM_EINVAL;
  if (mode < GCM_SPATIAL_RADIUS_CAUSAL || mode > GCM_SPATIAL_KNN) return GCM_EINVAL;
  if (mode == GCM_SPATIAL_KNN && k < 1) return GCM_EINVAL;
  if (P > GCM_SPATIAL_MAX_COLS || N > 32768) return GCM_EUNSUPPORTED;
  cols = Cols{};
  for (int p = 0; p < P; ++p) {
    if (cols_host[p] < 0 || cols_host[p] >= F) return GCM_EINVAL;
    cols.c[p] = cols_host[p];
  }
  const int npad = (N + 63) / 64 * 64;
  lds_bytes = (size_t)(P + 1) * npad * sizeof(float);
  if (lds_bytes > GCM_SPATIAL_MAX_LDS) return GCM_EUNSUPPORTED;
  M = 1;
  if (mode == GCM_SPATIAL_KNN) {
    while (M * 64 < N) M *= 2;
    if (M > 64) return GCM_EUNSUPPORTED;
  }
  return npad;
}

}  // namespace

extern "C" int gcm_spatial_supported(int mode, int B, int N, int F, int P) {
  if (B <= 0 || N <= 0 || F <= 0 || P < 0 || mode < GCM_SPATIAL_RADIUS_CAUSAL || mode > GCM_SPATIAL_KNN)
    return 0;
  if (P > GCM_SPATIAL_MAX_COLS || N > 32768) return 0;
  const int npad = (N + 63) / 64 * 64;
  if ((size_t)(P + 1) * npad * sizeof(float) > GCM_SPATIAL_MAX_LDS) return 0;
  if (mode == GCM_SPATIAL_KNN && npad > 64 * 64) return 0;
  return 1;
}

extern "C" int gcm_spatial_count(const float* nodes, const int64_t* T, const int64_t* taus, const int32_t* cols_host,
                                 int P, int mode, float radius, int k, int32_t* row_off, uint64_t* kth,
                                 int64_t* edge_off, int B, int N, int F, gcm_stream_t stream) {
  Cols cols;
  size_t lds = 0;
  int M = 1;
  const int npad = spatial_check(nodes, T, taus, cols_host, P, mode, k, B, N, F, cols, lds, M);
  if (npad < 0) return npad;
  GCM_REQUIRE(row_off && edge_off && (kth || mode != GCM_SPATIAL_KNN));
  const int PCsel = (P == 2 || P == 3) ? P : 0;
  const hipStream_t st = (hipStream_t)stream;
  int rc;
  if (mode == GCM_SPATIAL_RADIUS_CAUSAL)
    rc = dispatch_count<GCM_SPATIAL_RADIUS_CAUSAL>(PCsel, M, dim3(B), lds, st, nodes, T, taus, cols, P, radius, k,
                                                    row_off, kth, edge_off, N, F, npad);
  else if (mode == GCM_SPATIAL_RADIUS_ALL)
    rc = dispatch_count<GCM_SPATIAL_RADIUS_ALL>(PCsel, M, dim3(B), lds, st, nodes, T, taus, cols, P, radius, k,
                                                 row_off, kth, edge_off, N, F, npad);
  else
    rc = dispatch_count<GCM_SPATIAL_KNN>(PCsel, M, dim3(B), lds, st, nodes, T, taus, cols, P, radius, k, row_off,
                                          kth, edge_off, N, F, npad);
  if (rc != GCM_OK) return rc;
  hipLaunchKernelGGL(k_spatial_offsets, dim3(1), dim3(256), 0, st, T, taus, edge_off, B);
  return gcm_launch_status();
}

extern "C" int gcm_spatial_fill(const float* nodes, const int64_t* T, const int64_t* taus, const int32_t* cols_host,
                                int P, int mode, float radius, const int32_t* row_off, const uint64_t* kth,
                                const int64_t* edge_off, int64_t* indices, int64_t E, int B, int N, int F,
                                gcm_stream_t stream) {
  Cols cols;
  size_t lds = 0;
  int M = 1;
  const int npad = spatial_check(nodes, T, taus, cols_host, P, mode, mode == GCM_SPATIAL_KNN ? 1 : 0, B, N, F, cols,
                                 lds, M);
  if (npad < 0) return npad;
  GCM_REQUIRE(row_off && edge_off && E >= 0 && (kth || mode != GCM_SPATIAL_KNN));
  if (E == 0) return GCM_OK;
  GCM_REQUIRE(indices);
  lds = (size_t)P * npad * sizeof(float);
  const int PCsel = (P == 2 || P == 3) ? P : 0;
  const void* kern = mode == GCM_SPATIAL_RADIUS_CAUSAL ? fill_kernel<GCM_SPATIAL_RADIUS_CAUSAL>(PCsel)
                     : mode == GCM_SPATIAL_RADIUS_ALL  ? fill_kernel<GCM_SPATIAL_RADIUS_ALL>(PCsel)
                                                       : fill_kernel<GCM_SPATIAL_KNN>(PCsel);
  gcm_allow_dynamic_lds(kern, lds);
  void* args[] = {(void*)&nodes, (void*)&T, (void*)&taus, (void*)&cols, (void*)&P, (void*)&radius,
                  (void*)&row_off, (void*)&kth, (void*)&edge_off, (void*)&indices, (void*)&E, (void*)&N,
                  (void*)&F, (void*)&npad};
  const hipError_t e = hipLaunchKernel(kern, dim3(B), dim3(kThreads), args, lds, (hipStream_t)stream);
  return e == hipSuccess ? GCM_OK : (int)e;
}
