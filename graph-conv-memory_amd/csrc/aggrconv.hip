// Mean and max neighbourhood aggregation for GraphConv / DenseGraphConv (aggr="mean" | "max") and the SAGE
// layers on top of them, forward and backward on gfx950.
//
//   out = agg W_rel^T + x W_root^T + bias          (w_root, bias optional)
//   dense mean:  agg_i  = (sum_j adj_ij x_j) / max(sum_j adj_ij, 1)
//   dense max:   agg_ic = max over {j : adj_ij != 0} of x_jc          (0 for an empty row; ties: lowest j)
//   CSR mean:    agg_i  = (sum_{e -> i} w_e x_src(e)) / #{e -> i}     (0 without in-edges)
//   CSR max:     agg_ic = max over e -> i of w_e x_src(e),c           (0 without in-edges; ties: first CSR entry)
//
// The contractions run on v_mfma_f32_32x32x2_f32: the dense mean aggregation, its transpose and its adjacency
// gradient through gcn_mm.h's tile kernel (row-scale / row-add epilogues), the two linears of every leg in
// k_aggr_lin2, that kernel with two K segments into one accumulator.  The max legs are compare-select passes
// that keep the winning neighbour (dense: j as int16; CSR: the entry as int32) for the backward, which is a
// gather in a fixed order.  No atomics: every sum has one order.  Fi, Fo <= 128.
#include "gcn_mm.h"

namespace {

// ---------------------------------------------------------------------------
// C = A0 B0 + A1 B1 + bias: row-major A (lda = K of the segment), strided B, row-major C.  Segment 1 optional.
// ---------------------------------------------------------------------------
struct Lin2Args {
  const float* A[2];
  const float* B[2];
  int64_t b_ks[2], b_js[2];
  int K[2];
  int nseg;
  const float* bias;
  float* C;
  int M, N;
};

template <int NCT>
__global__ __launch_bounds__(256) void k_aggr_lin2(Lin2Args p) {
  __shared__ float sA[MB * (KT + 1)];        // [i][k]
  __shared__ float sB[KT * (32 * NCT + 1)];  // [k][j]
  const int i0 = blockIdx.x * MB;
  const TileLane t = tile_lane();
  f32x16 acc[NCT];
  tile_zero(acc);
  for (int seg = 0; seg < p.nseg; ++seg) {
    const float* A = p.A[seg];
    const float* B = p.B[seg];
    const int K = p.K[seg];
    const int64_t bks = p.b_ks[seg], bjs = p.b_js[seg];
    tile_mma<NCT, false>(
        acc, t, sA, sB, i0, 0, p.M, p.N, 0, K, false, bks == 1,
        [=](int gi, int gk) { return A[(size_t)gi * K + gk]; },
        [=](int gk, int gj) { return B[(size_t)gk * bks + (size_t)gj * bjs]; });
  }
  tile_store(acc, t, i0, 0, p.M, p.N, [=](int j) {
    const float bias = p.bias ? p.bias[j] : 0.f;
    return [=](int i, float v) { p.C[(size_t)i * p.N + j] = v + bias; };
  });
}

int launch_lin2(const Lin2Args& p, hipStream_t s) {  // N <= 128
  const dim3 grid(blocks(p.M, MB));
  dispatch_nct(nct_of(p.N), [&](auto n) { hipLaunchKernelGGL(k_aggr_lin2<n()>, grid, dim3(256), 0, s, p); });
  return gcm_launch_status();
}

// out = agg W_rel^T + x W_root^T + bias over R rows
int linear_fwd(const float* agg, const float* x, const float* w_rel, const float* w_root, const float* bias,
               float* out, int64_t R, int Fi, int Fo, hipStream_t s) {
  Lin2Args p = {};
  p.A[0] = agg, p.B[0] = w_rel, p.b_ks[0] = 1, p.b_js[0] = Fi, p.K[0] = Fi;
  p.A[1] = x, p.B[1] = w_root, p.b_ks[1] = 1, p.b_js[1] = Fi, p.K[1] = Fi;
  p.nseg = w_root ? 2 : 1;
  p.bias = bias, p.C = out, p.M = (int)R, p.N = Fo;
  return launch_lin2(p, s);
}

// the parameter gradients every leg shares: g_bias = colsum(G), g_w_rel = G^T agg, g_w_root = G^T x
int param_grads(const float* g_out, const float* agg, const float* x, float* g_w_rel, float* g_w_root,
                float* g_bias, float* slabs, int64_t R, int Fi, int Fo, hipStream_t s) {
  int rc;
  if (g_bias && (rc = colsum(g_out, R, Fo, g_bias, slabs, s))) return rc;
  if (g_w_rel && (rc = wgrad(g_out, agg, g_w_rel, slabs, R, Fi, Fo, s))) return rc;
  if (g_w_root && (rc = wgrad(g_out, x, g_w_root, slabs, R, Fi, Fo, s))) return rc;
  return GCM_OK;
}

size_t slab_floats(int64_t R, int Fi, int Fo) {
  int nsplit, kchunk;
  wgrad_split(R, &nsplit, &kchunk);
  return std::max<size_t>((size_t)nsplit * Fo * Fi, (size_t)colsum_slabs(R) * Fo);
}

// ---------------------------------------------------------------------------
// dense mean
// ---------------------------------------------------------------------------
// deg = rowsum(adj) (before the clamp), dinv = 1 / max(deg, 1); one wave per row
__global__ __launch_bounds__(256) void k_aggr_dense_deg(const float* __restrict__ adj, float* __restrict__ deg,
                                                        float* __restrict__ dinv, int64_t rows, int N) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* a = adj + (size_t)row * N;
  float s = 0.f;
  for (int j = lane; j < N; j += 64) s += a[j];
  s = gcm_wave_sum(s);
  if (lane == 0) {
    deg[row] = s;
    dinv[row] = 1.f / fmaxf(s, 1.f);
  }
}

// the degree term of g_adj: c_i = -dinv_i <dAgg_i, agg_i> where rowsum >= 1 (clamp(min=1) passes the gradient at
// the bound), else 0; one wave per row
__global__ __launch_bounds__(256) void k_aggr_dense_rowterm(const float* __restrict__ dagg,
                                                            const float* __restrict__ agg,
                                                            const float* __restrict__ deg,
                                                            const float* __restrict__ dinv, float* __restrict__ c,
                                                            int64_t rows, int Fi) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const size_t o = (size_t)row * Fi;
  float s = 0.f;
  for (int f = lane; f < Fi; f += 64) s = fmaf(dagg[o + f], agg[o + f], s);
  s = gcm_wave_sum(s);
  if (lane == 0) c[row] = deg[row] >= 1.f ? -dinv[row] * s : 0.f;
}

// ---------------------------------------------------------------------------
// dense max
// ---------------------------------------------------------------------------
constexpr int XR = 32;  // rows i per workgroup
constexpr int XJ = 64;  // neighbours j per tile: one 64-bit pattern word per row

// One workgroup per (graph, 32 rows).  Per tile of 64 neighbours: every row's adjacency entries are read once,
// coalesced, and reduced to a pattern word by ballot; the x tile sits in LDS; a thread owns (row, channel) pairs and
// walks the set bits in ascending j with a strict compare, so the lowest j wins a tie.
template <int NCT>
__global__ __launch_bounds__(256) void k_aggr_dense_max_fwd(const float* __restrict__ x,
                                                            const float* __restrict__ adj, float* __restrict__ agg,
                                                            int16_t* __restrict__ winner, int N, int Fi) {
  constexpr int FiP = 32 * NCT, PAIRS = XR * FiP / 256;
  __shared__ float sX[XJ * FiP];
  __shared__ unsigned long long sBits[XR];
  const int b = blockIdx.y, i0 = blockIdx.x * XR;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float* xb = x + (size_t)b * N * Fi;
  const float* ab = adj + (size_t)b * N * N;
  float best[PAIRS];
  int arg[PAIRS];
#pragma unroll
  for (int q = 0; q < PAIRS; ++q) best[q] = 0.f, arg[q] = -1;

  for (int j0 = 0; j0 < N; j0 += XJ) {
    for (int r = wave; r < XR; r += 4) {
      const int i = i0 + r, j = j0 + lane;
      const float a = (i < N && j < N) ? ab[(size_t)i * N + j] : 0.f;
      const unsigned long long word = __ballot(a != 0.f);
      if (lane == 0) sBits[r] = word;
    }
    for (int e = threadIdx.x; e < XJ * FiP; e += 256) {
      const int jj = e / FiP, c = e - jj * FiP;
      sX[e] = (j0 + jj < N && c < Fi) ? xb[(size_t)(j0 + jj) * Fi + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) {
      const int idx = threadIdx.x + 256 * q;
      const int r = idx / FiP, c = idx - r * FiP;
      unsigned long long word = sBits[r];
      while (word) {
        const int jj = __builtin_ctzll(word);
        word &= word - 1;
        const float v = sX[jj * FiP + c];
        if (arg[q] < 0 || v > best[q]) best[q] = v, arg[q] = j0 + jj;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < PAIRS; ++q) {
    const int idx = threadIdx.x + 256 * q;
    const int r = idx / FiP, c = idx - r * FiP;
    if (i0 + r < N && c < Fi) {
      const size_t o = ((size_t)b * N + i0 + r) * Fi + c;
      agg[o] = best[q];
      winner[o] = (int16_t)arg[q];
    }
  }
}

// g_x[b,j,c] (+)= sum over the rows i whose winner in channel c is j of dAgg[b,i,c], in ascending i.  One
// workgroup per (graph, 32 neighbours j); winner and dAgg tiles of 32 rows i go through LDS.  (winner == j
// implies the pattern bit (i, j), so the pattern is not read again.)
template <int NCT>
__global__ __launch_bounds__(256) void k_aggr_dense_max_bwd(const float* __restrict__ dagg,
                                                            const int16_t* __restrict__ winner,
                                                            float* __restrict__ g_x, int N, int Fi, int accumulate) {
  constexpr int FiP = 32 * NCT, PAIRS = XR * FiP / 256;
  __shared__ float sG[XR * FiP];
  __shared__ int16_t sW[XR * FiP];
  const int b = blockIdx.y, j0 = blockIdx.x * XR;
  const size_t base = (size_t)b * N * Fi;
  float acc[PAIRS];
#pragma unroll
  for (int q = 0; q < PAIRS; ++q) acc[q] = 0.f;
  for (int i0 = 0; i0 < N; i0 += XR) {
    for (int e = threadIdx.x; e < XR * FiP; e += 256) {
      const int r = e / FiP, c = e - r * FiP;
      const bool in = i0 + r < N && c < Fi;
      const size_t o = base + (size_t)(i0 + r) * Fi + c;
      sG[e] = in ? dagg[o] : 0.f;
      sW[e] = in ? winner[o] : (int16_t)-1;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) {
      const int idx = threadIdx.x + 256 * q;
      const int c = idx % FiP;
      const int j = j0 + idx / FiP;
      for (int r = 0; r < XR; ++r)
        if (sW[r * FiP + c] == j) acc[q] += sG[r * FiP + c];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < PAIRS; ++q) {
    const int idx = threadIdx.x + 256 * q;
    const int c = idx % FiP, j = j0 + idx / FiP;
    if (j < N && c < Fi) {
      const size_t o = base + (size_t)j * Fi + c;
      g_x[o] = accumulate ? g_x[o] + acc[q] : acc[q];
    }
  }
}

// ---------------------------------------------------------------------------
// CSR legs: one thread per (node, channel)
// ---------------------------------------------------------------------------
template <bool MAX>
__global__ void k_aggr_csr_fwd(const float* __restrict__ x, const int64_t* __restrict__ row_ptr,
                               const int64_t* __restrict__ col, const float* __restrict__ w,
                               float* __restrict__ agg, int32_t* __restrict__ winner, int64_t M, int Fi) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * Fi) return;
  const int64_t i = t / Fi;
  const int f = (int)(t - i * Fi);
  const int64_t e0 = row_ptr[i], e1 = row_ptr[i + 1];
  float a = 0.f;
  int64_t arg = -1;
  for (int64_t e = e0; e < e1; ++e) {
    const float xv = x[(size_t)col[e] * Fi + f];
    if (MAX) {
      const float v = w ? w[e] * xv : xv;
      if (arg < 0 || v > a) a = v, arg = e;
    } else {
      a = w ? fmaf(w[e], xv, a) : a + xv;
    }
  }
  if (MAX) winner[t] = (int32_t)arg;
  else if (e1 > e0) a /= (float)(e1 - e0);
  agg[t] = a;
}

// g_x[j,f] (+)= sum over the CSC column j, in its order, of the edge's share of dAgg[dst,f]:
// mean w_e / count(dst); max w_e where the edge won (dst, f)
template <bool MAX>
__global__ void k_aggr_csr_bwd_x(const float* __restrict__ dagg, const int64_t* __restrict__ row_ptr,
                                 const int64_t* __restrict__ col_ptr, const int64_t* __restrict__ rows,
                                 const int64_t* __restrict__ perm, const float* __restrict__ w,
                                 const int32_t* __restrict__ winner, float* __restrict__ g_x, int64_t M, int Fi,
                                 int accumulate) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * Fi) return;
  const int64_t j = t / Fi;
  const int f = (int)(t - j * Fi);
  float a = 0.f;
  if (col_ptr)
    for (int64_t k = col_ptr[j]; k < col_ptr[j + 1]; ++k) {
      const int64_t d = rows[k], e = perm[k];
      const float we = w ? w[e] : 1.f;
      const float g = dagg[(size_t)d * Fi + f];
      if (MAX) {
        if (winner[(size_t)d * Fi + f] == (int32_t)e) a = fmaf(we, g, a);
      } else {
        a += we * g / (float)(row_ptr[d + 1] - row_ptr[d]);
      }
    }
  g_x[t] = accumulate ? g_x[t] + a : a;
}

// g_w[e] = <x_src, dAgg_dst> / count(dst) (mean), or over the channels the edge won (max); one thread per CSR entry
template <bool MAX>
__global__ void k_aggr_csr_bwd_w(const float* __restrict__ x, const float* __restrict__ dagg,
                                 const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col,
                                 const int64_t* __restrict__ dst, const int32_t* __restrict__ winner,
                                 float* __restrict__ g_w, int64_t E, int Fi) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const int64_t s = col[e], d = dst[e];
  const float* xs = x + (size_t)s * Fi;
  const float* gd = dagg + (size_t)d * Fi;
  float a = 0.f;
  for (int f = 0; f < Fi; ++f)
    if (!MAX || winner[(size_t)d * Fi + f] == (int32_t)e) a = fmaf(xs[f], gd[f], a);
  g_w[e] = MAX ? a : a / (float)(row_ptr[d + 1] - row_ptr[d]);
}

bool aggr_ok(int aggr) { return aggr == GCM_AGGR_MEAN || aggr == GCM_AGGR_MAX; }

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: dense
// ---------------------------------------------------------------------------
extern "C" int gcm_dense_aggrconv_fwd(const float* x, const float* adj, const float* w_rel, const float* w_root,
                                      const float* bias, float* out, float* agg, float* deg, float* dinv,
                                      int16_t* winner, int B, int N, int Fi, int Fo, int aggr,
                                      gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && w_rel && out && agg && aggr_ok(aggr));
  GCM_REQUIRE(aggr == GCM_AGGR_MEAN ? (deg && dinv) : winner != nullptr);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && Fo > 0);
  if (Fi > 128 || Fo > 128 || B > 65535 || N > 32767 || (int64_t)B * N > (1 << 30)) return GCM_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * N;
  int rc;
  if (aggr == GCM_AGGR_MEAN) {
    hipLaunchKernelGGL(k_aggr_dense_deg, dim3(blocks(rows, 4)), dim3(256), 0, s, adj, deg, dinv, rows, N);
    if ((rc = gcm_launch_status())) return rc;
    MmArgs p = mm_args();  // agg = dinv_i sum_k adj_ik x_k
    p.A = adj, p.a_bs = (int64_t)N * N, p.a_is = N, p.a_ks = 1;
    p.B = x, p.b_bs = (int64_t)N * Fi, p.b_ks = Fi, p.b_js = 1;
    p.C = agg, p.c_bs = (int64_t)N * Fi, p.c_is = Fi, p.c_js = 1;
    p.c_rscale = dinv, p.s_bs = N;
    p.M = N, p.N = Fi, p.K = N, p.batch = B;
    if ((rc = launch_mm(p, 1, s))) return rc;
  } else {
    const dim3 grid(blocks(N, XR), B);
    dispatch_nct((Fi + 31) / 32, [&](auto n) {
      hipLaunchKernelGGL(k_aggr_dense_max_fwd<n()>, grid, dim3(256), 0, s, x, adj, agg, winner, N, Fi);
    });
    if ((rc = gcm_launch_status())) return rc;
  }
  return linear_fwd(agg, x, w_rel, w_root, bias, out, rows, Fi, Fo, s);
}

namespace {
struct DenseWs {
  size_t t, c, slabs, total;  // t: [rows, max(Fi, Fo)] (mean: A^T (dinv G), then dAgg; max: dAgg)
};
DenseWs dense_ws(int B, int N, int Fi, int Fo) {
  DenseWs w;
  const int64_t rows = (int64_t)B * N;
  Carve cv;
  w.t = cv.take(rows * std::max(Fi, Fo) * sizeof(float));
  w.c = cv.take(rows * sizeof(float));
  w.slabs = cv.at;  // the last field: not rounded up
  w.total = w.slabs + slab_floats(rows, Fi, Fo) * sizeof(float);
  return w;
}
}  // namespace

extern "C" size_t gcm_dense_aggrconv_bwd_workspace_bytes(int B, int N, int Fi, int Fo) {
  if (B <= 0 || N <= 0 || Fi <= 0 || Fo <= 0) return 0;
  return dense_ws(B, N, Fi, Fo).total;
}

extern "C" int gcm_dense_aggrconv_bwd(const float* g_out, const float* x, const float* adj, const float* w_rel,
                                      const float* w_root, const float* agg, const float* deg, const float* dinv,
                                      const int16_t* winner, float* g_x, float* g_adj, float* g_w_rel,
                                      float* g_w_root, float* g_bias, void* workspace, size_t workspace_bytes,
                                      int B, int N, int Fi, int Fo, int aggr, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && adj && w_rel && agg && workspace && aggr_ok(aggr));
  GCM_REQUIRE(aggr == GCM_AGGR_MEAN ? (deg && dinv) : (winner && !g_adj));
  GCM_REQUIRE(w_root || !g_w_root);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && Fo > 0);
  if (Fi > 128 || Fo > 128 || B > 65535 || N > 32767 || (int64_t)B * N > (1 << 30)) return GCM_EUNSUPPORTED;
  const DenseWs L = dense_ws(B, N, Fi, Fo);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* t = (float*)(ws + L.t);
  float* c = (float*)(ws + L.c);
  float* slabs = (float*)(ws + L.slabs);
  const int64_t rows = (int64_t)B * N;
  int rc;
  if ((rc = param_grads(g_out, agg, x, g_w_rel, g_w_root, g_bias, slabs, rows, Fi, Fo, s))) return rc;
  if (aggr == GCM_AGGR_MEAN) {
    if (g_x) {  // g_x = (A^T (dinv G)) W_rel + G W_root
      MmArgs p = mm_args();
      p.A = adj, p.a_bs = (int64_t)N * N, p.a_is = 1, p.a_ks = N;
      p.B = g_out, p.b_bs = (int64_t)N * Fo, p.b_ks = Fo, p.b_js = 1, p.b_kscale = dinv, p.s_bs = N;
      p.C = t, p.c_bs = (int64_t)N * Fo, p.c_is = Fo, p.c_js = 1;
      p.M = N, p.N = Fo, p.K = N, p.batch = B;
      if ((rc = launch_mm(p, 1, s))) return rc;
      Lin2Args q = {};
      q.A[0] = t, q.B[0] = w_rel, q.b_ks[0] = Fi, q.b_js[0] = 1, q.K[0] = Fo;
      q.A[1] = g_out, q.B[1] = w_root, q.b_ks[1] = Fi, q.b_js[1] = 1, q.K[1] = Fo;
      q.nseg = w_root ? 2 : 1;
      q.C = g_x, q.M = (int)rows, q.N = Fi;
      if ((rc = launch_lin2(q, s))) return rc;
    }
    if (g_adj) {  // g_adj_ij = dinv_i <dAgg_i, x_j> + c_i
      if ((rc = mm_gw(g_out, w_rel, t, rows, Fi, Fo, s))) return rc;
      hipLaunchKernelGGL(k_aggr_dense_rowterm, dim3(blocks(rows, 4)), dim3(256), 0, s, t, agg, deg, dinv, c, rows,
                         Fi);
      if ((rc = gcm_launch_status())) return rc;
      MmArgs p = mm_args();
      p.A = t, p.a_bs = (int64_t)N * Fi, p.a_is = Fi, p.a_ks = 1;
      p.B = x, p.b_bs = (int64_t)N * Fi, p.b_ks = 1, p.b_js = Fi;
      p.C = g_adj, p.c_bs = (int64_t)N * N, p.c_is = N, p.c_js = 1;
      p.c_rscale = dinv, p.c_radd = c, p.s_bs = N;
      p.M = N, p.N = N, p.K = Fi, p.batch = B;
      if ((rc = launch_mm(p, 1, s))) return rc;
    }
    return GCM_OK;
  }
  if (!g_x) return GCM_OK;
  if ((rc = mm_gw(g_out, w_rel, t, rows, Fi, Fo, s))) return rc;                    // dAgg
  if (w_root && (rc = mm_gw(g_out, w_root, g_x, rows, Fi, Fo, s))) return rc;       // the root term
  const dim3 grid(blocks(N, XR), B);
  const int accumulate = w_root != nullptr;
  dispatch_nct((Fi + 31) / 32, [&](auto n) {
    hipLaunchKernelGGL(k_aggr_dense_max_bwd<n()>, grid, dim3(256), 0, s, t, winner, g_x, N, Fi, accumulate);
  });
  return gcm_launch_status();
}

// ---------------------------------------------------------------------------
// C ABI: CSR
// ---------------------------------------------------------------------------
extern "C" int gcm_csr_aggrconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* w_edge,
                                    const float* w_rel, const float* w_root, const float* bias, float* out,
                                    float* agg, int32_t* winner, int64_t M, int64_t E, int Fi, int Fo, int aggr,
                                    gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && w_rel && out && agg && aggr_ok(aggr));
  GCM_REQUIRE(aggr == GCM_AGGR_MEAN || winner);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && Fo > 0);
  GCM_REQUIRE(E == 0 || col);
  if (Fi > 128 || Fo > 128 || M > (1 << 30) || E > INT32_MAX) return GCM_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(blocks(M * Fi, 256));
  if (aggr == GCM_AGGR_MAX)
    hipLaunchKernelGGL(k_aggr_csr_fwd<true>, grid, dim3(256), 0, s, x, row_ptr, col, w_edge, agg, winner, M, Fi);
  else
    hipLaunchKernelGGL(k_aggr_csr_fwd<false>, grid, dim3(256), 0, s, x, row_ptr, col, w_edge, agg, winner, M, Fi);
  const int rc = gcm_launch_status();
  return rc ? rc : linear_fwd(agg, x, w_rel, w_root, bias, out, M, Fi, Fo, s);
}

namespace {
struct CsrWs {
  size_t dagg, slabs, total;
};
CsrWs csr_ws(int64_t M, int Fi, int Fo) {
  CsrWs w;
  Carve cv;
  w.dagg = cv.take(M * Fi * sizeof(float));
  w.slabs = cv.at;  // the last field: not rounded up
  w.total = w.slabs + slab_floats(M, Fi, Fo) * sizeof(float);
  return w;
}
}  // namespace

extern "C" size_t gcm_csr_aggrconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int Fo) {
  if (M <= 0 || E < 0 || Fi <= 0 || Fo <= 0) return 0;
  return csr_ws(M, Fi, Fo).total;
}

extern "C" int gcm_csr_aggrconv_bwd(const float* g_out, const float* x, const float* agg, const int64_t* row_ptr,
                                    const int64_t* col, const int64_t* dst, const int64_t* col_ptr,
                                    const int64_t* rows, const int64_t* perm, const float* w_edge,
                                    const int32_t* winner, const float* w_rel, const float* w_root, float* g_x,
                                    float* g_edge, float* g_w_rel, float* g_w_root, float* g_bias, void* workspace,
                                    size_t workspace_bytes, int64_t M, int64_t E, int Fi, int Fo, int aggr,
                                    gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && agg && row_ptr && w_rel && workspace && aggr_ok(aggr));
  GCM_REQUIRE(aggr == GCM_AGGR_MEAN || winner);
  GCM_REQUIRE(w_root || !g_w_root);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && Fo > 0);
  GCM_REQUIRE(E == 0 || (col && dst && col_ptr && rows && perm) || (!g_x && !g_edge));
  if (Fi > 128 || Fo > 128 || M > (1 << 30) || E > INT32_MAX) return GCM_EUNSUPPORTED;
  const CsrWs L = csr_ws(M, Fi, Fo);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* dagg = (float*)(ws + L.dagg);
  float* slabs = (float*)(ws + L.slabs);
  int rc;
  if ((rc = param_grads(g_out, agg, x, g_w_rel, g_w_root, g_bias, slabs, M, Fi, Fo, s))) return rc;
  const bool has_e = E > 0;
  if (!g_x && !(g_edge && has_e)) return GCM_OK;
  if ((rc = mm_gw(g_out, w_rel, dagg, M, Fi, Fo, s))) return rc;
  if (g_x) {
    if (w_root && (rc = mm_gw(g_out, w_root, g_x, M, Fi, Fo, s))) return rc;
    const dim3 grid(blocks(M * Fi, 256));
    const int accumulate = w_root != nullptr;
    if (aggr == GCM_AGGR_MAX)
      hipLaunchKernelGGL(k_aggr_csr_bwd_x<true>, grid, dim3(256), 0, s, dagg, row_ptr, has_e ? col_ptr : nullptr,
                         rows, perm, w_edge, winner, g_x, M, Fi, accumulate);
    else
      hipLaunchKernelGGL(k_aggr_csr_bwd_x<false>, grid, dim3(256), 0, s, dagg, row_ptr, has_e ? col_ptr : nullptr,
                         rows, perm, w_edge, winner, g_x, M, Fi, accumulate);
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_edge && has_e) {
    const dim3 grid(blocks(E, 256));
    if (aggr == GCM_AGGR_MAX)
      hipLaunchKernelGGL(k_aggr_csr_bwd_w<true>, grid, dim3(256), 0, s, x, dagg, row_ptr, col, dst, winner, g_edge,
                         E, Fi);
    else
      hipLaunchKernelGGL(k_aggr_csr_bwd_w<false>, grid, dim3(256), 0, s, x, dagg, row_ptr, col, dst, winner, g_edge,
                         E, Fi);
    if ((rc = gcm_launch_status())) return rc;
  }
  return GCM_OK;
}
