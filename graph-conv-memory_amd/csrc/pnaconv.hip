// PNAConv / DensePNAConv (Principal Neighbourhood Aggregation, Corso et al. 2020), forward and backward on gfx950.
//
// The message of PNA is linear in its two halves: m_e = W_pre [x_i | x_src(e)] + b_pre = a_i + b_src(e) with
// a = x W_dst^T + b_pre and b = x W_src^T, so nothing of size E x F exists.  Every aggregator is a statistic of b over
// the neighbourhood: sum = n a + sum(b); mean, min, max = a + stat(b); var, std = stat(b).  One pass per destination
// row reads the pattern (or the CSR row) once and keeps per channel the count, the sum and the sum of squares about
// the first neighbour's value (an all-equal neighbourhood has variance exactly 0), min and max with their winners;
// its epilogue applies a, the n = 0 rule and the degree scalers and writes the operand of the post linear,
// cat = [x_t | scaled blocks].  Only the statistics the layer lists are computed.
//
// Backward: the scalers are folded into one gradient per aggregator and row (k_pna_fold, which also gives the
// gradient of a), then one pass per source over its sinks - ascending i (dense), CSC order (sparse) - gathers the
// gradient of b.  The linears' input gradients run on gcn_mm.h's tile step (k_pna_mm).  The forward linears, the per-row
// statistics, their gradients, and the weight and bias gradients (split-K slabs summed in fixed order) are accumulated in fp64 and
// rounded once.  No atomics: every sum has one order.  in_channels, out_channels <= 128.
#include "gcn_mm.h"

namespace {

struct PnaCfg {
  int A, S;
  int aggr[8], scal[8];
  int need_mm, need_var;  // min / max listed; var / std listed
};

bool pna_cfg(int aggrs, int A, int scalers, int S, PnaCfg* c) {
  if (A < 1 || A > 8 || S < 1 || S > 8) return false;
  c->A = A, c->S = S, c->need_mm = c->need_var = 0;
  for (int a = 0; a < A; ++a) {
    const int k = (aggrs >> (3 * a)) & 7;
    if (k > GCM_PNA_STD) return false;
    c->aggr[a] = k;
    if (k == GCM_PNA_MIN || k == GCM_PNA_MAX) c->need_mm = 1;
    if (k == GCM_PNA_VAR || k == GCM_PNA_STD) c->need_var = 1;
  }
  for (int s = 0; s < S; ++s) {
    const int k = (scalers >> (3 * s)) & 7;
    if (k > GCM_PNA_INVERSE_LINEAR) return false;
    c->scal[s] = k;
  }
  return true;
}

// the sizes every leg shares
struct PnaDims {
  int64_t R;      // rows: B N or M
  int in, out, T, Fi, Fo, C, K1, divide;
};

bool pna_dims(int64_t R, int in, int out, int T, int divide, int A, int S, PnaDims* d) {
  if (R <= 0 || in <= 0 || out <= 0 || T <= 0 || out % T || (divide && in % T)) return false;
  d->R = R, d->in = in, d->out = out, d->T = T, d->divide = divide;
  d->Fi = divide ? in / T : in;
  d->Fo = out / T;
  d->C = T * d->Fi;
  d->K1 = (1 + A * S) * d->Fi;
  return true;
}

__device__ __forceinline__ double pna_scaler(int kind, int n, double avg_lin, double avg_log) {
  switch (kind) {
    case GCM_PNA_AMPLIFICATION: return log((double)n + 1.0) / avg_log;
    case GCM_PNA_ATTENUATION: return avg_log / log((double)max(n, 1) + 1.0);
    case GCM_PNA_LINEAR: return (double)n / avg_lin;
    case GCM_PNA_INVERSE_LINEAR: return avg_lin / (double)max(n, 1);
    default: return 1.0;
  }
}

// what one (row, channel) accumulates over its neighbourhood
struct PnaAcc {
  int n, amn, amx;
  float shift, mn, mx;
  double sd, sd2;  // fp64: the sums are rounded once, in the epilogue
  __device__ __forceinline__ void init() { n = 0, amn = amx = -1, shift = mn = mx = 0.f, sd = sd2 = 0.0; }
  __device__ __forceinline__ void add(float v, int who, const PnaCfg& cfg) {
    if (n == 0) {
      shift = mn = mx = v, amn = amx = who;
    } else {
      if (cfg.need_mm) {
        if (v < mn) mn = v, amn = who;
        if (v > mx) mx = v, amx = who;
      }
      const double d = (double)v - (double)shift;
      sd += d;
      if (cfg.need_var) sd2 = fma(d, d, sd2);
    }
    ++n;
  }
};

// the epilogue of one (row, channel): the aggregators from the statistics of b and a, the n = 0 rule, the scalers;
// writes the tower's cat row (x and the A S blocks) and what the backward reads again.  so: the offset (row, c) of the
// [R, 2, C] arrays; their second plane is at so + C.
template <typename W>
__device__ __forceinline__ void pna_emit(const PnaCfg& cfg, const PnaAcc& s, float a, float xv, const float* avg,
                                         float* cat_row, int f, int Fi, float* stat, W* winner, size_t so, int C) {
  cat_row[f] = xv;
  // in fp64, rounded once when stored: the fp32 of the aggregators' inputs is all the error there is
  double val[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double mean_b = 0.0;
  float stdv = 0.f;
  if (s.n > 0) {
    const double n = (double)s.n, mean_d = s.sd / n;
    mean_b = (double)s.shift + mean_d;
    val[GCM_PNA_SUM] = n * ((double)a + (double)s.shift) + s.sd;
    val[GCM_PNA_MEAN] = (double)a + mean_b;
    val[GCM_PNA_MIN] = (double)a + (double)s.mn;
    val[GCM_PNA_MAX] = (double)a + (double)s.mx;
    if (cfg.need_var) {
      const double var = (s.sd2 - s.sd * mean_d) / n;
      stdv = (float)sqrt(fmax(var, 1e-5));
      if (stdv <= sqrtf(1e-5f)) stdv = 0.f;
      val[GCM_PNA_VAR] = var;
      val[GCM_PNA_STD] = (double)stdv;
    }
  }
  const double avg_lin = (double)avg[0], avg_log = (double)avg[1];
  for (int q = 0; q < cfg.S; ++q) {
    const double sc = s.n > 0 ? pna_scaler(cfg.scal[q], s.n, avg_lin, avg_log) : 0.0;
    for (int k = 0; k < cfg.A; ++k) cat_row[(size_t)Fi * (1 + q * cfg.A + k) + f] = (float)(sc * val[cfg.aggr[k]]);
  }
  if (cfg.need_var) stat[so] = (float)mean_b, stat[so + C] = stdv;
  if (cfg.need_mm) winner[so] = (W)s.amn, winner[so + C] = (W)s.amx;
}

// ---------------------------------------------------------------------------
// dense forward: one workgroup per (graph, 32 rows, CP channels); the pattern ballot walk of k_aggr_dense_max_fwd
// ---------------------------------------------------------------------------
constexpr int PR = 32;  // rows i per workgroup
constexpr int PJ = 64;  // neighbours j per tile: one 64-bit pattern word per row

template <int NCT>
__global__ __launch_bounds__(256) void k_pna_dense_fwd(PnaCfg cfg, const float* __restrict__ x,
                                                       const float* __restrict__ adj, const float* __restrict__ ab,
                                                       const float* __restrict__ avg, float* __restrict__ cat,
                                                       int32_t* __restrict__ cnt, float* __restrict__ stat,
                                                       int16_t* __restrict__ winner, int N, int in, int T, int Fi,
                                                       int divide, int add_loop) {
  constexpr int CP = 32 * NCT, PAIRS = PR * CP / 256;
  __shared__ float sB[PJ * CP];
  __shared__ unsigned long long sBits[PR];
  const int b = blockIdx.y, i0 = blockIdx.x * PR, c0 = blockIdx.z * CP;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int C = T * Fi, K1 = (1 + cfg.A * cfg.S) * Fi;
  const float* ab_b = ab + (size_t)b * N * C * 2;
  const float* adj_b = adj + (size_t)b * N * N;
  PnaAcc acc[PAIRS];
#pragma unroll
  for (int q = 0; q < PAIRS; ++q) acc[q].init();

  for (int j0 = 0; j0 < N; j0 += PJ) {
    for (int r = wave; r < PR; r += 4) {
      const int i = i0 + r, j = j0 + lane;
      const bool set = i < N && j < N && (adj_b[(size_t)i * N + j] != 0.f || (add_loop && i == j));
      const unsigned long long word = __ballot(set);
      if (lane == 0) sBits[r] = word;
    }
    for (int e = threadIdx.x; e < PJ * CP; e += 256) {
      const int jj = e / CP, c = c0 + e % CP;
      float v = 0.f;
      if (j0 + jj < N && c < C) {
        const int t = c / Fi, f = c - t * Fi;
        v = ab_b[((size_t)(j0 + jj) * T + t) * 2 * Fi + Fi + f];
      }
      sB[e] = v;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) {
      const int idx = threadIdx.x + 256 * q;
      const int r = idx / CP, cc = idx - r * CP;
      unsigned long long word = sBits[r];
      while (word) {
        const int jj = __builtin_ctzll(word);
        word &= word - 1;
        acc[q].add(sB[jj * CP + cc], j0 + jj, cfg);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < PAIRS; ++q) {
    const int idx = threadIdx.x + 256 * q;
    const int r = idx / CP, c = c0 + idx % CP;
    if (i0 + r >= N || c >= C) continue;
    const size_t row = (size_t)b * N + i0 + r;
    const int t = c / Fi, f = c - t * Fi;
    const float a = ab[(row * T + t) * 2 * Fi + f];
    const float xv = x[row * in + (divide ? t * Fi : 0) + f];
    pna_emit<int16_t>(cfg, acc[q], a, xv, avg, cat + (row * T + t) * K1, f, Fi, stat, winner, row * 2 * C + c, C);
    if (c == 0) cnt[row] = acc[q].n;
  }
}

// ---------------------------------------------------------------------------
// CSR forward: one thread per (node, channel)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pna_csr_fwd(PnaCfg cfg, const float* __restrict__ x,
                                                     const int64_t* __restrict__ row_ptr,
                                                     const int64_t* __restrict__ col, const float* __restrict__ ab,
                                                     const float* __restrict__ avg, float* __restrict__ cat,
                                                     int32_t* __restrict__ cnt, float* __restrict__ stat,
                                                     int32_t* __restrict__ winner, int64_t M, int in, int T, int Fi,
                                                     int divide) {
  const int C = T * Fi, K1 = (1 + cfg.A * cfg.S) * Fi;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= M * C) return;
  const int64_t row = tid / C;
  const int c = (int)(tid - row * C);
  const int t = c / Fi, f = c - t * Fi;
  PnaAcc acc;
  acc.init();
  const int64_t e0 = row_ptr[row], e1 = row_ptr[row + 1];
  for (int64_t e = e0; e < e1; ++e) acc.add(ab[((size_t)col[e] * T + t) * 2 * Fi + Fi + f], (int)e, cfg);
  const float a = ab[((size_t)row * T + t) * 2 * Fi + f];
  const float xv = x[(size_t)row * in + (divide ? t * Fi : 0) + f];
  pna_emit<int32_t>(cfg, acc, a, xv, avg, cat + ((size_t)row * T + t) * K1, f, Fi, stat, winner,
                    (size_t)row * 2 * C + c, C);
  if (c == 0) cnt[row] = acc.n;
}

// ---------------------------------------------------------------------------
// backward, per (row, channel): the scalers folded into one gradient per aggregator, the gradient of a, and the four
// per-row coefficients the transpose pass reads, q [R, 4, C]:
//   q0 = g_sum + g_mean / n        to every neighbour
//   q1 = 2 g_var / n + g_std / (n std)   (the std term 0 where std was clamped or masked), times (b_j - mean_b)
//   q2 = g_min, q3 = g_max         to the winner
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pna_fold(PnaCfg cfg, const float* __restrict__ g_cat,
                                                  const int32_t* __restrict__ cnt, const float* __restrict__ stat,
                                                  const float* __restrict__ avg, float* __restrict__ g_ab,
                                                  float* __restrict__ q, int64_t R, int T, int Fi) {
  const int C = T * Fi, K1 = (1 + cfg.A * cfg.S) * Fi;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= R * C) return;
  const int64_t row = tid / C;
  const int c = (int)(tid - row * C);
  const int t = c / Fi, f = c - t * Fi;
  const int n = cnt[row];
  double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double q0 = 0.0, q1 = 0.0, ga = 0.0;
  if (n > 0) {
    const double avg_lin = (double)avg[0], avg_log = (double)avg[1];
    const float* gc = g_cat + ((size_t)row * T + t) * K1;
    for (int s = 0; s < cfg.S; ++s) {
      const double sc = pna_scaler(cfg.scal[s], n, avg_lin, avg_log);
      for (int k = 0; k < cfg.A; ++k) g[cfg.aggr[k]] += sc * (double)gc[(size_t)Fi * (1 + s * cfg.A + k) + f];
    }
    const double inv = 1.0 / (double)n;
    ga = (double)n * g[GCM_PNA_SUM] + g[GCM_PNA_MEAN] + g[GCM_PNA_MIN] + g[GCM_PNA_MAX];
    q0 = g[GCM_PNA_SUM] + g[GCM_PNA_MEAN] * inv;
    if (cfg.need_var) {
      const float stdv = stat[(size_t)row * 2 * C + C + c];
      q1 = 2.0 * g[GCM_PNA_VAR] * inv;
      if (stdv > 0.f) q1 += g[GCM_PNA_STD] * inv / (double)stdv;
    }
  }
  g_ab[((size_t)row * T + t) * 2 * Fi + f] = (float)ga;
  float* qr = q + (size_t)row * 4 * C + c;
  qr[0] = (float)q0, qr[C] = (float)q1, qr[2 * C] = (float)g[GCM_PNA_MIN], qr[3 * C] = (float)g[GCM_PNA_MAX];
}

// what a sink (row d) contributes to the gradient of b of one of its sources, whose value is bj and whose name in the
// winner arrays is `who`
template <typename W>
__device__ __forceinline__ double pna_share(const PnaCfg& cfg, const float* __restrict__ q,
                                           const float* __restrict__ stat, const W* __restrict__ winner, size_t d,
                                           int c, int C, float bj, int who) {
  const float* qr = q + d * 4 * C + c;
  double v = (double)qr[0];
  if (cfg.need_var) v += (double)qr[C] * ((double)bj - (double)stat[d * 2 * C + c]);
  if (cfg.need_mm) {
    if ((int)winner[d * 2 * C + c] == who) v += (double)qr[2 * C];
    if ((int)winner[d * 2 * C + C + c] == who) v += (double)qr[3 * C];
  }
  return v;
}

// dense transpose pass: one thread per (graph, source j, channel), the sinks i in ascending order
__global__ __launch_bounds__(256) void k_pna_dense_bwd(PnaCfg cfg, const float* __restrict__ adj,
                                                       const float* __restrict__ ab, const float* __restrict__ q,
                                                       const float* __restrict__ stat,
                                                       const int16_t* __restrict__ winner, float* __restrict__ g_ab,
                                                       int64_t R, int N, int T, int Fi, int add_loop) {
  const int C = T * Fi;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= R * C) return;
  const int64_t row = tid / C;
  const int c = (int)(tid - row * C);
  const int t = c / Fi, f = c - t * Fi;
  const int64_t b = row / N;
  const int j = (int)(row - b * N);
  const size_t o = ((size_t)row * T + t) * 2 * Fi + Fi + f;
  const float bj = ab[o];
  const float* adj_b = adj + (size_t)b * N * N;
  double acc = 0.0;  // fp64: rounded once
  for (int i = 0; i < N; ++i)
    if (adj_b[(size_t)i * N + j] != 0.f || (add_loop && i == j))
      acc += pna_share<int16_t>(cfg, q, stat, winner, (size_t)b * N + i, c, C, bj, j);
  g_ab[o] = (float)acc;
}

// CSR transpose pass: one thread per (source j, channel), the CSC column of j in its order
__global__ __launch_bounds__(256) void k_pna_csr_bwd(PnaCfg cfg, const int64_t* __restrict__ col_ptr,
                                                     const int64_t* __restrict__ rows,
                                                     const int64_t* __restrict__ perm, const float* __restrict__ ab,
                                                     const float* __restrict__ q, const float* __restrict__ stat,
                                                     const int32_t* __restrict__ winner, float* __restrict__ g_ab,
                                                     int64_t M, int T, int Fi) {
  const int C = T * Fi;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= M * C) return;
  const int64_t row = tid / C;
  const int c = (int)(tid - row * C);
  const int t = c / Fi, f = c - t * Fi;
  const size_t o = ((size_t)row * T + t) * 2 * Fi + Fi + f;
  const float bj = ab[o];
  double acc = 0.0;
  if (col_ptr)
    for (int64_t k = col_ptr[row]; k < col_ptr[row + 1]; ++k)
      acc += pna_share<int32_t>(cfg, q, stat, winner, (size_t)rows[k], c, C, bj, (int)perm[k]);
  g_ab[o] = (float)acc;
}

// g_x = the x block of g_cat plus g_ab W_pre (tmp), summed over the towers in order unless each has its own columns
__global__ __launch_bounds__(256) void k_pna_gx(const float* __restrict__ g_cat, const float* __restrict__ tmp,
                                                float* __restrict__ g_x, int64_t R, int in, int T, int Fi, int K1,
                                                int divide) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (tid >= R * in) return;
  const int64_t row = tid / in;
  const int col = (int)(tid - row * in);
  double v = 0.0;
  if (divide) {
    const int t = col / Fi, f = col - t * Fi;
    v = (double)g_cat[((size_t)row * T + t) * K1 + f] + (double)tmp[((size_t)row * T + t) * Fi + f];
  } else {
    for (int t = 0; t < T; ++t)
      v += (double)g_cat[((size_t)row * T + t) * K1 + col] + (double)tmp[((size_t)row * T + t) * Fi + col];
  }
  g_x[tid] = (float)v;
}

// ---------------------------------------------------------------------------
// the input gradients of the linears: gcn_mm.h's tile step with leading dimensions, and every K tile started from a
// zero accumulator and then added to the running sum (mma32_tiles): the post linear's K is (1 + A S) F_in, up to 3968,
// and one fp32 chain of that length over scaled sums misses the tests' bound; with the tiles a chain is 32 products.
// ---------------------------------------------------------------------------
struct PmmArgs {
  const float* A;
  int64_t a_is, a_ks;
  const float* B;
  int64_t b_ks, b_js;
  float* C;               // C(i, j) at C[i * c_is + j]
  int64_t c_is;
  const float* bias;      // C(i, j) += bias[j]
  int M, N, K;
};

template <int NCT>
__global__ __launch_bounds__(256) void k_pna_mm(PmmArgs p) {
  __shared__ float sA[MB * (KT + 1)];        // [i][k]
  __shared__ float sB[KT * (32 * NCT + 1)];  // [k][j]
  const int i0 = blockIdx.x * MB, j0 = blockIdx.y * 32 * NCT;
  const TileLane t = tile_lane();
  const bool a_rfast = p.a_is == 1 && p.a_ks != 1;  // coalesced order of the global reads
  const bool b_kfast = p.b_ks == 1 && p.b_js != 1;
  f32x16 acc[NCT];
  tile_zero(acc);
  tile_mma<NCT, true>(
      acc, t, sA, sB, i0, j0, p.M, p.N, 0, p.K, a_rfast, b_kfast,
      [=](int gi, int gk) { return p.A[(size_t)gi * p.a_is + (size_t)gk * p.a_ks]; },
      [=](int gk, int gj) { return p.B[(size_t)gk * p.b_ks + (size_t)gj * p.b_js]; });
  tile_store(acc, t, i0, j0, p.M, p.N, [=](int j) {
    const float bias = p.bias ? p.bias[j] : 0.f;
    return [=](int i, float v) { p.C[(size_t)i * p.c_is + j] = v + bias; };
  });
}

int launch_pmm(const PmmArgs& p, hipStream_t s) {
  const int nct = nct_of(p.N);
  const dim3 grid(blocks(p.M, MB), blocks(p.N, 32 * nct));
  dispatch_nct(nct, [&](auto n) { hipLaunchKernelGGL(k_pna_mm<n()>, grid, dim3(256), 0, s, p); });
  return gcm_launch_status();
}

// The forward linears (pre, post, final): the same tiles with fp64 FMAs of the exact fp32 products on the vector ALUs,
// rounded once when stored.  What they write - a, b, the post linear's output h - is saved and multiplied again in the
// backward (g_w_lin = g^T h), so its error is a gradient's error: with the fp32 tile kernel h was a few ulp off, at
// magnitudes of tens, and a memory's accumulated lin.weight gradient missed the tests' bound because of it alone
// (every other gradient of the layer used a quarter of its bound).  A thread owns 4 rows x NC/8 columns of the tile, so
// that one LDS read of an operand feeds 4 or more FMAs and the fp64 pipe, not LDS, sets the pace.
template <int NCT>
__global__ __launch_bounds__(256) void k_pna_mm64(PmmArgs p) {
  constexpr int NC = 32 * NCT, CC = NC / 8, RR = MB / 32;
  __shared__ float sA[MB * (KT + 1)];  // [i][k]
  __shared__ double sB[KT * NC];       // [k][j]
  const int i0 = blockIdx.x * MB, j0 = blockIdx.y * NC;
  const int rg = threadIdx.x >> 3, c0 = (threadIdx.x & 7) * CC;  // rows rg + 32 q, columns c0 .. c0 + CC
  const bool a_rfast = p.a_is == 1 && p.a_ks != 1;  // coalesced order of the global reads
  const bool b_kfast = p.b_ks == 1 && p.b_js != 1;
  double acc[RR][CC];
#pragma unroll
  for (int q = 0; q < RR; ++q)
#pragma unroll
    for (int u = 0; u < CC; ++u) acc[q][u] = 0.0;

  for (int k0 = 0; k0 < p.K; k0 += KT) {
    tile_stage_a(sA, i0, p.M, k0, p.K, a_rfast,
                 [=](int gi, int gk) { return p.A[(size_t)gi * p.a_is + (size_t)gk * p.a_ks]; });
    for (int e = threadIdx.x; e < KT * NC; e += 256) {
      const int k = b_kfast ? e % KT : e / NC, j = b_kfast ? e / KT : e % NC;
      const int gk = k0 + k, gj = j0 + j;
      sB[k * NC + j] = (gk < p.K && gj < p.N) ? (double)p.B[(size_t)gk * p.b_ks + (size_t)gj * p.b_js] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < KT; ++k) {
      double a[RR];
#pragma unroll
      for (int q = 0; q < RR; ++q) a[q] = (double)sA[(rg + 32 * q) * (KT + 1) + k];
      const double* b = sB + k * NC + c0;
#pragma unroll
      for (int u = 0; u < CC; ++u) {
        const double bu = b[u];
#pragma unroll
        for (int q = 0; q < RR; ++q) acc[q][u] = fma(a[q], bu, acc[q][u]);
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int q = 0; q < RR; ++q) {
    const int i = i0 + rg + 32 * q;
    if (i >= p.M) continue;
#pragma unroll
    for (int u = 0; u < CC; ++u) {
      const int j = j0 + c0 + u;
      if (j < p.N) p.C[(size_t)i * p.c_is + j] = (float)(acc[q][u] + (p.bias ? (double)p.bias[j] : 0.0));
    }
  }
}

int launch_pmm64(const PmmArgs& p, hipStream_t s) {
  const int nct = nct_of(p.N);
  const dim3 grid(blocks(p.M, MB), blocks(p.N, 32 * nct));
  dispatch_nct(nct, [&](auto n) { hipLaunchKernelGGL(k_pna_mm64<n()>, grid, dim3(256), 0, s, p); });
  return gcm_launch_status();
}

// Column sums for the bias gradients, in fp64 and a fixed order: slabs of PCS_ROWS rows, then the slabs in sequence.
constexpr int PCS_ROWS = 256;

__global__ __launch_bounds__(256) void k_pna_colsum_slabs(const float* __restrict__ src, int64_t R, int F,
                                                          double* __restrict__ slabs) {
  const int64_t r0 = (int64_t)blockIdx.x * PCS_ROWS;
  const int64_t r1 = min(R, r0 + PCS_ROWS);
  for (int f = threadIdx.x; f < F; f += 256) {
    double a = 0.0;
    for (int64_t r = r0; r < r1; ++r) a += (double)src[(size_t)r * F + f];
    slabs[(size_t)blockIdx.x * F + f] = a;
  }
}

__global__ __launch_bounds__(256) void k_pna_colsum_final(const double* __restrict__ slabs, int n, int F,
                                                          float* __restrict__ out) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  double a = 0.0;
  for (int k = 0; k < n; ++k) a += slabs[(size_t)k * F + f];
  out[f] = (float)a;
}

int64_t pna_colsum_slabs(int64_t R) { return (R + PCS_ROWS - 1) / PCS_ROWS; }

int pna_colsum(const float* src, int64_t R, int F, float* out, double* slabs, hipStream_t s) {
  const int n = (int)pna_colsum_slabs(R);
  hipLaunchKernelGGL(k_pna_colsum_slabs, dim3(n), dim3(256), 0, s, src, R, F, slabs);
  int rc = gcm_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(k_pna_colsum_final, dim3(blocks(F, 256)), dim3(256), 0, s, (const double*)slabs, n, F, out);
  return gcm_launch_status();
}

// y[R, Fo] (ld ldy) = x[R, Fi] (ld ldx) W^T + bias,  W [Fo, Fi]
int lin_fwd(const float* x, int64_t ldx, const float* w, const float* bias, float* y, int64_t ldy, int64_t R, int Fi,
            int Fo, hipStream_t s) {
  PmmArgs p = {};
  p.A = x, p.a_is = ldx, p.a_ks = 1;
  p.B = w, p.b_ks = 1, p.b_js = Fi;
  p.C = y, p.c_is = ldy, p.bias = bias;
  p.M = (int)R, p.N = Fo, p.K = Fi;
  return launch_pmm64(p, s);
}

// c[R, Fi] (ld ldc) = g[R, Fo] (ld ldg) W,  W [Fo, Fi]
int lin_bwd_x(const float* g, int64_t ldg, const float* w, float* c, int64_t ldc, int64_t R, int Fi, int Fo,
              hipStream_t s) {
  PmmArgs p = {};
  p.A = g, p.a_is = ldg, p.a_ks = 1;
  p.B = w, p.b_ks = Fi, p.b_js = 1;
  p.C = c, p.c_is = ldc;
  p.M = (int)R, p.N = Fi, p.K = Fo;
  return launch_pmm(p, s);
}

// Weight gradients, gw[Fo, Fi] = sum_r g[r, :Fo]^T x[r, :Fi], as split-K slabs in fp64 summed in fixed order.  The rows
// are the batch: a sum over them of products of scaled neighbourhood sums, whose partial sums are far larger than the
// result.  One fp32 chain per 32 rows met the tests' bound on the layers' own cases and missed it by a quarter on a
// memory's accumulated gradient; fp64 FMAs of the exact fp32 products, rounded once, leave the operands' own fp32
// as the only error.  A workgroup owns 16 x 64 entries of gw over one slab of rows, staged 32 rows at a time in LDS;
// a thread 4 entries.
constexpr int PW_FO = 16, PW_FI = 64, PW_RT = 32;

void pna_wgrad_plan(int64_t R, int* nslab, int64_t* rows) {
  const int n = (int)std::max<int64_t>(1, std::min<int64_t>(256, (R + 127) / 128));
  *rows = (R + n - 1) / n;
  *nslab = (int)((R + *rows - 1) / *rows);
}

__global__ __launch_bounds__(256) void k_pna_wgrad(const float* __restrict__ g, int64_t ldg,
                                                   const float* __restrict__ x, int64_t ldx,
                                                   double* __restrict__ slabs, int64_t R, int64_t rows, int Fi,
                                                   int Fo) {
  __shared__ float sG[PW_RT][PW_FO];
  __shared__ float sX[PW_RT][PW_FI];
  const int fi0 = blockIdx.x * PW_FI, fo0 = blockIdx.y * PW_FO;
  const int64_t r0 = (int64_t)blockIdx.z * rows, r1 = min(R, r0 + rows);
  const int ti = threadIdx.x & 63, to = (threadIdx.x >> 6) * 4;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t rb = r0; rb < r1; rb += PW_RT) {
    for (int e = threadIdx.x; e < PW_RT * PW_FO; e += 256) {
      const int r = e / PW_FO, f = e % PW_FO;
      sG[r][f] = (rb + r < r1 && fo0 + f < Fo) ? g[(size_t)(rb + r) * ldg + fo0 + f] : 0.f;
    }
    for (int e = threadIdx.x; e < PW_RT * PW_FI; e += 256) {
      const int r = e / PW_FI, f = e % PW_FI;
      sX[r][f] = (rb + r < r1 && fi0 + f < Fi) ? x[(size_t)(rb + r) * ldx + fi0 + f] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < PW_RT; ++r) {
      const double xv = (double)sX[r][ti];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fma((double)sG[r][to + u], xv, acc[u]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int fo = fo0 + to + u, fi = fi0 + ti;
    if (fo < Fo && fi < Fi) slabs[((size_t)blockIdx.z * Fo + fo) * Fi + fi] = acc[u];
  }
}

int lin_bwd_w(const float* g, int64_t ldg, const float* x, int64_t ldx, float* gw, double* slabs, int64_t R, int Fi,
              int Fo, hipStream_t s) {
  int nslab;
  int64_t rows;
  pna_wgrad_plan(R, &nslab, &rows);
  hipLaunchKernelGGL(k_pna_wgrad, dim3(blocks(Fi, PW_FI), blocks(Fo, PW_FO), nslab), dim3(256), 0, s, g, ldg, x, ldx,
                     slabs, R, rows, Fi, Fo);
  const int rc = gcm_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(k_pna_colsum_final, dim3(blocks((int64_t)Fo * Fi, 256)), dim3(256), 0, s, (const double*)slabs,
                     nslab, Fo * Fi, gw);
  return gcm_launch_status();
}

// a, b of every tower: ab[:, t] = x_t w_pre[t]^T + b_pre[t]
int pna_pre(const PnaDims& d, const float* x, const float* w_pre, const float* b_pre, float* ab, hipStream_t s) {
  for (int t = 0; t < d.T; ++t) {
    const int rc = lin_fwd(x + (d.divide ? t * d.Fi : 0), d.in, w_pre + (size_t)t * 2 * d.Fi * d.Fi,
                           b_pre + (size_t)t * 2 * d.Fi, ab + (size_t)t * 2 * d.Fi, (int64_t)d.T * 2 * d.Fi, d.R, d.Fi,
                           2 * d.Fi, s);
    if (rc) return rc;
  }
  return GCM_OK;
}

// h_t = cat[:, t] w_post[t]^T + b_post[t], then out = h w_lin^T + b_lin (or out = h without w_lin)
int pna_post(const PnaDims& d, const float* cat, const float* w_post, const float* b_post, const float* w_lin,
             const float* b_lin, float* h, float* out, hipStream_t s) {
  float* dst = w_lin ? h : out;
  for (int t = 0; t < d.T; ++t) {
    const int rc = lin_fwd(cat + (size_t)t * d.K1, (int64_t)d.T * d.K1, w_post + (size_t)t * d.Fo * d.K1,
                           b_post + (size_t)t * d.Fo, dst + (size_t)t * d.Fo, d.out, d.R, d.K1, d.Fo, s);
    if (rc) return rc;
  }
  return w_lin ? lin_fwd(h, d.out, w_lin, b_lin, out, d.out, d.R, d.out, d.out, s) : GCM_OK;
}

struct PnaWs {
  size_t g_h, g_cat, q, g_ab, tmp, slabs, total;
};

PnaWs pna_ws(const PnaDims& d) {
  PnaWs w;
  Carve cv;
  w.g_h = cv.take(d.R * d.out * sizeof(float));
  w.g_cat = cv.take(d.R * d.T * d.K1 * sizeof(float));
  w.q = cv.take(d.R * 4 * d.C * sizeof(float));
  w.g_ab = cv.take(d.R * 2 * d.C * sizeof(float));
  w.tmp = cv.take(d.R * d.C * sizeof(float));
  w.slabs = cv.at;  // the last field: not rounded up
  int nslab;
  int64_t rows;
  pna_wgrad_plan(d.R, &nslab, &rows);
  const size_t wmax = std::max<size_t>({(size_t)d.out * d.out, (size_t)d.Fo * d.K1, (size_t)2 * d.Fi * d.Fi});
  const size_t doubles = std::max<size_t>((size_t)nslab * wmax,
                                          (size_t)pna_colsum_slabs(d.R) * std::max(d.out, 2 * d.C));
  w.total = w.slabs + doubles * sizeof(double);
  return w;
}

// the backward up to the per-aggregator gradients: g_h, the post and final linears' gradients, g_cat
int pna_bwd_head(const PnaDims& d, const PnaWs& L, char* ws, const float* g_out, const float* w_post,
                 const float* w_lin, const float* cat, const float* h, float* g_w_post, float* g_b_post,
                 float* g_w_lin, float* g_b_lin, hipStream_t s) {
  double* slabs = (double*)(ws + L.slabs);
  float* g_cat = (float*)(ws + L.g_cat);
  const float* g_h = g_out;
  int rc;
  if (w_lin) {
    if (g_w_lin && (rc = lin_bwd_w(g_out, d.out, h, d.out, g_w_lin, slabs, d.R, d.out, d.out, s))) return rc;
    if (g_b_lin && (rc = pna_colsum(g_out, d.R, d.out, g_b_lin, slabs, s))) return rc;
    if ((rc = lin_bwd_x(g_out, d.out, w_lin, (float*)(ws + L.g_h), d.out, d.R, d.out, d.out, s))) return rc;
    g_h = (const float*)(ws + L.g_h);
  }
  if (g_b_post && (rc = pna_colsum(g_h, d.R, d.out, g_b_post, slabs, s))) return rc;
  for (int t = 0; t < d.T; ++t) {
    if (g_w_post && (rc = lin_bwd_w(g_h + (size_t)t * d.Fo, d.out, cat + (size_t)t * d.K1, (int64_t)d.T * d.K1,
                                    g_w_post + (size_t)t * d.Fo * d.K1, slabs, d.R, d.K1, d.Fo, s)))
      return rc;
    if ((rc = lin_bwd_x(g_h + (size_t)t * d.Fo, d.out, w_post + (size_t)t * d.Fo * d.K1, g_cat + (size_t)t * d.K1,
                        (int64_t)d.T * d.K1, d.R, d.K1, d.Fo, s)))
      return rc;
  }
  return GCM_OK;
}

// the backward from g_ab on: the pre linear's gradients and g_x
int pna_bwd_tail(const PnaDims& d, const PnaWs& L, char* ws, const float* x, const float* w_pre, float* g_x,
                 float* g_w_pre, float* g_b_pre, hipStream_t s) {
  double* slabs = (double*)(ws + L.slabs);
  const float* g_ab = (const float*)(ws + L.g_ab);
  float* tmp = (float*)(ws + L.tmp);
  const int64_t ld = (int64_t)d.T * 2 * d.Fi;
  int rc;
  if (g_b_pre && (rc = pna_colsum(g_ab, d.R, (int)ld, g_b_pre, slabs, s))) return rc;
  for (int t = 0; t < d.T; ++t) {
    const float* g_t = g_ab + (size_t)t * 2 * d.Fi;
    if (g_w_pre && (rc = lin_bwd_w(g_t, ld, x + (d.divide ? t * d.Fi : 0), d.in, g_w_pre + (size_t)t * 2 * d.Fi * d.Fi,
                                   slabs, d.R, d.Fi, 2 * d.Fi, s)))
      return rc;
    if (g_x && (rc = lin_bwd_x(g_t, ld, w_pre + (size_t)t * 2 * d.Fi * d.Fi, tmp + (size_t)t * d.Fi,
                               (int64_t)d.T * d.Fi, d.R, d.Fi, 2 * d.Fi, s)))
      return rc;
  }
  if (g_x) {
    hipLaunchKernelGGL(k_pna_gx, dim3(blocks(d.R * d.in, 256)), dim3(256), 0, s, (const float*)(ws + L.g_cat), tmp, g_x,
                       d.R, d.in, d.T, d.Fi, d.K1, d.divide);
    return gcm_launch_status();
  }
  return GCM_OK;
}

int pna_fold(const PnaDims& d, const PnaCfg& cfg, const PnaWs& L, char* ws, const int32_t* cnt, const float* stat,
             const float* avg, hipStream_t s) {
  hipLaunchKernelGGL(k_pna_fold, dim3(blocks(d.R * d.C, 256)), dim3(256), 0, s, cfg, (const float*)(ws + L.g_cat), cnt,
                     stat, avg, (float*)(ws + L.g_ab), (float*)(ws + L.q), d.R, d.T, d.Fi);
  return gcm_launch_status();
}

bool pna_dense_ok(int B, int N, int in, int out, const PnaDims& d) {
  return in <= 128 && out <= 128 && B <= 65535 && N <= 32767 && (int64_t)B * N <= (1 << 30) &&
         (d.C + 31) / 32 <= 65535 && (int64_t)d.R * d.C <= ((int64_t)1 << 38);
}

bool pna_csr_ok(int64_t M, int64_t E, int in, int out, const PnaDims& d) {
  return in <= 128 && out <= 128 && M <= (1 << 30) && E <= INT32_MAX && (int64_t)d.R * d.C <= ((int64_t)1 << 38);
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: dense
// ---------------------------------------------------------------------------
extern "C" int gcm_dense_pnaconv_fwd(const float* x, const float* adj, const float* w_pre, const float* b_pre,
                                     const float* w_post, const float* b_post, const float* w_lin,
                                     const float* b_lin, const float* avg_deg, float* out, float* ab, float* cat,
                                     float* h, int32_t* cnt, float* stat, int16_t* winner, int B, int N,
                                     int in_channels, int out_channels, int towers, int divide_input, int aggrs, int A,
                                     int scalers, int S, int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && w_pre && b_pre && w_post && b_post && avg_deg && out && ab && cat && cnt);
  GCM_REQUIRE(B > 0 && N > 0);
  PnaCfg cfg;
  PnaDims d;
  GCM_REQUIRE(pna_cfg(aggrs, A, scalers, S, &cfg) && pna_dims((int64_t)B * N, in_channels, out_channels, towers,
                                                               divide_input, A, S, &d));
  GCM_REQUIRE((!w_lin || h) && (w_lin || !b_lin) && (!cfg.need_var || stat) && (!cfg.need_mm || winner));
  if (!pna_dense_ok(B, N, in_channels, out_channels, d)) return GCM_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = pna_pre(d, x, w_pre, b_pre, ab, s))) return rc;
  if (d.C <= 32) {
    hipLaunchKernelGGL(k_pna_dense_fwd<1>, dim3(blocks(N, PR), B, 1), dim3(256), 0, s, cfg, x, adj, ab, avg_deg, cat,
                       cnt, stat, winner, N, d.in, d.T, d.Fi, d.divide, add_loop);
  } else {
    hipLaunchKernelGGL(k_pna_dense_fwd<2>, dim3(blocks(N, PR), B, blocks(d.C, 64)), dim3(256), 0, s, cfg, x, adj, ab,
                       avg_deg, cat, cnt, stat, winner, N, d.in, d.T, d.Fi, d.divide, add_loop);
  }
  if ((rc = gcm_launch_status())) return rc;
  return pna_post(d, cat, w_post, b_post, w_lin, b_lin, h, out, s);
}

extern "C" size_t gcm_dense_pnaconv_bwd_workspace_bytes(int B, int N, int in_channels, int out_channels, int towers,
                                                        int divide_input, int A, int S) {
  PnaDims d;
  if (B <= 0 || N <= 0 || A < 1 || S < 1 ||
      !pna_dims((int64_t)B * N, in_channels, out_channels, towers, divide_input, A, S, &d))
    return 0;
  return pna_ws(d).total;
}

extern "C" int gcm_dense_pnaconv_bwd(const float* g_out, const float* x, const float* adj, const float* w_pre,
                                     const float* w_post, const float* w_lin, const float* avg_deg, const float* ab,
                                     const float* cat, const float* h, const int32_t* cnt, const float* stat,
                                     const int16_t* winner, float* g_x, float* g_w_pre, float* g_b_pre,
                                     float* g_w_post, float* g_b_post, float* g_w_lin, float* g_b_lin, void* workspace,
                                     size_t workspace_bytes, int B, int N, int in_channels, int out_channels,
                                     int towers, int divide_input, int aggrs, int A, int scalers, int S, int add_loop,
                                     gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && adj && w_pre && w_post && avg_deg && ab && cat && cnt && workspace);
  GCM_REQUIRE(B > 0 && N > 0);
  PnaCfg cfg;
  PnaDims d;
  GCM_REQUIRE(pna_cfg(aggrs, A, scalers, S, &cfg) && pna_dims((int64_t)B * N, in_channels, out_channels, towers,
                                                               divide_input, A, S, &d));
  GCM_REQUIRE((!w_lin || h) && (w_lin || (!g_w_lin && !g_b_lin)) && (!cfg.need_var || stat) &&
              (!cfg.need_mm || winner));
  if (!pna_dense_ok(B, N, in_channels, out_channels, d)) return GCM_EUNSUPPORTED;
  const PnaWs L = pna_ws(d);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int rc;
  if ((rc = pna_bwd_head(d, L, ws, g_out, w_post, w_lin, cat, h, g_w_post, g_b_post, g_w_lin, g_b_lin, s))) return rc;
  if (!g_x && !g_w_pre && !g_b_pre) return GCM_OK;
  if ((rc = pna_fold(d, cfg, L, ws, cnt, stat, avg_deg, s))) return rc;
  hipLaunchKernelGGL(k_pna_dense_bwd, dim3(blocks(d.R * d.C, 256)), dim3(256), 0, s, cfg, adj, ab,
                     (const float*)(ws + L.q), stat, winner, (float*)(ws + L.g_ab), d.R, N, d.T, d.Fi, add_loop);
  if ((rc = gcm_launch_status())) return rc;
  return pna_bwd_tail(d, L, ws, x, w_pre, g_x, g_w_pre, g_b_pre, s);
}

// ---------------------------------------------------------------------------
// C ABI: CSR
// ---------------------------------------------------------------------------
extern "C" int gcm_csr_pnaconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* w_pre,
                                   const float* b_pre, const float* w_post, const float* b_post, const float* w_lin,
                                   const float* b_lin, const float* avg_deg, float* out, float* ab, float* cat,
                                   float* h, int32_t* cnt, float* stat, int32_t* winner, int64_t M, int64_t E,
                                   int in_channels, int out_channels, int towers, int divide_input, int aggrs, int A,
                                   int scalers, int S, gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && w_pre && b_pre && w_post && b_post && avg_deg && out && ab && cat && cnt);
  GCM_REQUIRE(M > 0 && E >= 0 && (E == 0 || col));
  PnaCfg cfg;
  PnaDims d;
  GCM_REQUIRE(pna_cfg(aggrs, A, scalers, S, &cfg) && pna_dims(M, in_channels, out_channels, towers, divide_input, A,
                                                               S, &d));
  GCM_REQUIRE((!w_lin || h) && (w_lin || !b_lin) && (!cfg.need_var || stat) && (!cfg.need_mm || winner));
  if (!pna_csr_ok(M, E, in_channels, out_channels, d)) return GCM_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = pna_pre(d, x, w_pre, b_pre, ab, s))) return rc;
  hipLaunchKernelGGL(k_pna_csr_fwd, dim3(blocks(M * d.C, 256)), dim3(256), 0, s, cfg, x, row_ptr, col, ab, avg_deg,
                     cat, cnt, stat, winner, M, d.in, d.T, d.Fi, d.divide);
  if ((rc = gcm_launch_status())) return rc;
  return pna_post(d, cat, w_post, b_post, w_lin, b_lin, h, out, s);
}

extern "C" size_t gcm_csr_pnaconv_bwd_workspace_bytes(int64_t M, int64_t E, int in_channels, int out_channels,
                                                      int towers, int divide_input, int A, int S) {
  PnaDims d;
  if (M <= 0 || E < 0 || A < 1 || S < 1 || !pna_dims(M, in_channels, out_channels, towers, divide_input, A, S, &d))
    return 0;
  return pna_ws(d).total;
}

extern "C" int gcm_csr_pnaconv_bwd(const float* g_out, const float* x, const int64_t* col_ptr, const int64_t* rows,
                                   const int64_t* perm, const float* w_pre, const float* w_post, const float* w_lin,
                                   const float* avg_deg, const float* ab, const float* cat, const float* h,
                                   const int32_t* cnt, const float* stat, const int32_t* winner, float* g_x,
                                   float* g_w_pre, float* g_b_pre, float* g_w_post, float* g_b_post, float* g_w_lin,
                                   float* g_b_lin, void* workspace, size_t workspace_bytes, int64_t M, int64_t E,
                                   int in_channels, int out_channels, int towers, int divide_input, int aggrs, int A,
                                   int scalers, int S, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && w_pre && w_post && avg_deg && ab && cat && cnt && workspace);
  GCM_REQUIRE(M > 0 && E >= 0);
  PnaCfg cfg;
  PnaDims d;
  GCM_REQUIRE(pna_cfg(aggrs, A, scalers, S, &cfg) && pna_dims(M, in_channels, out_channels, towers, divide_input, A,
                                                               S, &d));
  GCM_REQUIRE((!w_lin || h) && (w_lin || (!g_w_lin && !g_b_lin)) && (!cfg.need_var || stat) &&
              (!cfg.need_mm || winner));
  const bool need_pre = g_x || g_w_pre || g_b_pre;
  GCM_REQUIRE(E == 0 || !need_pre || (col_ptr && rows && perm));
  if (!pna_csr_ok(M, E, in_channels, out_channels, d)) return GCM_EUNSUPPORTED;
  const PnaWs L = pna_ws(d);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int rc;
  if ((rc = pna_bwd_head(d, L, ws, g_out, w_post, w_lin, cat, h, g_w_post, g_b_post, g_w_lin, g_b_lin, s))) return rc;
  if (!need_pre) return GCM_OK;
  if ((rc = pna_fold(d, cfg, L, ws, cnt, stat, avg_deg, s))) return rc;
  hipLaunchKernelGGL(k_pna_csr_bwd, dim3(blocks(M * d.C, 256)), dim3(256), 0, s, cfg, E > 0 ? col_ptr : nullptr, rows,
                     perm, ab, (const float*)(ws + L.q), stat, winner, (float*)(ws + L.g_ab), M, d.T, d.Fi);
  if ((rc = gcm_launch_status())) return rc;
  return pna_bwd_tail(d, L, ws, x, w_pre, g_x, g_w_pre, g_b_pre, s);
}
