// GatedGraphConv / DenseGatedGraphConv (PyG; Li et al., Gated Graph Sequence Neural Networks) on gfx950.
//
//   h_0 = x zero-padded to C columns;  for l < L:
//     m   = A (h_l W_l)                               (A: adj, dense; the weighted edge list, sparse)
//     gi  = m W_ih^T + b_ih,  gh = h_l W_hh^T + b_hh  (gate order r, z, n)
//     r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n),  h_{l+1} = (1 - z) n + z h_l
//
// Forward, ONE launch per round (k_gg_round).  The projection is folded in by associativity, m = (A h_l) W_l: the
// neighbour sum then reads h_l, which the round only reads, so no projected copy p_l makes a round trip through HBM
// and no GEMM launch precedes the sweep; the price is a [rows, C] x [C, C] product per tile on the matrix cores,
// which idle during the sweep anyway.  A workgroup owns 128 / NCTP consecutive rows (NCTP = 1, 2, 4 column tiles of 32
// for C <= 32, 64, 128): (1) a group of 32 lanes per row walks the set bits of the pattern's image (attn_bits.h; adj
// is read for set bits only; when the workgroup's rows lie in one graph the neighbours' h comes in LDS tiles of 32 and
// tiles without a bit are skipped) or the row of the CSR, u = A h into LDS, the tile of h beside it; (2) m = u W_l on
// v_mfma_f32_32x32x2_f32, W_l staged through LDS in K tiles, m over u in LDS and out to `saved`; (3) the two gate
// products, all six [C, C] blocks of W_ih / W_hh staged per K tile (32 / NCTP rows of K: 24 KB whatever C), r and z
// accumulating gi + gh in one tile; (4) the GRU on the accumulators, in double (exp, tanh, IEEE division) with one
// rounding per stored value: fp32 gates cost the backward several ulp on small graphs.  gi, gh and the gates'
// arguments never leave the registers; r, z, n and gh_n (with bias) are stored for the backward.
//
// Backward, rounds in reverse, five launches per round: the pointwise adjoints G = [g_r | g_z | g_n | g_n r]
// (pre-activation; gi's adjoint is the first three blocks, gh's the blocks 0, 1, 3), g_m = G_gi W_ih,
// g_h = g_h' z + G_gh W_hh, g_p = A^T g_m (the transposed image, dense; the CSC, sparse), g_h += g_p W_l^T.  G and
// g_p of every round stay in the workspace, so the parameter gradients are ONE split-K product each over all L R rows
// (chunks of 64 rows, more once that would be over 512 slabs; slabs summed in a fixed order): g_w_ih = G_gi^T m,
// g_w_hh = G_gh^T h, g_weight[l] = h_l^T g_p_l (batched over l), the bias gradients the column sums of G.  When the
// adjacency (edge weights) asks: p_l = h_l W_l is recomputed and g_adj += g_m_l p_l^T (per edge: the dot product).
// No float atomics, no allocation, no host synchronisation: bitwise reproducible and capturable.  C <= 128.
#include <cmath>

#include "attn_bits.h"

namespace {

enum { SLOT_H = 0, SLOT_M, SLOT_R, SLOT_Z, SLOT_N, SLOT_HN, SLOTS };

// the neighbourhood of a row: dense (bit image + adj, by row or transposed) or sparse (CSR / CSC)
struct Nbr {
  const unsigned* bits;   // dense: [R, W], the image (tr: the transposed image)
  const float* adj;       // dense: [R, N]
  int N, W, add_loop, tr;
  const int64_t* ptr;     // sparse: [R + 1], NULL when there are no entries
  const int64_t* idx;     // sparse: the neighbour of each entry
  const int64_t* eperm;   // sparse: entry k weighs ew[eperm[k]] (NULL: ew[k])
  const float* ew;        // sparse: weights or NULL (1)
  int sparse;
};

// finite for every argument: v -> -inf gives 1 / (1 + inf) = 0, v -> +inf gives 1 / (1 + 0) = 1
__device__ __forceinline__ double gg_sigmoid(double v) { return 1.0 / (1.0 + exp(-v)); }

// acc[ch] += sum over the neighbours j of row r of a_rj src[j, gl + 32 ch]   (channels >= C stay untouched)
template <int NCH>
__device__ __forceinline__ void gg_nbr_sum(const Nbr& g, int64_t r, const float* __restrict__ src, int C, int gl,
                                           float* acc) {
  if (g.sparse) {
    if (!g.ptr) return;
    const int64_t e1 = g.ptr[r + 1];
    for (int64_t e = g.ptr[r]; e < e1; ++e) {
      const float a = g.ew ? g.ew[g.eperm ? g.eperm[e] : e] : 1.f;
      const float* s = src + (size_t)g.idx[e] * C;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c = gl + 32 * ch;
        if (c < C) acc[ch] = fmaf(a, s[c], acc[ch]);
      }
    }
    return;
  }
  const int i = (int)(r % g.N);
  const size_t rb = (size_t)(r - i);
  for (int w = 0; w < g.W; ++w) {
    unsigned m = g.bits[(size_t)r * g.W + w];
    while (m) {
      const int j = w * 32 + __ffs(m) - 1;
      m &= m - 1u;
      const float a = (g.add_loop && j == i) ? 1.f : (g.tr ? g.adj[(rb + j) * g.N + i] : g.adj[(size_t)r * g.N + j]);
      const float* s = src + (rb + j) * C;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int c = gl + 32 * ch;
        if (c < C) acc[ch] = fmaf(a, s[c], acc[ch]);
      }
    }
  }
}

// h0[r, c] = c < Fi ? x[r, c] : 0
__global__ __launch_bounds__(256) void k_gg_pad(const float* __restrict__ x, float* __restrict__ h0, int64_t R, int Fi,
                                                int C) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= R * C) return;
  const int64_t r = t / C;
  const int c = (int)(t - r * C);
  h0[t] = c < Fi ? x[(size_t)r * Fi + c] : 0.f;
}

// g_x[r, c] = g_h0[r, c], c < Fi
__global__ __launch_bounds__(256) void k_gg_unpad(const float* __restrict__ g_h0, float* __restrict__ g_x, int64_t R,
                                                  int Fi, int C) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= R * Fi) return;
  const int64_t r = t / Fi;
  const int c = (int)(t - r * Fi);
  g_x[t] = g_h0[(size_t)r * C + c];
}

// ---------------------------------------------------------------------------
// forward: one round
// ---------------------------------------------------------------------------
struct RoundArgs {
  const float *h, *w_l, *w_ih, *w_hh, *b_ih, *b_hh;
  float *m, *rg, *zg, *ng, *hn, *h_next;
  int64_t R;
  int C;
};

template <int NCTP>
__global__ __launch_bounds__(256) void k_gg_round(Nbr g, RoundArgs p) {
  constexpr int CP = 32 * NCTP, RT = 128 / NCTP, KTW = 32 / NCTP, LDT = CP + 1, LDW = 6 * CP + 1;
  __shared__ float sU[RT * LDT];   // [row][c]: u = A h, then m = u W_l
  __shared__ float sH[RT * LDT];   // [row][c]: h_l
  __shared__ float sW[KTW * LDW];  // [k][block * CP + j]
  const int C = p.C;
  const int64_t row0 = (int64_t)blockIdx.x * RT;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int ct = wave % NCTP, strip = wave / NCTP;
  const bool active = ct * 32 < C;

  {  // (1) the neighbour sum and the tile of h
    const int grp = threadIdx.x >> 5, gl = threadIdx.x & 31;
    constexpr int RQ = RT / 8;  // rows of a lane group
    const int64_t rlast = (row0 + RT < p.R ? row0 + RT : p.R) - 1;
    // dense, all rows in one graph: neighbours in tiles of 32 = one word of the image.  Lane t of a group loads adj's
    // value of neighbour t of the tile when its bit is set (one coalesced, predicated load per row and word, every
    // row's in flight together); a tile no row of the workgroup has a bit in is skipped; otherwise h of the 32
    // neighbours is staged in the weights' LDS, [neighbour][channel], and each group walks its rows' set bits
    if (!g.sparse && row0 / g.N == rlast / g.N) {
      float* sN = sW;
      const int i0 = (int)(row0 % g.N);
      const size_t rb = (size_t)(row0 - i0);
      float acc[RQ][NCTP];
#pragma unroll
      for (int q = 0; q < RQ; ++q)
#pragma unroll
        for (int ch = 0; ch < NCTP; ++ch) acc[q][ch] = 0.f;
      for (int w = 0; w < g.W; ++w) {
        unsigned word[RQ], any = 0u;
        float av[RQ];
#pragma unroll
        for (int q = 0; q < RQ; ++q) {
          const int64_t r = row0 + grp + 8 * q;
          word[q] = r < p.R ? g.bits[(size_t)r * g.W + w] : 0u;
          any |= word[q];
        }
#pragma unroll
        for (int q = 0; q < RQ; ++q) {
          const int64_t r = row0 + grp + 8 * q;
          const int j = w * 32 + gl;
          av[q] = 0.f;
          if ((word[q] >> gl) & 1u)
            av[q] = (g.add_loop && j == i0 + grp + 8 * q) ? 1.f : g.adj[(size_t)r * g.N + j];
        }
        if (!__syncthreads_or(any != 0u)) continue;  // also: the previous tile is consumed
        for (int e = threadIdx.x; e < 32 * CP; e += 256) {
          const int t = e / CP, c = e % CP;
          const int j = w * 32 + t;
          sN[e] = (j < g.N && c < C) ? p.h[(rb + j) * C + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RQ; ++q) {
          unsigned m = word[q];
          while (m) {
            const int t = __ffs(m) - 1;
            m &= m - 1u;
            const float a = __shfl(av[q], t, 32);
#pragma unroll
            for (int ch = 0; ch < NCTP; ++ch) acc[q][ch] = fmaf(a, sN[t * CP + gl + 32 * ch], acc[q][ch]);
          }
        }
      }
#pragma unroll
      for (int q = 0; q < RQ; ++q) {
        const int rr = grp + 8 * q;
        const int64_t r = row0 + rr;
#pragma unroll
        for (int ch = 0; ch < NCTP; ++ch) {
          const int c = gl + 32 * ch;
          sU[rr * LDT + c] = acc[q][ch];
          sH[rr * LDT + c] = (r < p.R && c < C) ? p.h[(size_t)r * C + c] : 0.f;
        }
      }
    } else {
      for (int rr = grp; rr < RT; rr += 8) {
        const int64_t r = row0 + rr;
        float acc[NCTP], hv[NCTP];
#pragma unroll
        for (int ch = 0; ch < NCTP; ++ch) acc[ch] = hv[ch] = 0.f;
        if (r < p.R) {
          gg_nbr_sum<NCTP>(g, r, p.h, C, gl, acc);
#pragma unroll
          for (int ch = 0; ch < NCTP; ++ch) {
            const int c = gl + 32 * ch;
            if (c < C) hv[ch] = p.h[(size_t)r * C + c];
          }
        }
#pragma unroll
        for (int ch = 0; ch < NCTP; ++ch) {
          sU[rr * LDT + gl + 32 * ch] = acc[ch];
          sH[rr * LDT + gl + 32 * ch] = hv[ch];
        }
      }
    }
  }
  __syncthreads();

  {  // (2) m = u W_l   (B(k, j) = w_l[k, j])
    f32x16 am;
#pragma unroll
    for (int r = 0; r < 16; ++r) am[r] = 0.f;
    for (int k0 = 0; k0 < C; k0 += KTW) {
      for (int e = threadIdx.x; e < KTW * CP; e += 256) {
        const int k = e / CP, j = e % CP;
        const int gk = k0 + k;
        sW[k * LDW + j] = (gk < C && j < C) ? p.w_l[(size_t)gk * C + j] : 0.f;
      }
      __syncthreads();
      if (active) mma32(am, sU + strip * 32 * LDT + k0, LDT, 1, sW + ct * 32, LDW, 1, KTW, li, lh);
      __syncthreads();
    }
    if (active) {
      const int c = ct * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = strip * 32 + acc_row(r, lh);
        sU[i * LDT + c] = am[r];  // 0 for c >= C: w_l is staged zero-padded
        const int64_t row = row0 + i;
        if (row < p.R && c < C) p.m[(size_t)row * C + c] = am[r];
      }
    }
  }
  __syncthreads();

  // (3) the gate products: r and z accumulate gi + gh, n keeps the two apart
  f32x16 ar, az, ain, ahn;
#pragma unroll
  for (int r = 0; r < 16; ++r) ar[r] = az[r] = ain[r] = ahn[r] = 0.f;
  for (int k0 = 0; k0 < C; k0 += KTW) {
    for (int e = threadIdx.x; e < KTW * 6 * CP; e += 256) {
      const int k = e % KTW, q = e / KTW;
      const int blk = q / CP, j = q % CP;
      const int gk = k0 + k;
      const float* w = blk < 3 ? p.w_ih : p.w_hh;
      sW[k * LDW + q] = (gk < C && j < C) ? w[((size_t)(blk % 3) * C + j) * C + gk] : 0.f;
    }
    __syncthreads();
    if (active) {
      const float* am_ = sU + strip * 32 * LDT + k0;
      const float* ah_ = sH + strip * 32 * LDT + k0;
      const float* b = sW + ct * 32;
      mma32(ar, am_, LDT, 1, b, LDW, 1, KTW, li, lh);
      mma32(ar, ah_, LDT, 1, b + 3 * CP, LDW, 1, KTW, li, lh);
      mma32(az, am_, LDT, 1, b + CP, LDW, 1, KTW, li, lh);
      mma32(az, ah_, LDT, 1, b + 4 * CP, LDW, 1, KTW, li, lh);
      mma32(ain, am_, LDT, 1, b + 2 * CP, LDW, 1, KTW, li, lh);
      mma32(ahn, ah_, LDT, 1, b + 5 * CP, LDW, 1, KTW, li, lh);
    }
    __syncthreads();
  }

  // (4) the GRU
  const int c = ct * 32 + li;
  if (!active || c >= C) return;
  // in double from the fp32 accumulators, rounded once per stored value: the gates and the new state are the
  // correctly rounded fp32 values of their formulas, not three or four roundings away from them
  double br = 0.0, bz = 0.0, bin = 0.0, bhn = 0.0;
  if (p.b_ih) br += p.b_ih[c], bz += p.b_ih[C + c], bin = p.b_ih[2 * C + c];
  if (p.b_hh) br += p.b_hh[c], bz += p.b_hh[C + c], bhn = p.b_hh[2 * C + c];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = strip * 32 + acc_row(r, lh);
    const int64_t row = row0 + i;
    if (row >= p.R) continue;
    const size_t o = (size_t)row * C + c;
    const double hv = sH[i * LDT + c];
    const double rg = gg_sigmoid(ar[r] + br);
    const double zg = gg_sigmoid(az[r] + bz);
    const double hn = ahn[r] + bhn;
    const double ng = tanh(ain[r] + bin + rg * hn);
    p.rg[o] = (float)rg, p.zg[o] = (float)zg, p.ng[o] = (float)ng, p.hn[o] = (float)hn;
    p.h_next[o] = (float)((1.0 - zg) * ng + zg * hv);
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// G[row, :] = [g_r | g_z | g_n | g_n r]: the adjoints of the gates' arguments
__global__ __launch_bounds__(256) void k_gg_bwd_point(const float* __restrict__ gh, const float* __restrict__ h,
                                                      const float* __restrict__ rg, const float* __restrict__ zg,
                                                      const float* __restrict__ ng, const float* __restrict__ hn,
                                                      float* __restrict__ G, int64_t R, int C) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= R * C) return;
  const int64_t row = t / C;
  const int c = (int)(t - row * C);
  const double g = gh[t], r = rg[t], z = zg[t], n = ng[t];  // products in double, each adjoint rounded once
  const double gnp = g * (1.0 - z) * (1.0 - n * n);
  const double gzp = g * ((double)h[t] - n) * z * (1.0 - z);
  const double grp = gnp * (double)hn[t] * r * (1.0 - r);
  float* o = G + (size_t)row * 4 * C + c;
  o[0] = (float)grp, o[C] = (float)gzp, o[2 * C] = (float)gnp, o[3 * C] = (float)(gnp * r);
}

// C(b, i, j) = sum_k A(b, i, col(k)) B(b, k, j) + add(b, i, j) mul(b, i, j);  col(k) = k < a_split ? k : k + a_skip;
// add / mul in C's layout (add may be C itself: every element is read and written by one thread)
struct GgMm {
  const float* A;
  int64_t a_bs;
  int lda, a_split, a_skip;
  const float* B;
  int64_t b_bs, b_ks, b_js;
  float* C;
  int64_t c_bs;
  int ldc;
  const float *add, *mul;
  int M, N, K, zero_diag;
};

template <int NCT>
__global__ __launch_bounds__(256) void k_gg_mm(GgMm p) {
  __shared__ float sA[MB * (KT + 1)];        // [i][k]
  __shared__ float sB[KT * (32 * NCT + 1)];  // [k][j]
  const int b = blockIdx.z;
  const int i0 = blockIdx.x * MB, j0 = blockIdx.y * 32 * NCT;
  const TileLane t = tile_lane();
  const float* Ab = p.A + (size_t)b * p.a_bs;
  const float* Bb = p.B + (size_t)b * p.b_bs;
  const bool b_kfast = p.b_ks == 1 && p.b_js != 1;
  f32x16 acc[NCT];
  tile_zero(acc);
  tile_mma<NCT, false>(
      acc, t, sA, sB, i0, j0, p.M, p.N, 0, p.K, false, b_kfast,
      [=](int gi, int gk) { return Ab[(size_t)gi * p.lda + (gk < p.a_split ? gk : gk + p.a_skip)]; },
      [=](int gk, int gj) { return Bb[(size_t)gk * p.b_ks + (size_t)gj * p.b_js]; });
  const size_t cb = (size_t)b * p.c_bs;
  tile_store(acc, t, i0, j0, p.M, p.N, [=](int j) {
    return [=](int i, float v) {
      const size_t off = cb + (size_t)i * p.ldc + j;
      if (p.add) v = p.mul ? fmaf(p.add[off], p.mul[off], v) : v + p.add[off];
      if (p.zero_diag && i == j) v = 0.f;
      p.C[off] = v;
    };
  });
}

GgMm gg_mm_args() {
  GgMm p = {};
  p.a_split = 1 << 30;
  return p;
}

int gg_launch_mm(const GgMm& p, int batch, hipStream_t s) {
  const int nct = nct_of(p.N);
  const dim3 grid(blocks(p.M, MB), blocks(p.N, 32 * nct), batch);
  dispatch_nct(nct, [&](auto n) { hipLaunchKernelGGL(k_gg_mm<n()>, grid, dim3(256), 0, s, p); });
  return gcm_launch_status();
}

// out[r, :] = sum over the neighbours of r of a src[nbr, :]; a group of 32 lanes per row
template <int NCH>
__global__ __launch_bounds__(256) void k_gg_sweep(Nbr g, const float* __restrict__ src, float* __restrict__ out,
                                                  int64_t R, int C) {
  const int64_t r = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (r >= R) return;
  const int gl = threadIdx.x & 31;
  float acc[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) acc[ch] = 0.f;
  gg_nbr_sum<NCH>(g, r, src, C, gl, acc);
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + 32 * ch;
    if (c < C) out[(size_t)r * C + c] = acc[ch];
  }
}

// g_ew[e] (+)= <g_m[i, :], p[col[e], :]> for the entries e of CSR row i; a group of 32 lanes per row
__global__ __launch_bounds__(256) void k_gg_edge_grad(const int64_t* __restrict__ row_ptr,
                                                      const int64_t* __restrict__ col, const float* __restrict__ gm,
                                                      const float* __restrict__ pj, float* __restrict__ g_ew,
                                                      int64_t M, int C, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (i >= M) return;
  const int gl = threadIdx.x & 31;
  const int64_t e1 = row_ptr[i + 1];
  for (int64_t e = row_ptr[i]; e < e1; ++e) {
    const float* s = pj + (size_t)col[e] * C;
    float d = 0.f;
    for (int c = gl; c < C; c += 32) d = fmaf(gm[(size_t)i * C + c], s[c], d);
    d = group_sum<32>(d);
    if (gl == 0) g_ew[e] = accumulate ? g_ew[e] + d : d;
  }
}

// the column sums of G = [g_r | g_z | g_n | g_n r] -> g_b_ih = blocks 0, 1, 2; g_b_hh = blocks 0, 1, 3
__global__ __launch_bounds__(256) void k_gg_bias_split(const float* __restrict__ sums, float* __restrict__ g_b_ih,
                                                       float* __restrict__ g_b_hh, int C) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 3 * C) return;
  if (g_b_ih) g_b_ih[t] = sums[t];
  if (g_b_hh) g_b_hh[t] = sums[t < 2 * C ? t : t + C];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool gg_unsupported(int64_t R, int C, int L) { return C > 128 || R > (1 << 30) || (int64_t)L * R > (1 << 30); }

// `saved`: [SLOTS][L][R][C] floats (h_l, m_l, r, z, n, gh_n per round), then the bit image (dense)
size_t gg_slot(int slot, int l, int L, int64_t R, int C) { return ((size_t)slot * L + l) * (size_t)R * C; }
size_t gg_saved_bytes(int64_t R, int C, int L, int64_t bit_words) {
  return ((size_t)SLOTS * L * R * C + (size_t)bit_words) * 4;
}

constexpr int WL_BATCH = 64;  // rounds per launch of the g_weight product (grid.z = rounds x splits <= 65535)

struct BwdWs {
  size_t G, gP, gM, gHa, gHb, P, sums, bitsT, slabs, total;
};
BwdWs gg_bwd_ws(int64_t R, int C, int L, int64_t bit_words) {
  BwdWs w;
  const size_t RC = (size_t)R * C * 4;
  int nsK, nsR, kc;
  wgrad_split64((int64_t)L * R, &nsK, &kc);
  wgrad_split64(R, &nsR, &kc);
  size_t slab_f = (size_t)nsK * 3 * C * C;
  slab_f = std::max(slab_f, (size_t)std::min(L, WL_BATCH) * nsR * C * C);
  slab_f = std::max(slab_f, (size_t)colsum_slabs((int64_t)L * R) * 4 * C);
  Carve c;
  w.G = c.take((size_t)L * R * 4 * C * 4), w.gP = c.take((size_t)L * R * C * 4);
  w.gM = c.take(RC), w.gHa = c.take(RC), w.gHb = c.take(RC), w.P = c.take(RC);
  w.sums = c.take((size_t)4 * C * 4), w.bitsT = c.take((size_t)bit_words * 4), w.slabs = c.take(slab_f * 4);
  w.total = c.at;
  return w;
}

#define GG_BY_WIDTH(C, CALL) \
  if ((C) <= 32) { CALL(1) } else if ((C) <= 64) { CALL(2) } else { CALL(4) }

int gg_forward(const Nbr& g, const float* x, const float* weight, const float* w_ih, const float* w_hh,
               const float* b_ih, const float* b_hh, float* out, float* sv, int64_t R, int Fi, int C, int L,
               hipStream_t s) {
  hipLaunchKernelGGL(k_gg_pad, dim3(blocks(R * C, 256)), dim3(256), 0, s, x, sv + gg_slot(SLOT_H, 0, L, R, C), R, Fi,
                     C);
  int rc = gcm_launch_status();
  if (rc) return rc;
  for (int l = 0; l < L; ++l) {
    RoundArgs p;
    p.h = sv + gg_slot(SLOT_H, l, L, R, C);
    p.w_l = weight + (size_t)l * C * C, p.w_ih = w_ih, p.w_hh = w_hh, p.b_ih = b_ih, p.b_hh = b_hh;
    p.m = sv + gg_slot(SLOT_M, l, L, R, C), p.rg = sv + gg_slot(SLOT_R, l, L, R, C);
    p.zg = sv + gg_slot(SLOT_Z, l, L, R, C), p.ng = sv + gg_slot(SLOT_N, l, L, R, C);
    p.hn = sv + gg_slot(SLOT_HN, l, L, R, C);
    p.h_next = l + 1 < L ? sv + gg_slot(SLOT_H, l + 1, L, R, C) : out;
    p.R = R, p.C = C;
#define GG_ROUND(T) hipLaunchKernelGGL(k_gg_round<T>, dim3(blocks(R, 128 / T)), dim3(256), 0, s, g, p);
    GG_BY_WIDTH(C, GG_ROUND)
#undef GG_ROUND
    if ((rc = gcm_launch_status())) return rc;
  }
  return GCM_OK;
}

struct BwdOut {
  float *g_x, *g_weight, *g_w_ih, *g_w_hh, *g_b_ih, *g_b_hh, *g_adj, *g_ew;
};

// gt: the transposed neighbourhood (g_p = A^T g_m); row_ptr / col: the CSR, for g_ew; B, N: dense, for g_adj
int gg_backward(const Nbr& gt, const int64_t* row_ptr, const int64_t* col, const float* g_out, const float* weight,
                const float* w_ih, const float* w_hh, const float* sv, const BwdOut& o, char* ws, const BwdWs& K,
                int64_t R, int B, int N, int Fi, int C, int L, int add_loop, hipStream_t s) {
  float* G = (float*)(ws + K.G);
  float* gP = (float*)(ws + K.gP);
  float* gM = (float*)(ws + K.gM);
  float* gHbuf[2] = {(float*)(ws + K.gHa), (float*)(ws + K.gHb)};
  float* P = (float*)(ws + K.P);
  float* sums = (float*)(ws + K.sums);
  float* slabs = (float*)(ws + K.slabs);
  const size_t RC = (size_t)R * C;
  const float* gh = g_out;
  int rc, flip = 0;
  bool first_adj = true;
  for (int l = L - 1; l >= 0; --l) {
    const float* h_l = sv + gg_slot(SLOT_H, l, L, R, C);
    const float* z_l = sv + gg_slot(SLOT_Z, l, L, R, C);
    const float* w_l = weight + (size_t)l * C * C;
    float* G_l = G + (size_t)l * R * 4 * C;
    float* gP_l = gP + (size_t)l * RC;
    float* gh_new = gHbuf[flip];
    flip ^= 1;
    hipLaunchKernelGGL(k_gg_bwd_point, dim3(blocks(R * C, 256)), dim3(256), 0, s, gh, h_l,
                       sv + gg_slot(SLOT_R, l, L, R, C), z_l, sv + gg_slot(SLOT_N, l, L, R, C),
                       sv + gg_slot(SLOT_HN, l, L, R, C), G_l, R, C);
    if ((rc = gcm_launch_status())) return rc;
    GgMm p = gg_mm_args();  // g_m = G_gi W_ih
    p.A = G_l, p.lda = 4 * C;
    p.B = w_ih, p.b_ks = C, p.b_js = 1;
    p.C = gM, p.ldc = C;
    p.M = (int)R, p.N = C, p.K = 3 * C;
    if ((rc = gg_launch_mm(p, 1, s))) return rc;
    p.a_split = 2 * C, p.a_skip = C;  // g_h = g_h' z + G_gh W_hh
    p.B = w_hh;
    p.C = gh_new, p.add = gh, p.mul = z_l;
    if ((rc = gg_launch_mm(p, 1, s))) return rc;
#define GG_SWEEP(T) hipLaunchKernelGGL(k_gg_sweep<T>, dim3(blocks(R, 8)), dim3(256), 0, s, gt, (const float*)gM, gP_l, R, C);
    GG_BY_WIDTH(C, GG_SWEEP)  // g_p = A^T g_m
#undef GG_SWEEP
    if ((rc = gcm_launch_status())) return rc;
    p = gg_mm_args();  // g_h += g_p W_l^T
    p.A = gP_l, p.lda = C;
    p.B = w_l, p.b_ks = 1, p.b_js = C;
    p.C = gh_new, p.ldc = C, p.add = gh_new;
    p.M = (int)R, p.N = C, p.K = C;
    if ((rc = gg_launch_mm(p, 1, s))) return rc;
    if (o.g_adj || o.g_ew) {
      p = gg_mm_args();  // p_l = h_l W_l
      p.A = h_l, p.lda = C;
      p.B = w_l, p.b_ks = C, p.b_js = 1;
      p.C = P, p.ldc = C;
      p.M = (int)R, p.N = C, p.K = C;
      if ((rc = gg_launch_mm(p, 1, s))) return rc;
      if (o.g_adj) {  // g_adj[b] (+)= g_m[b] p_l[b]^T
        p = gg_mm_args();
        p.A = gM, p.a_bs = (int64_t)N * C, p.lda = C;
        p.B = P, p.b_bs = (int64_t)N * C, p.b_ks = 1, p.b_js = C;
        p.C = o.g_adj, p.c_bs = (int64_t)N * N, p.ldc = N;
        p.add = first_adj ? nullptr : o.g_adj;
        p.M = N, p.N = N, p.K = C, p.zero_diag = add_loop;
        if ((rc = gg_launch_mm(p, B, s))) return rc;
      } else {
        hipLaunchKernelGGL(k_gg_edge_grad, dim3(blocks(R, 8)), dim3(256), 0, s, row_ptr, col, (const float*)gM,
                           (const float*)P, o.g_ew, R, C, first_adj ? 0 : 1);
        if ((rc = gcm_launch_status())) return rc;
      }
      first_adj = false;
    }
    gh = gh_new;
  }
  if (o.g_x) {
    hipLaunchKernelGGL(k_gg_unpad, dim3(blocks(R * Fi, 256)), dim3(256), 0, s, gh, o.g_x, R, Fi, C);
    if ((rc = gcm_launch_status())) return rc;
  }
  const int64_t LR = (int64_t)L * R;
  const float* h_all = sv + gg_slot(SLOT_H, 0, L, R, C);
  const float* m_all = sv + gg_slot(SLOT_M, 0, L, R, C);
  int ns, kc;
  wgrad_split64(LR, &ns, &kc);
  // g_w[rows, :] = sum over all L R rows of G[:, col0 + rows]^T y
  auto wgrad = [&](int col0, int rows, const float* y, float* g) -> int {
    MmArgs q = mm_args();
    q.A = G + col0, q.a_is = 1, q.a_ks = 4 * C;
    q.B = y, q.b_ks = C, q.b_js = 1;
    q.C = slabs, q.c_is = C, q.c_js = 1, q.c_ss = (int64_t)rows * C;
    q.M = rows, q.N = C, q.K = (int)LR, q.kchunk = kc;
    const int e = launch_mm(q, ns, s);
    return e ? e : gcm_sum_slabs(slabs, ns, rows * C, g, s);
  };
  if (o.g_w_ih && (rc = wgrad(0, 3 * C, m_all, o.g_w_ih))) return rc;
  if (o.g_w_hh) {
    if ((rc = wgrad(0, 2 * C, h_all, o.g_w_hh))) return rc;
    if ((rc = wgrad(3 * C, C, h_all, o.g_w_hh + (size_t)2 * C * C))) return rc;
  }
  if (o.g_weight) {  // g_weight[l] = h_l^T g_p_l, the rounds batched
    wgrad_split64(R, &ns, &kc);
    for (int l0 = 0; l0 < L; l0 += WL_BATCH) {
      const int nb = std::min(WL_BATCH, L - l0);
      MmArgs q = mm_args();
      q.A = h_all + (size_t)l0 * RC, q.a_bs = (int64_t)RC, q.a_is = 1, q.a_ks = C;
      q.B = gP + (size_t)l0 * RC, q.b_bs = (int64_t)RC, q.b_ks = C, q.b_js = 1;
      q.C = slabs, q.c_bs = (int64_t)C * C, q.c_is = C, q.c_js = 1, q.c_ss = (int64_t)nb * C * C;
      q.M = C, q.N = C, q.K = (int)R, q.kchunk = kc, q.batch = nb;
      if ((rc = launch_mm(q, ns, s))) return rc;
      if ((rc = gcm_sum_slabs(slabs, ns, nb * C * C, o.g_weight + (size_t)l0 * C * C, s))) return rc;
    }
  }
  if (o.g_b_ih || o.g_b_hh) {
    if ((rc = colsum(G, LR, 4 * C, sums, slabs, s))) return rc;
    hipLaunchKernelGGL(k_gg_bias_split, dim3(blocks(3 * C, 256)), dim3(256), 0, s, (const float*)sums, o.g_b_ih,
                       o.g_b_hh, C);
    if ((rc = gcm_launch_status())) return rc;
  }
  return GCM_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: DenseGatedGraphConv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_dense_gatedgraphconv_fwd_workspace_bytes(int B, int N, int C, int L) {
  if (B <= 0 || N <= 0 || C <= 0 || L <= 0) return 0;
  const int64_t R = (int64_t)B * N;
  return gg_saved_bytes(R, C, L, R * ((N + 31) / 32));
}

extern "C" int gcm_dense_gatedgraphconv_fwd(const float* x, const float* adj, const float* weight, const float* w_ih,
                                            const float* w_hh, const float* b_ih, const float* b_hh, float* out,
                                            void* saved, size_t saved_bytes, int B, int N, int Fi, int C, int L,
                                            int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && weight && w_ih && w_hh && out && saved);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && C > 0 && L > 0 && Fi <= C);
  const int64_t R = (int64_t)B * N;
  if (gg_unsupported(R, C, L) || B > 65535) return GCM_EUNSUPPORTED;
  const int W = (N + 31) / 32;
  GCM_REQUIRE(saved_bytes >= gg_saved_bytes(R, C, L, R * W));
  hipStream_t s = (hipStream_t)stream;
  float* sv = (float*)saved;
  unsigned* bits = (unsigned*)(sv + (size_t)SLOTS * L * R * C);
  const int rc = mask_bits(adj, bits, R, N, W, add_loop, s);
  if (rc) return rc;
  Nbr g = {};
  g.bits = bits, g.adj = adj, g.N = N, g.W = W, g.add_loop = add_loop;
  return gg_forward(g, x, weight, w_ih, w_hh, b_ih, b_hh, out, sv, R, Fi, C, L, s);
}

extern "C" size_t gcm_dense_gatedgraphconv_bwd_workspace_bytes(int B, int N, int C, int L) {
  if (B <= 0 || N <= 0 || C <= 0 || L <= 0) return 0;
  const int64_t R = (int64_t)B * N;
  return gg_bwd_ws(R, C, L, R * ((N + 31) / 32)).total;
}

extern "C" int gcm_dense_gatedgraphconv_bwd(const float* g_out, const float* adj, const float* weight,
                                            const float* w_ih, const float* w_hh, const void* saved, float* g_x,
                                            float* g_weight, float* g_w_ih, float* g_w_hh, float* g_b_ih,
                                            float* g_b_hh, float* g_adj, void* workspace, size_t workspace_bytes,
                                            int B, int N, int Fi, int C, int L, int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && adj && weight && w_ih && w_hh && saved && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && C > 0 && L > 0 && Fi <= C);
  const int64_t R = (int64_t)B * N;
  if (gg_unsupported(R, C, L) || B > 65535) return GCM_EUNSUPPORTED;
  const int W = (N + 31) / 32;
  const BwdWs K = gg_bwd_ws(R, C, L, R * W);
  GCM_REQUIRE(workspace_bytes >= K.total);
  if (!g_x && !g_weight && !g_w_ih && !g_w_hh && !g_b_ih && !g_b_hh && !g_adj) return GCM_OK;
  hipStream_t s = (hipStream_t)stream;
  const float* sv = (const float*)saved;
  const unsigned* bits = (const unsigned*)(sv + (size_t)SLOTS * L * R * C);
  unsigned* bitsT = (unsigned*)((char*)workspace + K.bitsT);
  const int rc = mask_bits_t(bits, bitsT, R, N, W, s);
  if (rc) return rc;
  Nbr gt = {};
  gt.bits = bitsT, gt.adj = adj, gt.N = N, gt.W = W, gt.add_loop = add_loop, gt.tr = 1;
  const BwdOut o = {g_x, g_weight, g_w_ih, g_w_hh, g_b_ih, g_b_hh, g_adj, nullptr};
  return gg_backward(gt, nullptr, nullptr, g_out, weight, w_ih, w_hh, sv, o, (char*)workspace, K, R, B, N, Fi, C, L,
                     add_loop, s);
}

// ---------------------------------------------------------------------------
// C ABI: GatedGraphConv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_csr_gatedgraphconv_fwd_workspace_bytes(int64_t M, int64_t E, int C, int L) {
  if (M <= 0 || E < 0 || C <= 0 || L <= 0) return 0;
  return gg_saved_bytes(M, C, L, 0);
}

extern "C" int gcm_csr_gatedgraphconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col,
                                          const float* edge_weight, const float* weight, const float* w_ih,
                                          const float* w_hh, const float* b_ih, const float* b_hh, float* out,
                                          void* saved, size_t saved_bytes, int64_t M, int64_t E, int Fi, int C, int L,
                                          gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && weight && w_ih && w_hh && out && saved);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && C > 0 && L > 0 && Fi <= C);
  GCM_REQUIRE(E == 0 || col);
  if (gg_unsupported(M, C, L)) return GCM_EUNSUPPORTED;
  GCM_REQUIRE(saved_bytes >= gg_saved_bytes(M, C, L, 0));
  Nbr g = {};
  g.sparse = 1, g.ptr = E > 0 ? row_ptr : nullptr, g.idx = col, g.ew = edge_weight;
  return gg_forward(g, x, weight, w_ih, w_hh, b_ih, b_hh, out, (float*)saved, M, Fi, C, L, (hipStream_t)stream);
}

extern "C" size_t gcm_csr_gatedgraphconv_bwd_workspace_bytes(int64_t M, int64_t E, int C, int L) {
  if (M <= 0 || E < 0 || C <= 0 || L <= 0) return 0;
  return gg_bwd_ws(M, C, L, 0).total;
}

extern "C" int gcm_csr_gatedgraphconv_bwd(const float* g_out, const int64_t* row_ptr, const int64_t* col,
                                          const int64_t* col_ptr, const int64_t* rows, const int64_t* perm,
                                          const float* edge_weight, const float* weight, const float* w_ih,
                                          const float* w_hh, const void* saved, float* g_x, float* g_weight,
                                          float* g_w_ih, float* g_w_hh, float* g_b_ih, float* g_b_hh,
                                          float* g_edge_weight, void* workspace, size_t workspace_bytes, int64_t M,
                                          int64_t E, int Fi, int C, int L, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && row_ptr && weight && w_ih && w_hh && saved && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && C > 0 && L > 0 && Fi <= C);
  GCM_REQUIRE(E == 0 || (col && col_ptr && rows));
  GCM_REQUIRE(E == 0 || !edge_weight || perm);
  GCM_REQUIRE(!g_edge_weight || edge_weight);
  if (gg_unsupported(M, C, L)) return GCM_EUNSUPPORTED;
  const BwdWs K = gg_bwd_ws(M, C, L, 0);
  GCM_REQUIRE(workspace_bytes >= K.total);
  if (!g_x && !g_weight && !g_w_ih && !g_w_hh && !g_b_ih && !g_b_hh && !g_edge_weight) return GCM_OK;
  Nbr gt = {};
  gt.sparse = 1, gt.ptr = E > 0 ? col_ptr : nullptr, gt.idx = rows, gt.eperm = perm, gt.ew = edge_weight;
  const BwdOut o = {g_x, g_weight, g_w_ih, g_w_hh, g_b_ih, g_b_hh, nullptr, E > 0 ? g_edge_weight : nullptr};
  return gg_backward(gt, row_ptr, col, g_out, weight, w_ih, w_hh, (const float*)saved, o, (char*)workspace, K, M, 1, 0,
                     Fi, C, L, 0, (hipStream_t)stream);
}
