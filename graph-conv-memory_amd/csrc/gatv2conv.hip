// GATv2Conv / DenseGATv2Conv (PyG's GATv2Conv with edge_dim, and a dense twin) forward and backward on gfx950.
//
//   x_l = x W_l^T + b_l,  x_r = x W_r^T + b_r  viewed [rows, H, C]  (shared weights: x_r = x_l)
//   term k = (j -> i):  z_k = x_l[j] + x_r[i] (+ W_e a_k),  s_k[h] = sum_c att[h,c] leaky_relu(z_k[h,c])
//   alpha = softmax of s over the terms of i,  o[i,h,:] = sum_k alpha_k[h] x_l[j,h,:],  out = concat / mean_h + bias
//
// Unlike GAT v1 the score does not split into a per-source and a per-destination number: it is a length-C dot product
// through a nonlinearity per edge and head.  There is no contraction for the matrix cores in it, and written out it
// costs five [E, H*C] arrays (x_l[j], x_r[i], W_e a, z, the messages).  The kernels here write NOTHING per edge: an edge
// costs its index, its D features and the gathered row of x_l.  The forward keeps x_l, x_r and the softmax's per-row
// maximum and sum [rows, H]; the backward recomputes z, s and alpha from those, with the SAME device function
// (Gv2::score), so both passes see the same bits of s.
//
// Lanes and channels, as gineconv.hip: a group of G lanes owns a row (a destination in the row sweeps, a source in the
// column sweep); lane gl holds channel gl (and gl + 64 when H*C > 64) and ITS rows of W_e in registers (the template's
// DB = 0 without edge features, 4 or 32).  The D features of an edge are one address across the group: a broadcast
// read, reached through the index's permutation - edge_attr is never copied into another order.  The score of a head is
// a sum over the C lanes that hold it (Gv2::head_sum): a butterfly over C lanes when C is a power of two, the group sum
// when H == 1, else through the group's own words of LDS.  Every lane of a head ends with the same bits.
//
// forward, sparse  k_gv2_csr_fwd     a group walks its destination's CSR row ONCE with the online softmax: running
//                                    maximum, sum and aggregate are rescaled when the maximum moves.  i -> i entries are
//                                    skipped in place when loops are added, the sum of the features for a "mean" loop
//                                    comes from the same walk, and the loop is the row's last term.
// forward, dense   k_gv2_dense_fwd   the adjacency is read once into the bit image of its pattern (attn_bits.h).  A
//                                    workgroup takes 256 / G rows of a graph and sweeps the neighbours in tiles of 32 =
//                                    one word of the image: a tile none of its rows has a bit in is skipped, else
//                                    x_l of the 32 neighbours is staged in LDS and every row scores ITS set bits only.
//                                    alpha x_l runs on the vector ALU inside that loop: the scores cannot use the matrix
//                                    cores at all, a memory's patterns are sparse (cfg2's band: <= 4 of 128 entries),
//                                    and a 32x32x2 MFMA over the tile would multiply the zeros of the other 28 - 31.
// backward         k_gv2_drow        by destination, two walks of the row: delta_i = sum_k alpha_k dP_k from the
//                                    recomputed alpha (the same alpha on both sides of dP - delta: the note at the top
//                                    of gatconv.hip), then dS_k = alpha_k (dP_k - delta_i), dz_k = dS_k att
//                                    leaky_relu'(z_k): g_xr[i] = sum dz, g_edge_attr[k] = W_e^T dz_k (+ the mean loop's
//                                    share), and the lane's own sums for g_att and g_w_e, which leave as one partial per
//                                    workgroup and are summed in index order.  The loop term's share of g_xl[i] is
//                                    written here.
//                  k_gv2_dcol        by source over the CSC column (dense: the transposed image): recomputes the term
//                                    and adds alpha_k dO_i + dz_k into g_xl[j].
//                  One pair of kernels serves both layers: the sweeps are templates over where the entries of a row
//                  or column come from (CsrSrc / DenseSrc).
// x W^T, g_x = g_xl W_l + g_xr W_r and the weight gradients use the tile GEMM of gcn_mm.h, the bias gradients its
// column sum.  Nothing accumulates with atomics: every sum runs in a fixed order.  Fi, H*C <= 128, D <= 32; any N.
#include <cmath>

#include "attn_bits.h"  // GT, mask_bits, group_sum

namespace {

constexpr int GV2_PARTS = 2048;  // workgroups of the backward's row sweep, at most (8 per compute unit)

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// the features of one edge, as every lane of the group holds them
template <int DB>
struct Attr {
  float v[DB > 0 ? DB : 1];
  __device__ __forceinline__ void load(const float* __restrict__ a, int D) {
#pragma unroll
    for (int d = 0; d < DB; ++d) v[d] = d < D ? a[d] : 0.f;
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int d = 0; d < (DB > 0 ? DB : 1); ++d) v[d] = 0.f;
  }
  __device__ __forceinline__ void add(const Attr& o) {
#pragma unroll
    for (int d = 0; d < DB; ++d) v[d] += o.v[d];
  }
  // the loop term's features: the mean of the `cnt` summed ones (zero for none), or `fill` in each of the D columns
  __device__ __forceinline__ Attr loop(int cnt, int fill_mean, float fill, int D) const {
    Attr r;
    r.zero();
#pragma unroll
    for (int d = 0; d < DB; ++d)
      if (d < D) r.v[d] = fill_mean ? (cnt > 0 ? v[d] / (float)cnt : 0.f) : fill;
    return r;
  }
};

// What a lane keeps for its NCH channels: att, its rows of W_e, the head of each channel.
template <int G, int NCH, int DB>
struct Gv2 {
  float w[NCH][DB > 0 ? DB : 1], att[NCH];
  int hd[NCH];
  bool ok[NCH];
  int gl, C, HC, mode;
  float slope;
  volatile float* sT;  // the group's NCH * G words of LDS (mode 2)

  __device__ __forceinline__ void init(const float* __restrict__ att_, const float* __restrict__ w_e, float* lds, int H,
                                       int C_, int D, float slope_, int mode_) {
    gl = threadIdx.x % G, C = C_, HC = H * C_, mode = mode_, slope = slope_;
    sT = lds + (threadIdx.x / G) * (G * NCH);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      ok[ch] = c < HC;
      hd[ch] = ok[ch] ? c / C : 0;
      att[ch] = ok[ch] ? att_[c] : 0.f;
#pragma unroll
      for (int d = 0; d < DB; ++d) w[ch][d] = (ok[ch] && d < D) ? w_e[(size_t)c * D + d] : 0.f;
    }
  }

  // t[ch] := the sum of t over the channels of the head of the lane's channel ch (0 where the lane has no channel).
  // Every lane of the group must call it.  0: C a power of two <= G; 1: one head; 2: any C, through LDS.
  __device__ __forceinline__ void head_sum(float (&t)[NCH]) const {
    if (mode == 0) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        float v = t[ch];
#pragma unroll
        for (int off = 1; off < G; off <<= 1)
          if (off < C) v += __shfl_xor(v, off);  // uniform
        t[ch] = v;
      }
    } else if (mode == 1) {
      float v = t[0];
      if (NCH == 2) v += t[NCH - 1];
      v = group_sum<G>(v);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) t[ch] = v;
    } else {
      // a group is within one wave: its lanes run in lockstep and LDS serves a wave's accesses in order, so the
      // volatile stores of all lanes precede the loads below and those precede the next call's stores
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) sT[gl + ch * G] = t[ch];
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        float v = 0.f;
        if (ok[ch])
          for (int q = 0; q < C; ++q) v += sT[hd[ch] * C + q];
        t[ch] = v;
      }
    }
  }

  // z of a term and, per lane channel, the score of the channel's head
  __device__ __forceinline__ void score(const float (&xl)[NCH], const float (&xr)[NCH], const Attr<DB>& A,
                                        float (&z)[NCH], float (&s)[NCH]) const {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      float e = 0.f;
#pragma unroll
      for (int d = 0; d < DB; ++d) e = fmaf(w[ch][d], A.v[d], e);
      z[ch] = ok[ch] ? xl[ch] + xr[ch] + e : 0.f;
      s[ch] = att[ch] * lrelu(z[ch], slope);
    }
    head_sum(s);
  }

  // the lane's channels of row r of a [rows, H*C] array (0 where the lane has none)
  __device__ __forceinline__ void row(const float* __restrict__ src, int64_t r, float (&v)[NCH]) const {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) v[ch] = ok[ch] ? src[(size_t)r * HC + gl + ch * G] : 0.f;
  }
  // the lane's heads' entries of row r of a [rows, H] array
  __device__ __forceinline__ void stat(const float* __restrict__ src, int64_t r, float (&v)[NCH]) const {
    const int H = HC / C;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) v[ch] = src[(size_t)r * H + hd[ch]];
  }
};

// the online softmax of a row: running maximum, sum and aggregate per lane channel
template <int NCH>
struct Soft {
  float m[NCH], l[NCH], acc[NCH];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) m[ch] = -INFINITY, l[ch] = 0.f, acc[ch] = 0.f;
  }
  __device__ __forceinline__ void add(const float (&s)[NCH], const float (&xl)[NCH]) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const float mn = fmaxf(m[ch], s[ch]);
      const float sc = expf(m[ch] - mn);  // 0 at the first term (m = -inf)
      const float p = expf(s[ch] - mn);
      l[ch] = fmaf(l[ch], sc, p);
      acc[ch] = fmaf(acc[ch], sc, p * xl[ch]);
      m[ch] = mn;
    }
  }
};

// ---------------------------------------------------------------------------
// where the entries of a row (by destination) or a column (by source) come from.  next(): the other end of the next
// entry as a row of x_l / x_r, and the entry's position in edge_attr.
// ---------------------------------------------------------------------------
struct CsrIt {
  const int64_t* idx;
  const int64_t* perm;
  int64_t p, p1;
  __device__ __forceinline__ bool next(int64_t& other, int64_t& k) {
    if (p >= p1) return false;
    other = idx[p];
    k = perm ? perm[p] : p;
    ++p;
    return true;
  }
};

struct CsrSrc {
  const int64_t *row_ptr, *col, *csr_perm;  // row_ptr NULL: no entries
  const int64_t *col_ptr, *rows, *csc_perm;
  __device__ __forceinline__ CsrIt row(int64_t i) const {
    return row_ptr ? CsrIt{col, csr_perm, row_ptr[i], row_ptr[i + 1]} : CsrIt{nullptr, nullptr, 0, 0};
  }
  __device__ __forceinline__ CsrIt column(int64_t j) const {
    return col_ptr ? CsrIt{rows, csc_perm, col_ptr[j], col_ptr[j + 1]} : CsrIt{nullptr, nullptr, 0, 0};
  }
};

struct BitIt {
  const unsigned* words;
  int W, w;
  unsigned m;
  int64_t rb, N, loc;
  bool transposed;
  __device__ __forceinline__ bool next(int64_t& other, int64_t& k) {
    while (!m) {
      if (++w >= W) return false;
      m = words[w];
    }
    const int o = w * 32 + __ffs(m) - 1;
    m &= m - 1u;
    other = rb + o;
    k = transposed ? (rb + o) * N + loc : (rb + loc) * N + o;
    return true;
  }
};

struct DenseSrc {
  const unsigned *bits, *bitsT;  // [B, N, W]; bit t of word w of row i: adj[b, i, 32 w + t] != 0 (bitsT: adj[b, 32 w + t, i])
  int N, W;
  __device__ __forceinline__ BitIt make(const unsigned* img, int64_t r, bool t) const {
    const int64_t loc = r % N;
    return BitIt{img + (size_t)r * W, W, -1, 0u, r - loc, N, loc, t};
  }
  __device__ __forceinline__ BitIt row(int64_t i) const { return make(bits, i, false); }
  __device__ __forceinline__ BitIt column(int64_t j) const { return make(bitsT, j, true); }
};

// the end of a forward row: o = acc / l (0 for a row without a term), the statistics, out
template <int G, int NCH, int DB>
__device__ __forceinline__ void gv2_fwd_finish(const Gv2<G, NCH, DB>& g, const Soft<NCH>& sm, int64_t i,
                                               const float* __restrict__ bias, float* __restrict__ out,
                                               float* __restrict__ row_m, float* __restrict__ row_l, int concat) {
  const int H = g.HC / g.C;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = g.gl + ch * G;
    if (!g.ok[ch]) continue;
    float v = sm.l[ch] > 0.f ? sm.acc[ch] / sm.l[ch] : 0.f;
    if (concat && bias) v += bias[c];
    out[(size_t)i * g.HC + c] = v;  // !concat: the per-head aggregate, k_gv2_heads finishes
    if (c == g.hd[ch] * g.C) row_m[(size_t)i * H + g.hd[ch]] = sm.m[ch], row_l[(size_t)i * H + g.hd[ch]] = sm.l[ch];
  }
}

// ---------------------------------------------------------------------------
// forward, sparse: a group per destination, one walk of its CSR row
// ---------------------------------------------------------------------------
template <int G, int NCH, int DB, class Src>
__global__ __launch_bounds__(256) void k_gv2_csr_fwd(Src src, const float* __restrict__ xl,
                                                     const float* __restrict__ xr, const float* __restrict__ ea,
                                                     const float* __restrict__ w_e, const float* __restrict__ att,
                                                     const float* __restrict__ bias, float* __restrict__ out,
                                                     float* __restrict__ row_m, float* __restrict__ row_l, int64_t M,
                                                     int H, int C, int D, int concat, int loops, int fill_mean,
                                                     float fill, float slope, int mode) {
  __shared__ float sT[256 * NCH];
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (i >= M) return;
  Gv2<G, NCH, DB> g;
  g.init(att, w_e, sT, H, C, D, slope, mode);
  float xri[NCH], xlj[NCH], z[NCH], s[NCH];
  g.row(xr, i, xri);
  Soft<NCH> sm;
  sm.init();
  Attr<DB> A, asum;
  A.zero(), asum.zero();
  int cnt = 0;
  auto it = src.row(i);
  int64_t j, k;
  while (it.next(j, k)) {
    if (loops && j == i) continue;
    if (DB > 0) {
      A.load(ea + (size_t)k * D, D);
      if (fill_mean) asum.add(A), ++cnt;
    }
    g.row(xl, j, xlj);
    g.score(xlj, xri, A, z, s);
    sm.add(s, xlj);
  }
  if (loops) {
    A = asum.loop(cnt, fill_mean, fill, D);
    g.row(xl, i, xlj);
    g.score(xlj, xri, A, z, s);
    sm.add(s, xlj);
  }
  gv2_fwd_finish(g, sm, i, bias, out, row_m, row_l, concat);
}

// ---------------------------------------------------------------------------
// forward, dense: 256 / G rows of a graph per workgroup, neighbour tiles of 32 with x_l staged in LDS
// ---------------------------------------------------------------------------
template <int G, int NCH, int DB, class Src>
__global__ __launch_bounds__(256) void k_gv2_dense_fwd(Src src, const float* __restrict__ xl,
                                                       const float* __restrict__ xr, const float* __restrict__ ea,
                                                       const float* __restrict__ w_e, const float* __restrict__ att,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       float* __restrict__ row_m, float* __restrict__ row_l, int H,
                                                       int C, int D, int concat, int loops, int fill_mean, float fill,
                                                       float slope, int mode) {
  constexpr int CP = G * NCH, S = 256 / G;
  const unsigned* __restrict__ bits = src.bits;
  const int N = src.N, W = src.W, HC = H * C;
  __shared__ float sX[GT * CP];  // [j][c]: conflict-free for G >= 32 (a group reads 32 consecutive words)
  __shared__ float sT[256 * NCH];
  const int b = blockIdx.y, i = blockIdx.x * S + threadIdx.x / G;
  const bool valid = i < N;
  const size_t rb = (size_t)b * N;
  const int64_t r = valid ? (int64_t)(rb + i) : (int64_t)rb;  // a row past the graph's end reads row 0 and writes nothing
  Gv2<G, NCH, DB> g;
  g.init(att, w_e, sT, H, C, D, slope, mode);
  float xri[NCH], xlj[NCH], z[NCH], s[NCH];
  g.row(xr, r, xri);
  Soft<NCH> sm;
  sm.init();
  Attr<DB> A, asum;
  A.zero(), asum.zero();
  int cnt = 0;
  for (int w = 0; w < W; ++w) {
    unsigned word = valid ? bits[(size_t)r * W + w] : 0u;
    if (loops && w == (i >> 5)) word &= ~(1u << (i & 31));  // the diagonal is the loop term's
    if (!__syncthreads_or(word != 0u)) continue;             // also: the previous tile is consumed
    for (int e = threadIdx.x; e < GT * CP; e += 256) {
      const int t = e / CP, c = e - t * CP;
      const int n = w * 32 + t;
      sX[e] = (n < N && c < HC) ? xl[(rb + n) * HC + c] : 0.f;
    }
    __syncthreads();
    while (word) {
      const int jj = __ffs(word) - 1;
      word &= word - 1u;
      if (DB > 0) {
        A.load(ea + ((size_t)r * N + w * 32 + jj) * D, D);
        if (fill_mean) asum.add(A), ++cnt;
      }
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) xlj[ch] = sX[jj * CP + g.gl + ch * G];
      g.score(xlj, xri, A, z, s);
      sm.add(s, xlj);
    }
  }
  if (!valid) return;
  if (loops) {
    A = asum.loop(cnt, fill_mean, fill, D);
    g.row(xl, r, xlj);
    g.score(xlj, xri, A, z, s);
    sm.add(s, xlj);
  }
  gv2_fwd_finish(g, sm, r, bias, out, row_m, row_l, concat);
}

// out [rows, C] = mean over the heads of o [rows, H*C], + bias
__global__ void k_gv2_heads(const float* __restrict__ o, const float* __restrict__ bias, float* __restrict__ out,
                            int64_t rows, int H, int C) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * C) return;
  const int64_t r = t / C;
  const int c = (int)(t - r * C);
  float v = 0.f;
  for (int h = 0; h < H; ++h) v += o[(size_t)r * H * C + h * C + c];
  v *= 1.f / (float)H;
  out[t] = bias ? v + bias[c] : v;
}

// its backward: dO [rows, H*C] = g_out / H broadcast over the heads
__global__ void k_gv2_dout(const float* __restrict__ g_out, float* __restrict__ dO, int64_t rows, int H, int C) {
  const int HC = H * C;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * HC) return;
  const int64_t r = t / HC;
  const int c = (int)(t - r * HC) % C;
  dO[t] = g_out[r * C + c] * (1.f / (float)H);
}

__global__ void k_gv2_add(float* __restrict__ a, const float* __restrict__ b, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) a[t] += b[t];
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------
// the workgroup's sums of the per-group values v (one per lane) over its slots, in slot order -> slot 0's lanes
template <int G>
__device__ __forceinline__ float gv2_slot_sum(float v, float* red) {
  constexpr int S = 256 / G;
  __syncthreads();  // the previous round is read
  red[threadIdx.x] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x < G)
    for (int s = 0; s < S; ++s) t += red[s * G + threadIdx.x];
  return t;
}

// by destination.  part[blk][c * (D + 1) + d]: the workgroup's sum of dz_k[c] a_k[d]; d == D: of dS_k leaky_relu(z_k[c])
template <int G, int NCH, int DB, class Src>
__global__ __launch_bounds__(256) void k_gv2_drow(Src src, const float* __restrict__ xl, const float* __restrict__ xr,
                                                  const float* __restrict__ dO, const float* __restrict__ ea,
                                                  const float* __restrict__ w_e, const float* __restrict__ att,
                                                  const float* __restrict__ row_m, const float* __restrict__ row_l,
                                                  float* __restrict__ delta_out, float* __restrict__ g_xl,
                                                  float* __restrict__ g_xr, float* __restrict__ g_ea,
                                                  float* __restrict__ part, int64_t M, int H, int C, int D, int loops,
                                                  int fill_mean, float fill, float slope, int mode) {
  constexpr int S = 256 / G, DW = DB > 0 ? DB : 1;
  __shared__ float sT[256 * NCH];
  __shared__ float red[256];
  Gv2<G, NCH, DB> g;
  g.init(att, w_e, sT, H, C, D, slope, mode);
  const int gl = g.gl, HC = g.HC;
  float gw[NCH][DW], gatt[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    gatt[ch] = 0.f;
#pragma unroll
    for (int d = 0; d < DW; ++d) gw[ch][d] = 0.f;
  }
  for (int64_t i = (int64_t)blockIdx.x * S + threadIdx.x / G; i < M; i += (int64_t)gridDim.x * S) {
    float xri[NCH], go[NCH], m[NCH], l[NCH], xlj[NCH], z[NCH], s[NCH], dp[NCH], delta[NCH], gxr[NCH];
    g.row(xr, i, xri), g.row(dO, i, go), g.stat(row_m, i, m), g.stat(row_l, i, l);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) delta[ch] = 0.f, gxr[ch] = 0.f;
    const bool live = row_l[(size_t)i * H] > 0.f;  // the row has a term (the same for every head)
    Attr<DB> A, asum, gm;
    A.zero(), asum.zero(), gm.zero();
    int cnt = 0;
    int64_t j, k;
    // alpha and dP of the term (j, A): s and dp
    auto term = [&](int64_t jj) {
      g.row(xl, jj, xlj);
      g.score(xlj, xri, A, z, s);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        s[ch] = expf(s[ch] - m[ch]) / l[ch];
        dp[ch] = go[ch] * xlj[ch];
      }
      g.head_sum(dp);
    };
    // the gradients of the term: dz in z; -> gxr, gatt, gw
    auto grads = [&]() {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const float ds = s[ch] * (dp[ch] - delta[ch]);
        gatt[ch] = fmaf(ds, lrelu(z[ch], slope), gatt[ch]);
        z[ch] = g.ok[ch] ? ds * g.att[ch] * (z[ch] > 0.f ? 1.f : slope) : 0.f;
        gxr[ch] += z[ch];
#pragma unroll
        for (int d = 0; d < DB; ++d) gw[ch][d] = fmaf(z[ch], A.v[d], gw[ch][d]);
      }
    };
    // W_e^T dz, the same in every lane of the group
    auto to_attr = [&](Attr<DB>& r) {
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        float t = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) t = fmaf(g.w[ch][d], z[ch], t);
        r.v[d] = d < D ? group_sum<G>(t) : 0.f;  // uniform
      }
    };
    // g_edge_attr[k] = a + b: column d by lane d % G
    auto store_attr = [&](const Attr<DB>& a, const Attr<DB>& b, int64_t kk) {
#pragma unroll
      for (int d = 0; d < DB; ++d)
        if (d < D && d % G == gl) g_ea[(size_t)kk * D + d] = a.v[d] + b.v[d];
    };
    if (live) {
      auto it = src.row(i);
      while (it.next(j, k)) {
        if (loops && j == i) continue;
        if (DB > 0) {
          A.load(ea + (size_t)k * D, D);
          if (fill_mean) asum.add(A), ++cnt;
        }
        term(j);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) delta[ch] = fmaf(s[ch], dp[ch], delta[ch]);
      }
      if (loops) {
        A = asum.loop(cnt, fill_mean, fill, D);
        term(i);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) delta[ch] = fmaf(s[ch], dp[ch], delta[ch]);
        // second walk, the loop first: its share of g_xl[i], and of the features its mean was taken over
        float al[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) al[ch] = s[ch];
        grads();
        if (g_xl) {
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
            if (g.ok[ch]) g_xl[(size_t)i * HC + gl + ch * G] = fmaf(al[ch], go[ch], z[ch]);
        }
        if (DB > 0 && g_ea && fill_mean && cnt > 0) {
          to_attr(gm);
#pragma unroll
          for (int d = 0; d < DB; ++d) gm.v[d] /= (float)cnt;
        }
      }
      it = src.row(i);
      while (it.next(j, k)) {
        if (loops && j == i) {
          if (DB > 0 && g_ea) A.zero(), store_attr(A, A, k);
          continue;
        }
        if (DB > 0) A.load(ea + (size_t)k * D, D);
        term(j);
        grads();
        if (DB > 0 && g_ea) {
          Attr<DB> ga;
          to_attr(ga);
          store_attr(ga, gm, k);
        }
      }
    }
    if (g_xl && !(live && loops)) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch)
        if (g.ok[ch]) g_xl[(size_t)i * HC + gl + ch * G] = 0.f;
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (!g.ok[ch]) continue;
      g_xr[(size_t)i * HC + gl + ch * G] = gxr[ch];
      if (gl + ch * G == g.hd[ch] * C) delta_out[(size_t)i * H + g.hd[ch]] = delta[ch];
    }
  }
  if (!part) return;  // uniform
  float* mine = part + (size_t)blockIdx.x * HC * (D + 1);
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + ch * G;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      if (d < D) {  // uniform
        const float t = gv2_slot_sum<G>(gw[ch][d], red);
        if (threadIdx.x < G && c < HC) mine[c * (D + 1) + d] = t;
      }
    }
    const float t = gv2_slot_sum<G>(gatt[ch], red);
    if (threadIdx.x < G && c < HC) mine[c * (D + 1) + D] = t;
  }
}

// by source: g_xl[j] (holding the loop term's share) += sum over the column of alpha_k dO_i + dz_k
template <int G, int NCH, int DB, class Src>
__global__ __launch_bounds__(256) void k_gv2_dcol(Src src, const float* __restrict__ xl, const float* __restrict__ xr,
                                                  const float* __restrict__ dO, const float* __restrict__ ea,
                                                  const float* __restrict__ w_e, const float* __restrict__ att,
                                                  const float* __restrict__ row_m, const float* __restrict__ row_l,
                                                  const float* __restrict__ delta, float* __restrict__ g_xl, int64_t M,
                                                  int H, int C, int D, int loops, float slope, int mode) {
  __shared__ float sT[256 * NCH];
  const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (j >= M) return;
  Gv2<G, NCH, DB> g;
  g.init(att, w_e, sT, H, C, D, slope, mode);
  float xlj[NCH], acc[NCH], xri[NCH], go[NCH], m[NCH], l[NCH], dl[NCH], z[NCH], s[NCH], dp[NCH];
  g.row(xl, j, xlj), g.row(g_xl, j, acc);
  Attr<DB> A;
  A.zero();
  auto it = src.column(j);
  int64_t i, k;
  while (it.next(i, k)) {
    if (loops && i == j) continue;
    if (DB > 0) A.load(ea + (size_t)k * D, D);
    g.row(xr, i, xri), g.row(dO, i, go), g.stat(row_m, i, m), g.stat(row_l, i, l), g.stat(delta, i, dl);
    g.score(xlj, xri, A, z, s);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) dp[ch] = go[ch] * xlj[ch];
    g.head_sum(dp);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const float alpha = expf(s[ch] - m[ch]) / l[ch];
      const float ds = alpha * (dp[ch] - dl[ch]);
      acc[ch] += fmaf(alpha, go[ch], ds * g.att[ch] * (z[ch] > 0.f ? 1.f : slope));
    }
  }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
    if (g.ok[ch]) g_xl[(size_t)j * g.HC + g.gl + ch * G] = acc[ch];
}

// g_w_e[c * D + d] and g_att[c] = the sum over the n partials of part[p][c * (D + 1) + d] in index order.  A workgroup
// takes 16 elements; 16 slices of the partials are summed side by side and then added up in slice order.
__global__ __launch_bounds__(256) void k_gv2_sum_parts(const float* __restrict__ part, int n, float* __restrict__ g_w,
                                                       float* __restrict__ g_att, int HC, int D) {
  __shared__ float red[256];
  const int L = HC * (D + 1);
  const int el = threadIdx.x % 16, sl = threadIdx.x / 16;
  const int e = blockIdx.x * 16 + el;
  const int per = (n + 15) / 16;
  float t = 0.f;
  if (e < L)
    for (int p = sl * per; p < min(n, (sl + 1) * per); ++p) t += part[(size_t)p * L + e];
  red[threadIdx.x] = t;
  __syncthreads();
  if (sl != 0 || e >= L) return;
  t = 0.f;
  for (int s = 0; s < 16; ++s) t += red[s * 16 + el];
  const int c = e / (D + 1), d = e - c * (D + 1);
  if (d < D) {
    if (g_w) g_w[c * D + d] = t;
  } else if (g_att) {
    g_att[c] = t;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool gv2_unsupported(int64_t R, int Fi, int H, int C, int D) {
  return Fi > 128 || (int64_t)H * C > 128 || D > GCM_GATV2_MAX_EDGE_DIM || R > (1 << 30);
}

int lane_group(int HC) { return HC <= 8 ? 8 : HC <= 16 ? 16 : HC <= 32 ? 32 : 64; }

// how a head's score is summed over its lanes (Gv2::head_sum)
int head_mode(int H, int C) {
  if ((C & (C - 1)) == 0 && C <= lane_group(H * C)) return 0;
  return H == 1 ? 1 : 2;
}

// launch K<G, NCH, DB, ...> with the lane group of this H*C and the register bucket of this D (0: no edge features)
#define GV2_LAUNCH_G(K, SRC, DB, GRID, s, ...)                                                         \
  if (HC <= 8) hipLaunchKernelGGL((K<8, 1, DB, SRC>), GRID(8), dim3(256), 0, s, __VA_ARGS__);          \
  else if (HC <= 16) hipLaunchKernelGGL((K<16, 1, DB, SRC>), GRID(16), dim3(256), 0, s, __VA_ARGS__);  \
  else if (HC <= 32) hipLaunchKernelGGL((K<32, 1, DB, SRC>), GRID(32), dim3(256), 0, s, __VA_ARGS__);  \
  else if (HC <= 64) hipLaunchKernelGGL((K<64, 1, DB, SRC>), GRID(64), dim3(256), 0, s, __VA_ARGS__);  \
  else hipLaunchKernelGGL((K<64, 2, DB, SRC>), GRID(64), dim3(256), 0, s, __VA_ARGS__);
#define GV2_LAUNCH(K, SRC, GRID, s, ...)           \
  if (D == 0) {                                    \
    GV2_LAUNCH_G(K, SRC, 0, GRID, s, __VA_ARGS__)  \
  } else if (D <= 4) {                             \
    GV2_LAUNCH_G(K, SRC, 4, GRID, s, __VA_ARGS__)  \
  } else {                                         \
    GV2_LAUNCH_G(K, SRC, 32, GRID, s, __VA_ARGS__) \
  }

#define GV2_ROW_GRID(G) dim3(blocks(R * (G), 256))
#define GV2_DROW_GRID(G) dim3(nb)
#define GV2_DENSE_GRID(G) dim3(blocks(N, 256 / (G)), B)

unsigned drow_blocks(int64_t R, int HC) {
  return (unsigned)std::min<int64_t>(GV2_PARTS, blocks(R * lane_group(HC), 256));
}

// x_l, x_r
int project(const float* x, const float* w_l, const float* b_l, const float* w_r, const float* b_r, float* xl,
            float* xr, int64_t R, int Fi, int HC, hipStream_t s) {
  int rc = mm_xwt(x, w_l, b_l, xl, R, Fi, HC, s);
  if (rc || !w_r) return rc;
  return mm_xwt(x, w_r, b_r, xr, R, Fi, HC, s);
}

int heads(const float* o, const float* bias, float* out, int64_t R, int H, int C, hipStream_t s) {
  hipLaunchKernelGGL(k_gv2_heads, dim3(blocks(R * C, 256)), dim3(256), 0, s, o, bias, out, R, H, C);
  return gcm_launch_status();
}

struct BwdWs {
  size_t dO, gxl, gxr, delta, part, tmp, slabs, bitsT, total;
};
BwdWs bwd_ws(int64_t R, int Fi, int H, int C, int D, int concat, size_t bitsT_bytes) {
  BwdWs w;
  const int64_t HC = (int64_t)H * C;
  int nsplit, kchunk;
  wgrad_split(R, &nsplit, &kchunk);
  const size_t slab_f = std::max<size_t>((size_t)nsplit * HC * Fi, (size_t)colsum_slabs(R) * HC);
  Carve c;
  w.dO = c.take(concat ? 0 : R * HC * 4);
  w.gxl = c.take(R * HC * 4), w.gxr = c.take(R * HC * 4), w.delta = c.take(R * H * 4);
  w.part = c.take((size_t)drow_blocks(R, (int)HC) * HC * (D + 1) * 4);
  w.tmp = c.take(R * Fi * 4);
  w.slabs = c.take(slab_f * 4);
  w.bitsT = c.take(bitsT_bytes);
  w.total = c.at;
  return w;
}

struct Cfg {
  int Fi, H, C, D, concat, loops, fill_mean;
  float fill, slope;
};

bool cfg_ok(const Cfg& c) { return c.Fi > 0 && c.H > 0 && c.C > 0 && c.D >= 0; }

// both layers' backward after dO is known: the two sweeps over `src`, the parameter sums, the GEMMs
template <class Src>
int backward(Src src, const float* dO, const float* x, const float* w_l, const float* w_r, const float* att,
             const float* w_e, const float* ea, const float* xl, const float* xr, const float* row_m,
             const float* row_l, float* g_x, float* g_w_l, float* g_b_l, float* g_w_r, float* g_b_r, float* g_att,
             float* g_w_e, float* g_ea, const BwdWs& L, char* ws, int64_t R, const Cfg& cf, hipStream_t s) {
  const int H = cf.H, C = cf.C, D = cf.D, HC = H * C, Fi = cf.Fi;
  const int mode = head_mode(H, C);
  const bool shared = !w_r;
  const bool want_l = g_x || g_w_l || g_b_l;  // with shared weights these take x_r's share too
  float* gxl = (float*)(ws + L.gxl);
  float* gxr = (float*)(ws + L.gxr);
  float* dl = (float*)(ws + L.delta);
  float* part = (g_att || g_w_e) ? (float*)(ws + L.part) : nullptr;
  float* slabs = (float*)(ws + L.slabs);
  if (!xr) xr = xl;
  int rc;
  const unsigned nb = drow_blocks(R, HC);
  GV2_LAUNCH(k_gv2_drow, Src, GV2_DROW_GRID, s, src, xl, xr, dO, ea, w_e, att, row_m, row_l, dl, want_l ? gxl : nullptr,
             gxr, g_ea, part, R, H, C, D, cf.loops, cf.fill_mean, cf.fill, cf.slope, mode)
  if ((rc = gcm_launch_status())) return rc;
  if (want_l) {
    GV2_LAUNCH(k_gv2_dcol, Src, GV2_ROW_GRID, s, src, xl, xr, dO, ea, w_e, att, row_m, row_l, (const float*)dl, gxl, R, H,
               C, D, cf.loops, cf.slope, mode)
    if ((rc = gcm_launch_status())) return rc;
  }
  if (part) {
    hipLaunchKernelGGL(k_gv2_sum_parts, dim3(blocks((int64_t)HC * (D + 1), 16)), dim3(256), 0, s, part, (int)nb, g_w_e,
                       g_att, HC, D);
    if ((rc = gcm_launch_status())) return rc;
  }
  if (shared) {
    if (!want_l) return GCM_OK;
    hipLaunchKernelGGL(k_gv2_add, dim3(blocks(R * HC, 256)), dim3(256), 0, s, gxl, (const float*)gxr, R * HC);
    if ((rc = gcm_launch_status())) return rc;
    if (g_x && (rc = mm_gw(gxl, w_l, g_x, R, Fi, HC, s))) return rc;
    if (g_w_l && (rc = wgrad(gxl, x, g_w_l, slabs, R, Fi, HC, s))) return rc;
    if (g_b_l && (rc = colsum(gxl, R, HC, g_b_l, slabs, s))) return rc;
    return GCM_OK;
  }
  if (g_x) {
    float* tmp = (float*)(ws + L.tmp);
    if ((rc = mm_gw(gxl, w_l, tmp, R, Fi, HC, s)) || (rc = mm_gw(gxr, w_r, g_x, R, Fi, HC, s))) return rc;
    hipLaunchKernelGGL(k_gv2_add, dim3(blocks(R * Fi, 256)), dim3(256), 0, s, g_x, (const float*)tmp, R * Fi);
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_w_l && (rc = wgrad(gxl, x, g_w_l, slabs, R, Fi, HC, s))) return rc;
  if (g_b_l && (rc = colsum(gxl, R, HC, g_b_l, slabs, s))) return rc;
  if (g_w_r && (rc = wgrad(gxr, x, g_w_r, slabs, R, Fi, HC, s))) return rc;
  if (g_b_r && (rc = colsum(gxr, R, HC, g_b_r, slabs, s))) return rc;
  return GCM_OK;
}

// g_bias, and dO: g_out itself when the heads are concatenated
int bwd_head(const float* g_out, float* g_bias, const float** dO, const BwdWs& L, char* ws, int64_t R, const Cfg& cf,
             hipStream_t s) {
  int rc;
  if (g_bias && (rc = colsum(g_out, R, cf.concat ? cf.H * cf.C : cf.C, g_bias, (float*)(ws + L.slabs), s))) return rc;
  *dO = g_out;
  if (!cf.concat) {
    float* d = (float*)(ws + L.dO);
    hipLaunchKernelGGL(k_gv2_dout, dim3(blocks(R * cf.H * cf.C, 256)), dim3(256), 0, s, g_out, d, R, cf.H, cf.C);
    if ((rc = gcm_launch_status())) return rc;
    *dO = d;
  }
  return GCM_OK;
}

size_t fwd_ws_bytes(int64_t R, int H, int C, int concat) { return concat ? 0 : align256((size_t)R * H * C * 4); }

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: GATv2Conv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_csr_gatv2_fwd_workspace_bytes(int64_t M, int H, int C, int concat) {
  if (M <= 0 || H <= 0 || C <= 0) return 0;
  return fwd_ws_bytes(M, H, C, concat);
}

extern "C" int gcm_csr_gatv2_fwd(const float* x, const float* w_l, const float* b_l, const float* w_r,
                                 const float* b_r, const float* att, const float* w_e, const float* bias,
                                 const float* edge_attr, const int64_t* row_ptr, const int64_t* col,
                                 const int64_t* csr_perm, float* out, float* xl, float* xr, float* row_m, float* row_l,
                                 void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int Fi, int H, int C,
                                 int D, int concat, int add_self_loops, int fill_mean, float fill_value,
                                 float negative_slope, gcm_stream_t stream) {
  GCM_REQUIRE(x && w_l && att && row_ptr && out && xl && row_m && row_l);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && H > 0 && C > 0 && D >= 0);
  GCM_REQUIRE(E == 0 || col);
  GCM_REQUIRE(w_r ? xr != nullptr : !b_r);
  GCM_REQUIRE(!w_e == (D == 0) && (D == 0 || E == 0 || edge_attr));
  if (gv2_unsupported(M, Fi, H, C, D)) return GCM_EUNSUPPORTED;
  GCM_REQUIRE(concat || (workspace && workspace_bytes >= fwd_ws_bytes(M, H, C, concat)));
  hipStream_t s = (hipStream_t)stream;
  const int HC = H * C;
  const int64_t R = M;
  int rc = project(x, w_l, b_l, w_r, b_r, xl, xr, M, Fi, HC, s);
  if (rc) return rc;
  float* o = concat ? out : (float*)workspace;
  const CsrSrc src{E > 0 ? row_ptr : nullptr, col, csr_perm, nullptr, nullptr, nullptr};
  GV2_LAUNCH(k_gv2_csr_fwd, CsrSrc, GV2_ROW_GRID, s, src, (const float*)xl, (const float*)(w_r ? xr : xl), edge_attr, w_e, att,
             bias, o, row_m, row_l, M, H, C, D, concat, add_self_loops, fill_mean, fill_value, negative_slope,
             head_mode(H, C))
  if ((rc = gcm_launch_status())) return rc;
  return concat ? GCM_OK : heads(o, bias, out, M, H, C, s);
}

extern "C" size_t gcm_csr_gatv2_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int D, int concat) {
  if (M <= 0 || E < 0 || Fi <= 0 || H <= 0 || C <= 0 || D < 0) return 0;
  return bwd_ws(M, Fi, H, C, D, concat, 0).total;
}

extern "C" int gcm_csr_gatv2_bwd(const float* g_out, const float* x, const float* w_l, const float* w_r,
                                 const float* att, const float* w_e, const float* edge_attr, const int64_t* row_ptr,
                                 const int64_t* col, const int64_t* csr_perm, const int64_t* col_ptr,
                                 const int64_t* rows, const int64_t* csc_perm, const float* xl, const float* xr,
                                 const float* row_m, const float* row_l, float* g_x, float* g_w_l, float* g_b_l,
                                 float* g_w_r, float* g_b_r, float* g_att, float* g_w_e, float* g_edge_attr,
                                 float* g_bias, void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int Fi,
                                 int H, int C, int D, int concat, int add_self_loops, int fill_mean, float fill_value,
                                 float negative_slope, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && w_l && att && row_ptr && xl && row_m && row_l && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && H > 0 && C > 0 && D >= 0);
  GCM_REQUIRE(w_r ? xr != nullptr : (!g_w_r && !g_b_r));
  GCM_REQUIRE(!w_e == (D == 0) && (D == 0 || E == 0 || edge_attr) && (D > 0 || (!g_w_e && !g_edge_attr)));
  const bool want_l = g_x || g_w_l || g_b_l;
  GCM_REQUIRE(E == 0 || (col && (!want_l || (col_ptr && rows && csc_perm))));
  if (gv2_unsupported(M, Fi, H, C, D)) return GCM_EUNSUPPORTED;
  const BwdWs L = bwd_ws(M, Fi, H, C, D, concat, 0);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const Cfg cf{Fi, H, C, D, concat, add_self_loops, fill_mean, fill_value, negative_slope};
  const float* dO;
  int rc = bwd_head(g_out, g_bias, &dO, L, ws, M, cf, s);
  if (rc) return rc;
  if (!want_l && !g_w_r && !g_b_r && !g_att && !g_w_e && !g_edge_attr) return GCM_OK;
  const CsrSrc src{E > 0 ? row_ptr : nullptr, col, csr_perm, E > 0 ? col_ptr : nullptr, rows, csc_perm};
  return backward(src, dO, x, w_l, w_r, att, w_e, edge_attr, xl, xr, row_m, row_l, g_x, g_w_l, g_b_l, g_w_r, g_b_r,
                  g_att, g_w_e, g_edge_attr, L, ws, M, cf, s);
}

// ---------------------------------------------------------------------------
// C ABI: DenseGATv2Conv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_dense_gatv2_fwd_workspace_bytes(int B, int N, int H, int C, int concat) {
  if (B <= 0 || N <= 0 || H <= 0 || C <= 0) return 0;
  return fwd_ws_bytes((int64_t)B * N, H, C, concat);
}

extern "C" int gcm_dense_gatv2_fwd(const float* x, const float* adj, const float* w_l, const float* b_l,
                                   const float* w_r, const float* b_r, const float* att, const float* w_e,
                                   const float* bias, const float* edge_attr, float* out, float* xl, float* xr,
                                   float* row_m, float* row_l, unsigned* bits, void* workspace, size_t workspace_bytes,
                                   int B, int N, int Fi, int H, int C, int D, int concat, int add_loop, int fill_mean,
                                   float fill_value, float negative_slope, gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && w_l && att && out && xl && row_m && row_l && bits);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && H > 0 && C > 0 && D >= 0);
  GCM_REQUIRE(w_r ? xr != nullptr : !b_r);
  GCM_REQUIRE(!w_e == (D == 0) && (D == 0 || edge_attr));
  const int64_t R = (int64_t)B * N;
  if (gv2_unsupported(R, Fi, H, C, D) || B > 65535) return GCM_EUNSUPPORTED;
  GCM_REQUIRE(concat || (workspace && workspace_bytes >= fwd_ws_bytes(R, H, C, concat)));
  hipStream_t s = (hipStream_t)stream;
  const int HC = H * C, W = (N + 31) / 32;
  int rc = mask_bits(adj, bits, R, N, W, 0, s);  // the diagonal as adj has it: the loop term is the kernels' own
  if (rc || (rc = project(x, w_l, b_l, w_r, b_r, xl, xr, R, Fi, HC, s))) return rc;
  float* o = concat ? out : (float*)workspace;
  const DenseSrc src{bits, nullptr, N, W};
  GV2_LAUNCH(k_gv2_dense_fwd, DenseSrc, GV2_DENSE_GRID, s, src, (const float*)xl, (const float*)(w_r ? xr : xl),
             edge_attr, w_e, att, bias, o, row_m, row_l, H, C, D, concat, add_loop, fill_mean, fill_value,
             negative_slope, head_mode(H, C))
  if ((rc = gcm_launch_status())) return rc;
  return concat ? GCM_OK : heads(o, bias, out, R, H, C, s);
}

extern "C" size_t gcm_dense_gatv2_bwd_workspace_bytes(int B, int N, int Fi, int H, int C, int D, int concat) {
  if (B <= 0 || N <= 0 || Fi <= 0 || H <= 0 || C <= 0 || D < 0) return 0;
  const int64_t R = (int64_t)B * N;
  return bwd_ws(R, Fi, H, C, D, concat, (size_t)R * ((N + 31) / 32) * 4).total;
}

extern "C" int gcm_dense_gatv2_bwd(const float* g_out, const float* x, const float* w_l, const float* w_r,
                                   const float* att, const float* w_e, const float* edge_attr, const unsigned* bits,
                                   const float* xl, const float* xr, const float* row_m, const float* row_l, float* g_x,
                                   float* g_w_l, float* g_b_l, float* g_w_r, float* g_b_r, float* g_att, float* g_w_e,
                                   float* g_edge_attr, float* g_bias, void* workspace, size_t workspace_bytes, int B,
                                   int N, int Fi, int H, int C, int D, int concat, int add_loop, int fill_mean,
                                   float fill_value, float negative_slope, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && w_l && att && bits && xl && row_m && row_l && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && H > 0 && C > 0 && D >= 0);
  GCM_REQUIRE(w_r ? xr != nullptr : (!g_w_r && !g_b_r));
  GCM_REQUIRE(!w_e == (D == 0) && (D == 0 || edge_attr) && (D > 0 || (!g_w_e && !g_edge_attr)));
  const int64_t R = (int64_t)B * N;
  if (gv2_unsupported(R, Fi, H, C, D) || B > 65535) return GCM_EUNSUPPORTED;
  const int W = (N + 31) / 32;
  const BwdWs L = bwd_ws(R, Fi, H, C, D, concat, (size_t)R * W * 4);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const Cfg cf{Fi, H, C, D, concat, add_loop, fill_mean, fill_value, negative_slope};
  const float* dO;
  int rc = bwd_head(g_out, g_bias, &dO, L, ws, R, cf, s);
  if (rc) return rc;
  const bool want_l = g_x || g_w_l || g_b_l;
  if (!want_l && !g_w_r && !g_b_r && !g_att && !g_w_e && !g_edge_attr) return GCM_OK;
  unsigned* bitsT = (unsigned*)(ws + L.bitsT);
  if (want_l && (rc = mask_bits_t(bits, bitsT, R, N, W, s))) return rc;
  if (g_edge_attr) {  // the sweep visits the set entries only: the rest is zero
    if (hipMemsetAsync(g_edge_attr, 0, (size_t)R * N * D * 4, s) != hipSuccess) return gcm_launch_status();
  }
  const DenseSrc src{bits, bitsT, N, W};
  return backward(src, dO, x, w_l, w_r, att, w_e, edge_attr, xl, xr, row_m, row_l, g_x, g_w_l, g_b_l, g_w_r, g_b_r,
                  g_att, g_w_e, g_edge_attr, L, ws, R, cf, s);
}
