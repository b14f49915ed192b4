// GATConv / DenseGATConv (PyG, GAT v1) forward and backward on gfx950.
//
//   y = x W^T viewed [rows, H, C];  s_src[j,h] = <y[j,h,:], att_src[h]>, s_dst likewise
//   e[i,j,h] = leaky_relu(s_dst[i,h] + s_src[j,h]) over the neighbours j of i, alpha = softmax_j(e)
//   o[i,h,:] = sum_j alpha y[j,h,:];  out = concat_h(o) + bias, or mean_h(o) + bias
//
// A row with no neighbour aggregates nothing: its o is 0 and its out is bias.
//
// dense: the adjacency is read once, into a bit image of its nonzero pattern with the diagonal set when add_loop
// ([B, N, ceil(N/32)] words), which the rest of the forward and the whole backward read instead.  k_gat_dense_fwd
// runs an online softmax over tiles of 32 neighbours, heads outer: scores, masking and the exponentials stay in
// registers and LDS, alpha y runs on v_mfma_f32_32x32x2_f32, and only the per-row statistics (max, sum) [B,N,H]
// leave for the backward, which recomputes alpha from them.  k_gat_dense_bwd is organised by neighbour block:
// dP = dO y^T on the matrix cores, dE = P (dP - delta_i) leaky_relu', alpha^T dO on the matrix cores, the column
// sums of dE in registers, the row sums of dE as one slab per neighbour block summed in order afterwards.  A
// pre-pass of the same kernel computes delta_i = sum_j P dP from the recomputed P (not <dO_i, o_i>: the same P on
// both sides of dP - delta keeps the near-total cancellation of sum_j dE, which the att_dst gradient sums, exact).
// sparse: one thread per (destination, column) over its CSR row, two passes (max, then sum and gather); the self
// loop is a term of its own and i -> i edges are skipped in place.  The backward scatters through the CSC view.
// x W^T, the input gradient and the weight gradient use the tile GEMM of gcn_mm.h.  Nothing accumulates with
// atomics: every sum runs in a fixed order.  Fi, H*C <= 128; any N.
#include <cmath>

#include "attn_bits.h"  // GT, mask_bits

namespace {

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// s_src[r,h] = <y[r,h,:], att_src[h]>, s_dst[r,h] likewise.  One thread per (r, h).
__global__ void k_gat_scores(const float* __restrict__ y, const float* __restrict__ att_src,
                             const float* __restrict__ att_dst, float* __restrict__ s_src,
                             float* __restrict__ s_dst, int64_t rows, int H, int C) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * H) return;
  const int h = (int)(t % H);
  const float* yr = y + (size_t)t * C;  // y[r, h, :] (row r = t / H)
  float a = 0.f, d = 0.f;
  for (int c = 0; c < C; ++c) {
    a = fmaf(yr[c], att_src[h * C + c], a);
    d = fmaf(yr[c], att_dst[h * C + c], d);
  }
  s_src[t] = a, s_dst[t] = d;
}

// out from the per-head aggregates o [rows, H*C]: concat -> o + bias; else mean over h + bias.
__global__ void k_gat_heads(const float* __restrict__ o, const float* __restrict__ bias, float* __restrict__ out,
                            int64_t rows, int H, int C, int concat) {
  const int Fo = concat ? H * C : C;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * Fo) return;
  const int64_t r = t / Fo;
  const int c = (int)(t - r * Fo);
  float v;
  if (concat) {
    v = o[t];
  } else {
    v = 0.f;
    for (int h = 0; h < H; ++h) v += o[(size_t)r * H * C + h * C + c];
    v *= 1.f / (float)H;
  }
  out[t] = bias ? v + bias[c] : v;
}

// backward of k_gat_heads: dO [rows, H*C] = g_out, or g_out / H broadcast over the heads.
__global__ void k_gat_dout(const float* __restrict__ g_out, float* __restrict__ dO, int64_t rows, int H, int C,
                           int concat) {
  const int HC = H * C;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * HC) return;
  const int64_t r = t / HC;
  const int c = (int)(t - r * HC) % C;
  dO[t] = concat ? g_out[t] : g_out[r * C + c] * (1.f / (float)H);
}

// After the attention backward: gsd[r,h] = the sum of its nparts slabs (in order); g_y[r,h,c] += gsd att_dst[h,c];
// t_src = gss y, t_dst = gsd y (the rows whose column sums are g_att_src / g_att_dst).  One thread per (r, h*C + c).
// part: [B][nparts][N][H] with rows = B * N.
__global__ void k_gat_finish(const float* __restrict__ part, int nparts, int N, const float* __restrict__ gss,
                             const float* __restrict__ y, const float* __restrict__ att_dst, float* __restrict__ gy,
                             float* __restrict__ t_src, float* __restrict__ t_dst, int64_t rows, int H, int C) {
  const int HC = H * C;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * HC) return;
  const int64_t r = t / HC;
  const int cc = (int)(t - r * HC), h = cc / C;
  const int64_t b = r / N, i = r - b * N;
  float gsd = 0.f;
  for (int p = 0; p < nparts; ++p) gsd += part[((size_t)(b * nparts + p) * N + i) * H + h];
  gy[t] = fmaf(gsd, att_dst[cc], gy[t]);
  if (t_src) t_src[t] = gss[r * H + h] * y[t];
  if (t_dst) t_dst[t] = gsd * y[t];
}

// out[r,h] = the sum of its nparts slabs part[b][p][i][h] (in order), rows = B * N.  One thread per (r, h).
__global__ void k_gat_sum_parts(const float* __restrict__ part, int nparts, int N, float* __restrict__ out,
                                int64_t rows, int H) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= rows * H) return;
  const int64_t r = t / H;
  const int h = (int)(t - r * H);
  const int64_t b = r / N, i = r - b * N;
  float a = 0.f;
  for (int p = 0; p < nparts; ++p) a += part[((size_t)(b * nparts + p) * N + i) * H + h];
  out[t] = a;
}

// ---------------------------------------------------------------------------
// dense forward: workgroup = (128 rows of one graph, 4 waves x 32), heads outer, neighbour tiles of 32 inner.
// Lane (li, lh) of a wave scores row li against neighbours 16 lh .. 16 lh + 15 of the tile; the MFMA accumulates
// o[32 rows, C of head h] in NCTC tiles of 32 columns.
// ---------------------------------------------------------------------------
template <int NCTC>
__global__ __launch_bounds__(256) void k_gat_dense_fwd(const unsigned* __restrict__ bits, const float* __restrict__ y,
                                                       const float* __restrict__ s_src,
                                                       const float* __restrict__ s_dst, float* __restrict__ o,
                                                       float* __restrict__ row_m, float* __restrict__ row_l, int N,
                                                       int H, int C, float slope) {
  constexpr int CP = 32 * NCTC;
  __shared__ float sY[GT * (CP + 1)];       // [j][c]
  __shared__ float sP[4 * GT * (GT + 1)];   // per wave [i][j]
  __shared__ float sSrc[GT];
  __shared__ float sScale[4 * GT];          // per wave, per row: the rescale of this tile, then l
  const int b = blockIdx.y, i0 = blockIdx.x * 128;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int HC = H * C, W = (N + 31) / 32;
  const int i = i0 + wave * 32 + li;  // the row this lane scores
  const bool row_ok = i < N;
  const size_t rb = (size_t)b * N;
  float* P = sP + wave * GT * (GT + 1);
  float* Sc = sScale + wave * GT;

  for (int h = 0; h < H; ++h) {
    const float sd = row_ok ? s_dst[(rb + i) * H + h] : 0.f;
    float m = -INFINITY, l = 0.f;
    f32x16 acc[NCTC];
#pragma unroll
    for (int c = 0; c < NCTC; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    for (int j0 = 0; j0 < N; j0 += GT) {
      __syncthreads();  // the previous tile's operands are consumed
      for (int e = threadIdx.x; e < GT * CP; e += 256) {
        const int k = e / CP, c = e - k * CP;
        const int j = j0 + k;
        sY[k * (CP + 1) + c] = (j < N && c < C) ? y[(rb + j) * HC + h * C + c] : 0.f;
      }
      if (threadIdx.x < GT) sSrc[threadIdx.x] = j0 + threadIdx.x < N ? s_src[(rb + j0 + threadIdx.x) * H + h] : 0.f;
      const unsigned word = row_ok ? bits[(rb + i) * W + j0 / 32] >> (16 * lh) : 0u;
      __syncthreads();

      float ev[16];
      float tmax = -INFINITY;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        ev[q] = lrelu(sd + sSrc[16 * lh + q], slope);
        if ((word >> q) & 1u) tmax = fmaxf(tmax, ev[q]);
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      const float m_new = fmaxf(m, tmax);
      const float scale = m_new == -INFINITY ? 1.f : expf(m - m_new);
      float ps = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float p = ((word >> q) & 1u) ? expf(ev[q] - m_new) : 0.f;
        ps += p;
        P[li * (GT + 1) + 16 * lh + q] = p;
      }
      ps += __shfl_xor(ps, 32);
      l = fmaf(l, scale, ps);
      m = m_new;
      if (lh == 0) Sc[li] = scale;
      __syncthreads();

#pragma unroll
      for (int c = 0; c < NCTC; ++c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] *= Sc[acc_row(r, lh)];
        mma32(acc[c], P, GT + 1, 1, sY + c * 32, CP + 1, 1, GT, li, lh);
      }
    }

    __syncthreads();
    if (lh == 0) Sc[li] = l;
    if (row_ok && lh == 0) {
      row_m[(rb + i) * H + h] = m;
      row_l[(rb + i) * H + h] = l;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCTC; ++c) {
      const int cc = c * 32 + li;
      if (cc >= C) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = acc_row(r, lh);
        const int ii = i0 + wave * 32 + rr;
        const float lr = Sc[rr];
        if (ii < N) o[(rb + ii) * HC + h * C + cc] = lr > 0.f ? acc[c][r] / lr : 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dense backward: workgroup = (128 neighbours j of one graph, 4 waves x 32), heads outer, row tiles of 32 inner.
// Per tile, lane (li, lh) holds dP[i, j] for j = li and the 16 rows i = acc_row(r, lh) (the MFMA's layout) and
// turns it into P and dE there.  Outputs: gy[j,h,:] = sum_i P dO_i + gss_j att_src[h] (the att_dst term is added
// by k_gat_finish), gss[j,h] = sum_i dE, part[b, block, i, h] = sum over this block's j of dE.
// DELTA: the pre-pass - part[b, block, i, h] = sum over this block's j of P dP, nothing else (summed over the
// blocks, the softmax's row term delta_i = sum_j P dP, from the same P as dE: the two cancel as they should).
// ---------------------------------------------------------------------------
template <int NCTC, bool DELTA>
__global__ __launch_bounds__(256) void k_gat_dense_bwd(
    const unsigned* __restrict__ bits, const float* __restrict__ y, const float* __restrict__ s_src,
    const float* __restrict__ s_dst, const float* __restrict__ row_m, const float* __restrict__ row_l,
    const float* __restrict__ dO, const float* __restrict__ delta, const float* __restrict__ att_src,
    float* __restrict__ gy, float* __restrict__ gss, float* __restrict__ part, int N, int H, int C, float slope) {
  constexpr int CP = 32 * NCTC;
  __shared__ float sDO[GT * (CP + 1)];      // [i][c]
  __shared__ float sP[4 * GT * (GT + 1)];   // per wave [i][j]
  __shared__ float sDE[4 * GT * (GT + 1)];  // per wave [i][j]
  __shared__ float sRow[4 * GT];            // per row of the tile: s_dst, m, l, delta
  __shared__ unsigned sBits[GT * 4];        // [i][wave]
  __shared__ float sRed[4 * GT];
  __shared__ float sG[4 * GT];              // per wave: gss of its 32 j
  const int b = blockIdx.y, jb = blockIdx.x, j0 = jb * 128, nblk = gridDim.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int HC = H * C, W = (N + 31) / 32;
  const int j = j0 + wave * 32 + li;  // the neighbour of this lane
  const bool j_ok = j < N;
  const size_t rb = (size_t)b * N;
  float* P = sP + wave * GT * (GT + 1);
  float* DE = sDE + wave * GT * (GT + 1);

  for (int h = 0; h < H; ++h) {
    const float ss = j_ok ? s_src[(rb + j) * H + h] : 0.f;
    float yv[CP / 2];  // y[j, h, 2 s + lh]: the B operand of dP, for every row tile
#pragma unroll
    for (int s = 0; s < CP / 2; ++s) {
      const int k = 2 * s + lh;
      yv[s] = (j_ok && k < C) ? y[(rb + j) * HC + h * C + k] : 0.f;
    }
    f32x16 acc[NCTC];
#pragma unroll
    for (int c = 0; c < NCTC; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    float gs = 0.f;

    for (int i0 = 0; i0 < N; i0 += GT) {
      __syncthreads();
      for (int e = threadIdx.x; e < GT * CP; e += 256) {
        const int k = e / CP, c = e - k * CP;
        const int i = i0 + k;
        sDO[k * (CP + 1) + c] = (i < N && c < C) ? dO[(rb + i) * HC + h * C + c] : 0.f;
      }
      if (threadIdx.x < GT) {
        const int i = i0 + threadIdx.x;
        const bool ok = i < N;
        const size_t t = (rb + i) * H + h;
        sRow[threadIdx.x * 4 + 0] = ok ? s_dst[t] : 0.f;
        sRow[threadIdx.x * 4 + 1] = ok ? row_m[t] : 0.f;
        sRow[threadIdx.x * 4 + 2] = ok ? row_l[t] : 0.f;
        sRow[threadIdx.x * 4 + 3] = (ok && !DELTA) ? delta[t] : 0.f;
      }
      if (threadIdx.x < GT * 4) {
        const int r = threadIdx.x >> 2, w = threadIdx.x & 3;
        const int i = i0 + r, jw = j0 / 32 + w;
        sBits[r * 4 + w] = (i < N && jw < W) ? bits[(rb + i) * W + jw] : 0u;
      }
      __syncthreads();

      f32x16 dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[r] = 0.f;
#pragma unroll
      for (int s = 0; s < CP / 2; ++s)
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sDO[li * (CP + 1) + 2 * s + lh], yv[s], dp, 0, 0, 0);

#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = acc_row(r, lh);
        const float* row = sRow + rr * 4;
        const bool on = (sBits[rr * 4 + wave] >> li) & 1u;
        const float pre = row[0] + ss;
        const float p = on ? expf(lrelu(pre, slope) - row[1]) / row[2] : 0.f;   // on: l > 0
        if (DELTA) {
          DE[rr * (GT + 1) + li] = p * dp[r];
          continue;
        }
        const float de = p * (dp[r] - row[3]) * (pre > 0.f ? 1.f : slope);
        gs += de;
        P[rr * (GT + 1) + li] = p;
        DE[rr * (GT + 1) + li] = de;
      }
      __syncthreads();

      if (!DELTA)
#pragma unroll
        for (int c = 0; c < NCTC; ++c) mma32(acc[c], P, 1, GT + 1, sDO + c * 32, CP + 1, 1, GT, li, lh);
      if (threadIdx.x < GT * 4) {  // this wave's part of the row sums of dE, then the block's in wave order
        const int r = threadIdx.x & 31, w = threadIdx.x >> 5;
        const float* d = sDE + w * GT * (GT + 1) + r * (GT + 1);
        float a = 0.f;
        for (int q = 0; q < GT; ++q) a += d[q];
        sRed[w * GT + r] = a;
      }
      __syncthreads();
      if (threadIdx.x < GT && i0 + (int)threadIdx.x < N) {
        const int r = threadIdx.x;
        part[(((size_t)b * nblk + jb) * N + i0 + r) * H + h] = ((sRed[r] + sRed[GT + r]) + sRed[2 * GT + r]) + sRed[3 * GT + r];
      }
    }

    if (DELTA) continue;
    gs += __shfl_xor(gs, 32);
    if (lh == 0) sG[wave * GT + li] = gs;
    if (j_ok && lh == 0) gss[(rb + j) * H + h] = gs;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCTC; ++c) {
      const int cc = c * 32 + li;
      if (cc >= C) continue;
      const float as = att_src[h * C + cc];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = acc_row(r, lh);
        const int jj = j0 + wave * 32 + rr;
        if (jj < N) gy[(rb + jj) * HC + h * C + cc] = fmaf(sG[wave * GT + rr], as, acc[c][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// sparse
// ---------------------------------------------------------------------------
// forward: one thread per (destination i, column h*C + c); pass 1 the max score, pass 2 the sum and the gather.
// The loop term (add_self_loops) comes after the edges, as PyG appends the loops; i -> i edges are skipped then.
__global__ void k_gat_csr_fwd(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col,
                              const float* __restrict__ y, const float* __restrict__ s_src,
                              const float* __restrict__ s_dst, float* __restrict__ o, float* __restrict__ row_m,
                              float* __restrict__ row_l, int64_t M, int H, int C, int loops, float slope) {
  const int HC = H * C;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * HC) return;
  const int64_t i = t / HC;
  const int cc = (int)(t - i * HC), h = cc / C;
  const float sd = s_dst[i * H + h];
  const int64_t e0 = row_ptr[i], e1 = row_ptr[i + 1];
  const float el = lrelu(sd + s_src[i * H + h], slope);
  float m = loops ? el : -INFINITY;
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t s = col[e];
    if (loops && s == i) continue;
    m = fmaxf(m, lrelu(sd + s_src[s * H + h], slope));
  }
  float l = 0.f, a = 0.f;
  if (m != -INFINITY) {
    for (int64_t e = e0; e < e1; ++e) {
      const int64_t s = col[e];
      if (loops && s == i) continue;
      const float p = expf(lrelu(sd + s_src[s * H + h], slope) - m);
      l += p;
      a = fmaf(p, y[s * HC + cc], a);
    }
    if (loops) {
      const float p = expf(el - m);
      l += p;
      a = fmaf(p, y[i * HC + cc], a);
    }
  }
  o[t] = l > 0.f ? a / l : 0.f;
  if (cc == h * C) {
    row_m[i * H + h] = m;
    row_l[i * H + h] = l;
  }
}

// backward, per (destination i, head h): alpha and dE of every CSR entry (0 for a skipped i -> i edge) and of the
// loop, and gsd[i,h] = their sum.  Two passes over the row: dP and delta = sum P dP (kept in alpha / de), then dE.
__global__ void k_gat_csr_de(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col,
                             const float* __restrict__ y, const float* __restrict__ s_src,
                             const float* __restrict__ s_dst, const float* __restrict__ row_m,
                             const float* __restrict__ row_l, const float* __restrict__ dO, float* __restrict__ alpha,
                             float* __restrict__ de, float* __restrict__ p_loop, float* __restrict__ de_loop,
                             float* __restrict__ gsd, int64_t M, int H, int C, int loops, float slope) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * H) return;
  const int HC = H * C;
  const int64_t i = t / H;
  const int h = (int)(t - i * H);
  const float sd = s_dst[t], m = row_m[t], l = row_l[t];
  const float* g = dO + (size_t)i * HC + h * C;
  const int64_t e0 = row_ptr[i], e1 = row_ptr[i + 1];
  auto term = [&](int64_t s, float* p, float* dp) {  // P (an entry of a row: l > 0) and dP of source s
    *p = expf(lrelu(sd + s_src[s * H + h], slope) - m) / l;
    float a = 0.f;
    for (int c = 0; c < C; ++c) a = fmaf(g[c], y[(size_t)s * HC + h * C + c], a);
    *dp = a;
  };
  float delta = 0.f;
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t s = col[e];
    float p = 0.f, dp = 0.f;
    if (!(loops && s == i)) term(s, &p, &dp);
    alpha[e * H + h] = p;
    de[e * H + h] = dp;
    delta = fmaf(p, dp, delta);
  }
  float pl = 0.f, dpl = 0.f;
  if (loops) {
    term(i, &pl, &dpl);
    delta = fmaf(pl, dpl, delta);
  }
  float acc = 0.f;
  for (int64_t e = e0; e < e1; ++e) {
    const int64_t s = col[e];
    const float pre = sd + s_src[s * H + h];
    const float d = alpha[e * H + h] * (de[e * H + h] - delta) * (pre > 0.f ? 1.f : slope);
    de[e * H + h] = d;
    acc += d;
  }
  const float dl = loops ? pl * (dpl - delta) * (sd + s_src[t] > 0.f ? 1.f : slope) : 0.f;
  p_loop[t] = pl, de_loop[t] = dl;
  gsd[t] = acc + dl;
}

// backward, per (source j, column h*C + c) over its CSC column: gy = sum alpha dO[dst] + (loop) + gss att_src,
// gss[j,h] = sum dE (+ the loop's)
__global__ void k_gat_csr_gy(const int64_t* __restrict__ col_ptr, const int64_t* __restrict__ rows,
                             const int64_t* __restrict__ perm, const float* __restrict__ alpha,
                             const float* __restrict__ de, const float* __restrict__ p_loop,
                             const float* __restrict__ de_loop, const float* __restrict__ dO,
                             const float* __restrict__ att_src, float* __restrict__ gy, float* __restrict__ gss,
                             int64_t M, int H, int C) {
  const int HC = H * C;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * HC) return;
  const int64_t j = t / HC;
  const int cc = (int)(t - j * HC), h = cc / C;
  float a = 0.f, g = 0.f;
  if (col_ptr)
    for (int64_t k = col_ptr[j]; k < col_ptr[j + 1]; ++k) {
      const int64_t e = perm[k];
      a = fmaf(alpha[e * H + h], dO[rows[k] * HC + cc], a);
      g += de[e * H + h];
    }
  a = fmaf(p_loop[j * H + h], dO[t], a);
  g += de_loop[j * H + h];
  gy[t] = fmaf(g, att_src[cc], a);
  if (cc == h * C) gss[j * H + h] = g;
}

// the forward's common tail and head: y, scores; out from o
int fwd_head(const float* x, const float* w, const float* att_src, const float* att_dst, float* y, float* s_src,
             float* s_dst, int64_t R, int Fi, int H, int C, hipStream_t s) {
  int rc = mm_xwt(x, w, nullptr, y, R, Fi, H * C, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_gat_scores, dim3(blocks(R * H, 256)), dim3(256), 0, s, y, att_src, att_dst, s_src, s_dst,
                     R, H, C);
  return gcm_launch_status();
}

int fwd_tail(const float* o, const float* bias, float* out, int64_t R, int H, int C, int concat, hipStream_t s) {
  const int Fo = concat ? H * C : C;
  hipLaunchKernelGGL(k_gat_heads, dim3(blocks(R * Fo, 256)), dim3(256), 0, s, o, bias, out, R, H, C, concat);
  return gcm_launch_status();
}

bool unsupported(int64_t R, int Fi, int H, int C) {
  return Fi > 128 || (int64_t)H * C > 128 || R > (1 << 30);
}

// backward workspace: dO, gy, t_src, t_dst [R, HC]; delta (dense), gss [R, H]; part (dense: [B, nblk, N, H]; sparse:
// gsd [R, H]); sparse only: alpha, de [E, H], p_loop, de_loop [R, H]; slabs for wgrad / colsum
struct BwdWs {
  size_t dO, gy, tsrc, tdst, delta, gss, part, alpha, de, ploop, deloop, slabs, total;
};
BwdWs bwd_ws(int64_t R, int64_t nparts_rows, bool sparse, int64_t E, int Fi, int H, int C, int Fo) {
  BwdWs w;
  const int64_t HC = (int64_t)H * C;
  int nsplit, kchunk;
  wgrad_split(R, &nsplit, &kchunk);
  const size_t slab_f = std::max<size_t>((size_t)nsplit * HC * Fi,
                                         (size_t)colsum_slabs(R) * std::max<int64_t>(HC, Fo));
  Carve c;
  w.dO = c.take(R * HC * 4), w.gy = c.take(R * HC * 4), w.tsrc = c.take(R * HC * 4), w.tdst = c.take(R * HC * 4);
  w.delta = c.take(R * H * 4), w.gss = c.take(R * H * 4), w.part = c.take(nparts_rows * H * 4);
  const int64_t loop_rows = sparse ? R : 0;
  w.alpha = c.take(E * H * 4), w.de = c.take(E * H * 4), w.ploop = c.take(loop_rows * H * 4);
  w.deloop = c.take(loop_rows * H * 4);
  w.slabs = c.take(slab_f * 4);
  w.total = c.at;
  return w;
}

// the backward's common tail: the att_dst term of gy, g_att_*, g_x = gy W, g_w = gy^T x
int bwd_tail(const float* x, const float* w, const float* y, const float* att_dst, const float* part, int nparts,
             int N, const BwdWs& L, char* ws, float* g_x, float* g_w, float* g_att_src, float* g_att_dst,
             int64_t R, int Fi, int H, int C, hipStream_t s) {
  const int HC = H * C;
  float* gy = (float*)(ws + L.gy);
  float* tsrc = g_att_src ? (float*)(ws + L.tsrc) : nullptr;
  float* tdst = g_att_dst ? (float*)(ws + L.tdst) : nullptr;
  float* slabs = (float*)(ws + L.slabs);
  hipLaunchKernelGGL(k_gat_finish, dim3(blocks(R * HC, 256)), dim3(256), 0, s, part, nparts, N,
                     (const float*)(ws + L.gss), y, att_dst, gy, tsrc, tdst, R, H, C);
  int rc = gcm_launch_status();
  if (rc) return rc;
  if (g_att_src && (rc = colsum(tsrc, R, HC, g_att_src, slabs, s))) return rc;
  if (g_att_dst && (rc = colsum(tdst, R, HC, g_att_dst, slabs, s))) return rc;
  if (g_x && (rc = mm_gw(gy, w, g_x, R, Fi, HC, s))) return rc;  // g_x = gy W
  if (g_w && (rc = wgrad(gy, x, g_w, slabs, R, Fi, HC, s))) return rc;
  return GCM_OK;
}

int dout(const float* g_out, const BwdWs& L, char* ws, int64_t R, int H, int C, int concat, hipStream_t s) {
  hipLaunchKernelGGL(k_gat_dout, dim3(blocks(R * H * C, 256)), dim3(256), 0, s, g_out, (float*)(ws + L.dO), R, H, C,
                     concat);
  return gcm_launch_status();
}

int dense_blocks(int N) { return (N + 127) / 128; }

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: DenseGATConv
// ---------------------------------------------------------------------------
extern "C" int gcm_dense_gatconv_fwd(const float* x, const float* adj, const float* w, const float* att_src,
                                     const float* att_dst, const float* bias, float* out, float* y, float* o,
                                     float* s_src, float* s_dst, float* row_m, float* row_l, unsigned* bits, int B,
                                     int N, int Fi, int H, int C, int concat, int add_loop, float negative_slope,
                                     gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && w && att_src && att_dst && out && y && o && s_src && s_dst && row_m && row_l && bits);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && H > 0 && C > 0);
  const int64_t R = (int64_t)B * N;
  if (unsupported(R, Fi, H, C) || B > 65535) return GCM_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int W = (N + 31) / 32;
  int rc = mask_bits(adj, bits, R, N, W, add_loop, s);
  if (rc || (rc = fwd_head(x, w, att_src, att_dst, y, s_src, s_dst, R, Fi, H, C, s))) return rc;
  const dim3 grid(dense_blocks(N), B);
  dispatch_nct((C + 31) / 32, [&](auto n) {
    hipLaunchKernelGGL(k_gat_dense_fwd<n()>, grid, dim3(256), 0, s, bits, y, s_src, s_dst, o, row_m, row_l, N, H, C,
                       negative_slope);
  });
  if ((rc = gcm_launch_status())) return rc;
  return fwd_tail(o, bias, out, R, H, C, concat, s);
}

extern "C" size_t gcm_dense_gatconv_bwd_workspace_bytes(int B, int N, int Fi, int H, int C, int concat) {
  if (B <= 0 || N <= 0 || Fi <= 0 || H <= 0 || C <= 0) return 0;
  const int64_t R = (int64_t)B * N;
  return bwd_ws(R, R * dense_blocks(N), false, 0, Fi, H, C, concat ? H * C : C).total;
}

extern "C" int gcm_dense_gatconv_bwd(const float* g_out, const float* x, const float* w, const float* att_src,
                                     const float* att_dst, const float* y, const float* s_src,
                                     const float* s_dst, const float* row_m, const float* row_l,
                                     const unsigned* bits, float* g_x, float* g_w, float* g_att_src,
                                     float* g_att_dst, float* g_bias, void* workspace, size_t workspace_bytes, int B,
                                     int N, int Fi, int H, int C, int concat, float negative_slope,
                                     gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && w && att_src && att_dst && y && s_src && s_dst && row_m && row_l && bits && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && H > 0 && C > 0);
  const int64_t R = (int64_t)B * N;
  if (unsupported(R, Fi, H, C) || B > 65535) return GCM_EUNSUPPORTED;
  const int Fo = concat ? H * C : C;
  const int nblk = dense_blocks(N);
  const BwdWs L = bwd_ws(R, R * nblk, false, 0, Fi, H, C, Fo);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int rc;
  if (g_bias && (rc = colsum(g_out, R, Fo, g_bias, (float*)(ws + L.slabs), s))) return rc;
  if (!g_x && !g_w && !g_att_src && !g_att_dst) return GCM_OK;
  if ((rc = dout(g_out, L, ws, R, H, C, concat, s))) return rc;
  float* part = (float*)(ws + L.part);
  const dim3 grid(nblk, B);
  const float* dO = (const float*)(ws + L.dO);
  float* gy = (float*)(ws + L.gy);
  float* gss = (float*)(ws + L.gss);
  float* dl = (float*)(ws + L.delta);
  for (int pass = 0; pass < 2; ++pass) {  // delta = sum_j P dP, then the gradients
    dispatch_nct((C + 31) / 32, [&](auto n) {
      if (pass == 0)
        hipLaunchKernelGGL((k_gat_dense_bwd<n(), true>), grid, dim3(256), 0, s, bits, y, s_src, s_dst, row_m, row_l, dO,
                           dl, att_src, gy, gss, part, N, H, C, negative_slope);
      else
        hipLaunchKernelGGL((k_gat_dense_bwd<n(), false>), grid, dim3(256), 0, s, bits, y, s_src, s_dst, row_m, row_l, dO,
                           dl, att_src, gy, gss, part, N, H, C, negative_slope);
    });
    if ((rc = gcm_launch_status())) return rc;
    if (pass == 0) {
      hipLaunchKernelGGL(k_gat_sum_parts, dim3(blocks(R * H, 256)), dim3(256), 0, s, part, nblk, N, dl, R, H);
      if ((rc = gcm_launch_status())) return rc;
    }
  }
  if ((rc = gcm_launch_status())) return rc;
  return bwd_tail(x, w, y, att_dst, part, nblk, N, L, ws, g_x, g_w, g_att_src, g_att_dst, R, Fi, H, C, s);
}

// ---------------------------------------------------------------------------
// C ABI: GATConv
// ---------------------------------------------------------------------------
extern "C" int gcm_csr_gatconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* w,
                                   const float* att_src, const float* att_dst, const float* bias, float* out,
                                   float* y, float* o, float* s_src, float* s_dst, float* row_m, float* row_l,
                                   int64_t M, int64_t E, int Fi, int H, int C, int concat, int add_self_loops,
                                   float negative_slope, gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && w && att_src && att_dst && out && y && o && s_src && s_dst && row_m && row_l);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && H > 0 && C > 0);
  GCM_REQUIRE(E == 0 || col);
  if (unsupported(M, Fi, H, C)) return GCM_EUNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  int rc = fwd_head(x, w, att_src, att_dst, y, s_src, s_dst, M, Fi, H, C, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_gat_csr_fwd, dim3(blocks(M * H * C, 256)), dim3(256), 0, s, row_ptr, col, y, s_src, s_dst,
                     o, row_m, row_l, M, H, C, add_self_loops, negative_slope);
  if ((rc = gcm_launch_status())) return rc;
  return fwd_tail(o, bias, out, M, H, C, concat, s);
}

extern "C" size_t gcm_csr_gatconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int concat) {
  if (M <= 0 || E < 0 || Fi <= 0 || H <= 0 || C <= 0) return 0;
  return bwd_ws(M, M, true, E, Fi, H, C, concat ? H * C : C).total;
}

extern "C" int gcm_csr_gatconv_bwd(const float* g_out, const float* x, const int64_t* row_ptr, const int64_t* col,
                                   const int64_t* col_ptr, const int64_t* rows, const int64_t* perm, const float* w,
                                   const float* att_src, const float* att_dst, const float* y, const float* s_src, const float* s_dst, const float* row_m, const float* row_l,
                                   float* g_x, float* g_w, float* g_att_src, float* g_att_dst, float* g_bias,
                                   void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int Fi, int H,
                                   int C, int concat, int add_self_loops, float negative_slope,
                                   gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && row_ptr && w && att_src && att_dst && y && s_src && s_dst && row_m && row_l && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && H > 0 && C > 0);
  // (the CSC view serves g_x / g_w / g_att_*: a bias-only request comes without one)
  const bool bias_only = !g_x && !g_w && !g_att_src && !g_att_dst;
  GCM_REQUIRE(E == 0 || (col && (bias_only || (col_ptr && rows && perm))));
  if (unsupported(M, Fi, H, C)) return GCM_EUNSUPPORTED;
  const int Fo = concat ? H * C : C;
  const BwdWs L = bwd_ws(M, M, true, E, Fi, H, C, Fo);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int rc;
  if (g_bias && (rc = colsum(g_out, M, Fo, g_bias, (float*)(ws + L.slabs), s))) return rc;
  if (bias_only) return GCM_OK;
  if ((rc = dout(g_out, L, ws, M, H, C, concat, s))) return rc;
  float* alpha = (float*)(ws + L.alpha);
  float* de = (float*)(ws + L.de);
  float* ploop = (float*)(ws + L.ploop);
  float* deloop = (float*)(ws + L.deloop);
  float* gsd = (float*)(ws + L.part);
  const float* dO = (const float*)(ws + L.dO);
  hipLaunchKernelGGL(k_gat_csr_de, dim3(blocks(M * H, 256)), dim3(256), 0, s, row_ptr, col, y, s_src, s_dst, row_m,
                     row_l, dO, alpha, de, ploop, deloop, gsd, M, H, C,
                     add_self_loops, negative_slope);
  if ((rc = gcm_launch_status())) return rc;
  hipLaunchKernelGGL(k_gat_csr_gy, dim3(blocks(M * H * C, 256)), dim3(256), 0, s, E ? col_ptr : nullptr, rows,
                     perm, alpha, de, ploop, deloop, dO, att_src, (float*)(ws + L.gy), (float*)(ws + L.gss), M, H,
                     C);
  if ((rc = gcm_launch_status())) return rc;
  return bwd_tail(x, w, y, att_dst, gsd, 1, (int)M, L, ws, g_x, g_w, g_att_src, g_att_dst, M, Fi, H, C, s);
}
