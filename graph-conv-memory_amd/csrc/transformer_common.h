// The kernels and host helpers of TransformerConv / DenseTransformerConv that csrc/transformerconv.hip (without edge
// features) and csrc/transformer_edge.hip (with them) both build on: the heads / skip / gate kernels, the edge-free
// attention kernels, the saved and workspace layouts and the stacked projection and its gradients.  Everything is
// in an unnamed namespace: each of the two files gets its own copy, as when this was part of transformerconv.hip.
#pragma once
#include <cmath>

#include "attn_bits.h"

namespace {

// ---------------------------------------------------------------------------
// heads, skip and gate.  One wave per row, lane e holds columns e and e + 64 of the D <= 128 outputs.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

__device__ __forceinline__ float heads_of(const float* __restrict__ orow, int c, int H, int C, int concat) {
  if (concat) return orow[c];
  float v = 0.f;
  for (int h = 0; h < H; ++h) v += orow[h * C + c];
  return v * (1.f / (float)H);
}

// out from the per-head aggregates o [rows, H*C] and the skip r = proj[:, 3 H C ...] (root)
__global__ __launch_bounds__(256) void k_tr_out(const float* __restrict__ o, const float* __restrict__ proj, int ldp,
                                                const float* __restrict__ w_beta, float* __restrict__ out,
                                                float* __restrict__ gate, int64_t rows, int H, int C, int concat,
                                                int root) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63, HC = H * C, D = concat ? HC : C;
  const float* orow = o + (size_t)row * HC;
  const float* rrow = proj + (size_t)row * ldp + 3 * HC;
  float om[2], r[2], part = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = lane + 64 * q;
    om[q] = r[q] = 0.f;
    if (c >= D) continue;
    om[q] = heads_of(orow, c, H, C, concat);
    if (root) r[q] = rrow[c];
    if (w_beta) part += fmaf(w_beta[2 * D + c], om[q] - r[q], fmaf(w_beta[D + c], r[q], w_beta[c] * om[q]));
  }
  float g = 0.f;
  if (w_beta) {
    g = 1.f / (1.f + expf(-wave_sum(part)));
    if (lane == 0) gate[row] = g;
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = lane + 64 * q;
    if (c >= D) continue;
    out[(size_t)row * D + c] = w_beta ? fmaf(g, r[q] - om[q], om[q]) : om[q] + r[q];
  }
}

// backward of k_tr_out: dO [rows, H*C] (g_om, or g_om / H broadcast over the heads), dR into gp[:, 3 H C ...] (root),
// t [rows, 3 D] = g_logit [om, r, om - r] (the rows whose column sum is g_w_beta; with t only)
__global__ __launch_bounds__(256) void k_tr_dout(const float* __restrict__ g_out, const float* __restrict__ o,
                                                 const float* __restrict__ proj, int ldp,
                                                 const float* __restrict__ w_beta, const float* __restrict__ gate,
                                                 float* __restrict__ dO, float* __restrict__ gp, float* __restrict__ t,
                                                 int64_t rows, int H, int C, int concat, int root) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63, HC = H * C, D = concat ? HC : C;
  const float* orow = o + (size_t)row * HC;
  const float* rrow = proj + (size_t)row * ldp + 3 * HC;
  float go[2], om[2], r[2], part = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = lane + 64 * q;
    go[q] = om[q] = r[q] = 0.f;
    if (c >= D) continue;
    go[q] = g_out[(size_t)row * D + c];
    if (w_beta) {
      om[q] = heads_of(orow, c, H, C, concat);
      r[q] = rrow[c];
      part = fmaf(go[q], r[q] - om[q], part);
    }
  }
  float g = 0.f, gl = 0.f;
  if (w_beta) {
    g = gate[row];
    gl = wave_sum(part) * g * (1.f - g);
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = lane + 64 * q;
    if (c >= D) continue;
    float g_om = go[q], g_r = go[q];
    if (w_beta) {
      g_om = fmaf(gl, w_beta[c] + w_beta[2 * D + c], go[q] * (1.f - g));
      g_r = fmaf(gl, w_beta[D + c] - w_beta[2 * D + c], go[q] * g);
      if (t) {
        float* tr = t + (size_t)row * 3 * D;
        tr[c] = gl * om[q], tr[D + c] = gl * r[q], tr[2 * D + c] = gl * (om[q] - r[q]);
      }
    }
    if (root) gp[(size_t)row * ldp + 3 * HC + c] = g_r;
    if (concat) {
      dO[(size_t)row * HC + c] = g_om;
    } else {
      const float v = g_om * (1.f / (float)H);
      for (int h = 0; h < H; ++h) dO[(size_t)row * HC + h * C + c] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// dense forward: workgroup = (128 rows of one graph, 4 waves x 32), heads outer, neighbour tiles of 32 inner.
// Lane (li, lh) holds q of row li (scaled, channels 2 s + lh: the B operand of S^T = K Q^T) and, after the product,
// the scores of row li against the 16 neighbours acc_row(r, lh) of the tile; P goes through LDS into P V, which
// accumulates o[32 rows, C of head h] in NCTC tiles of 32 columns.
// ---------------------------------------------------------------------------
#define TR_STAGE_KV()                                                          \
  for (int e = threadIdx.x; e < GT * CP; e += 256) {                           \
    const int k = e / CP, c = e - k * CP;                                      \
    const int j = j0 + k;                                                      \
    const bool ok = j < N && c < C;                                            \
    const float* src = proj + (rb + j) * ldp + HC + h * C + c;                 \
    sK[k * (CP + 1) + c] = ok ? src[0] : 0.f;                                  \
    sV[k * (CP + 1) + c] = ok ? src[HC] : 0.f;                                 \
  }

template <int NCTC>
__global__ __launch_bounds__(256) void k_tr_dense_fwd(const unsigned* __restrict__ bits, const float* __restrict__ proj,
                                                      int ldp, float* __restrict__ o, float* __restrict__ row_m,
                                                      float* __restrict__ row_l, int N, int H, int C, float scale) {
  constexpr int CP = 32 * NCTC;
  __shared__ float sK[GT * (CP + 1)];      // [j][c]
  __shared__ float sV[GT * (CP + 1)];      // [j][c]
  __shared__ float sP[4 * GT * (GT + 1)];  // per wave [i][j]
  __shared__ float sScale[4 * GT];         // per wave, per row: the rescale of this tile, then l
  const int b = blockIdx.y, i0 = blockIdx.x * 128;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int HC = H * C, W = (N + 31) / 32;
  const int i = i0 + wave * 32 + li;  // the row this lane scores
  const bool row_ok = i < N;
  const size_t rb = (size_t)b * N;
  float* P = sP + wave * GT * (GT + 1);
  float* Sc = sScale + wave * GT;

  for (int h = 0; h < H; ++h) {
    float qv[CP / 2];
#pragma unroll
    for (int s = 0; s < CP / 2; ++s) {
      const int k = 2 * s + lh;
      qv[s] = (row_ok && k < C) ? proj[(rb + i) * ldp + h * C + k] * scale : 0.f;
    }
    float m = -INFINITY, l = 0.f;
    f32x16 acc[NCTC];
#pragma unroll
    for (int c = 0; c < NCTC; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    for (int j0 = 0; j0 < N; j0 += GT) {
      __syncthreads();  // the previous tile's operands are consumed
      TR_STAGE_KV()
      const unsigned word = row_ok ? bits[(rb + i) * W + j0 / 32] : 0u;
      __syncthreads();

      f32x16 st;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
      for (int s = 0; s < CP / 2; ++s)
        if (2 * s < C) st = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[li * (CP + 1) + 2 * s + lh], qv[s], st, 0, 0, 0);

      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if ((word >> acc_row(r, lh)) & 1u) tmax = fmaxf(tmax, st[r]);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
      const float m_new = fmaxf(m, tmax);
      const float rescale = m_new == -INFINITY ? 1.f : expf(m - m_new);
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jj = acc_row(r, lh);
        const float p = ((word >> jj) & 1u) ? expf(st[r] - m_new) : 0.f;
        ps += p;
        P[li * (GT + 1) + jj] = p;
      }
      ps += __shfl_xor(ps, 32);
      l = fmaf(l, rescale, ps);
      m = m_new;
      if (lh == 0) Sc[li] = rescale;
      __syncthreads();

#pragma unroll
      for (int c = 0; c < NCTC; ++c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] *= Sc[acc_row(r, lh)];
        mma32(acc[c], P, GT + 1, 1, sV + c * 32, CP + 1, 1, GT, li, lh);
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
// dense backward, by row block (the forward's organisation): delta[i,h] = sum_j P dP, then dQ = scale sum_j dS K_j
// into gp[:, h C ...].  Lane (li, lh) holds q and dO of row li as the B operands of S^T = K Q^T and dP^T = V dO^T.
// ---------------------------------------------------------------------------
template <int NCTC>
__global__ __launch_bounds__(256) void k_tr_dense_dq(const unsigned* __restrict__ bits, const float* __restrict__ proj,
                                                     int ldp, const float* __restrict__ dO,
                                                     const float* __restrict__ row_m, const float* __restrict__ row_l,
                                                     float* __restrict__ delta, float* __restrict__ gp, int N, int H,
                                                     int C, float scale) {
  constexpr int CP = 32 * NCTC;
  __shared__ float sK[GT * (CP + 1)];       // [j][c]
  __shared__ float sV[GT * (CP + 1)];       // [j][c]
  __shared__ float sDS[4 * GT * (GT + 1)];  // per wave [i][j]
  const int b = blockIdx.y, i0 = blockIdx.x * 128;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int HC = H * C, W = (N + 31) / 32;
  const int i = i0 + wave * 32 + li;
  const bool row_ok = i < N;
  const size_t rb = (size_t)b * N;
  float* DS = sDS + wave * GT * (GT + 1);

  for (int h = 0; h < H; ++h) {
    float qv[CP / 2], dov[CP / 2];
#pragma unroll
    for (int s = 0; s < CP / 2; ++s) {
      const int k = 2 * s + lh;
      const bool ok = row_ok && k < C;
      qv[s] = ok ? proj[(rb + i) * ldp + h * C + k] * scale : 0.f;
      dov[s] = ok ? dO[(rb + i) * HC + h * C + k] : 0.f;
    }
    const float m = row_ok ? row_m[(rb + i) * H + h] : 0.f;
    const float l = row_ok ? row_l[(rb + i) * H + h] : 0.f;
    float dl = 0.f;
    f32x16 acc[NCTC];
#pragma unroll
    for (int c = 0; c < NCTC; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    for (int sweep = 0; sweep < 2; ++sweep) {
      for (int j0 = 0; j0 < N; j0 += GT) {
        __syncthreads();
        TR_STAGE_KV()
        const unsigned word = row_ok ? bits[(rb + i) * W + j0 / 32] : 0u;
        __syncthreads();

        f32x16 st, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.f;
#pragma unroll
        for (int s = 0; s < CP / 2; ++s)
          if (2 * s < C) {
            st = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[li * (CP + 1) + 2 * s + lh], qv[s], st, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sV[li * (CP + 1) + 2 * s + lh], dov[s], dp, 0, 0, 0);
          }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int jj = acc_row(r, lh);
          const float p = ((word >> jj) & 1u) ? expf(st[r] - m) / l : 0.f;  // on: l > 0
          if (sweep == 0)
            dl = fmaf(p, dp[r], dl);
          else
            DS[li * (GT + 1) + jj] = p * (dp[r] - dl);
        }
        if (sweep == 0) continue;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NCTC; ++c) mma32(acc[c], DS, GT + 1, 1, sK + c * 32, CP + 1, 1, GT, li, lh);
      }
      if (sweep == 0) {
        dl += __shfl_xor(dl, 32);
        if (row_ok && lh == 0) delta[(rb + i) * H + h] = dl;
      }
    }

#pragma unroll
    for (int c = 0; c < NCTC; ++c) {
      const int cc = c * 32 + li;
      if (cc >= C) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ii = i0 + wave * 32 + acc_row(r, lh);
        if (ii < N) gp[(rb + ii) * ldp + h * C + cc] = acc[c][r] * scale;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// dense backward, by neighbour block: workgroup = (128 neighbours j of one graph, 4 waves x 32), heads outer, row
// tiles of 32 inner.  Lane (li, lh) holds k and v of neighbour li as the B operands of S = Q K^T and dP = dO V^T, and
// after the products S and dP of j = li for the 16 rows acc_row(r, lh).  dK = dS^T (scale Q) into gp[:, H C + ...],
// dV = P^T dO into gp[:, 2 H C + ...]: each neighbour's sums stay in its wave, nothing is summed across workgroups.
// ---------------------------------------------------------------------------
template <int NCTC>
__global__ __launch_bounds__(256) void k_tr_dense_dkv(const unsigned* __restrict__ bits,
                                                      const float* __restrict__ proj, int ldp,
                                                      const float* __restrict__ dO, const float* __restrict__ row_m,
                                                      const float* __restrict__ row_l, const float* __restrict__ delta,
                                                      float* __restrict__ gp, int N, int H, int C, float scale) {
  constexpr int CP = 32 * NCTC;
  __shared__ float sQ[GT * (CP + 1)];      // [i][c], scaled
  __shared__ float sDO[GT * (CP + 1)];     // [i][c]
  __shared__ float sP[4 * GT * (GT + 1)];  // per wave [i][j]: P, then dS
  __shared__ float sRow[3 * GT];           // per row of the tile: m, l, delta
  __shared__ unsigned sBits[GT * 4];       // [i][wave]
  const int b = blockIdx.y, j0 = blockIdx.x * 128;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int HC = H * C, W = (N + 31) / 32;
  const int j = j0 + wave * 32 + li;  // the neighbour of this lane
  const bool j_ok = j < N;
  const size_t rb = (size_t)b * N;
  float* P = sP + wave * GT * (GT + 1);

  for (int h = 0; h < H; ++h) {
    float kv[CP / 2], vv[CP / 2];
#pragma unroll
    for (int s = 0; s < CP / 2; ++s) {
      const int k = 2 * s + lh;
      const bool ok = j_ok && k < C;
      kv[s] = ok ? proj[(rb + j) * ldp + HC + h * C + k] : 0.f;
      vv[s] = ok ? proj[(rb + j) * ldp + 2 * HC + h * C + k] : 0.f;
    }
    f32x16 accK[NCTC], accV[NCTC];
#pragma unroll
    for (int c = 0; c < NCTC; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) accK[c][r] = accV[c][r] = 0.f;

    for (int i0 = 0; i0 < N; i0 += GT) {
      __syncthreads();
      for (int e = threadIdx.x; e < GT * CP; e += 256) {
        const int k = e / CP, c = e - k * CP;
        const int i = i0 + k;
        const bool ok = i < N && c < C;
        sQ[k * (CP + 1) + c] = ok ? proj[(rb + i) * ldp + h * C + c] * scale : 0.f;
        sDO[k * (CP + 1) + c] = ok ? dO[(rb + i) * HC + h * C + c] : 0.f;
      }
      if (threadIdx.x < GT) {
        const int i = i0 + threadIdx.x;
        const bool ok = i < N;
        const size_t t = (rb + i) * H + h;
        sRow[threadIdx.x * 3 + 0] = ok ? row_m[t] : 0.f;
        sRow[threadIdx.x * 3 + 1] = ok ? row_l[t] : 0.f;
        sRow[threadIdx.x * 3 + 2] = ok ? delta[t] : 0.f;
      }
      if (threadIdx.x < GT * 4) {
        const int r = threadIdx.x >> 2, w = threadIdx.x & 3;
        const int i = i0 + r, jw = j0 / 32 + w;
        sBits[r * 4 + w] = (i < N && jw < W) ? bits[(rb + i) * W + jw] : 0u;
      }
      __syncthreads();

      f32x16 st, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.f;
#pragma unroll
      for (int s = 0; s < CP / 2; ++s)
        if (2 * s < C) {
          st = __builtin_amdgcn_mfma_f32_32x32x2f32(sQ[li * (CP + 1) + 2 * s + lh], kv[s], st, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_32x32x2f32(sDO[li * (CP + 1) + 2 * s + lh], vv[s], dp, 0, 0, 0);
        }
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = acc_row(r, lh);
        const float* row = sRow + rr * 3;
        const bool on = (sBits[rr * 4 + wave] >> li) & 1u;
        const float p = on ? expf(st[r] - row[0]) / row[1] : 0.f;  // on: l > 0
        ds[r] = p * (dp[r] - row[2]);
        P[rr * (GT + 1) + li] = p;
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < NCTC; ++c) mma32(accV[c], P, 1, GT + 1, sDO + c * 32, CP + 1, 1, GT, li, lh);
      __syncthreads();
#pragma unroll
      for (int r = 0; r < 16; ++r) P[acc_row(r, lh) * (GT + 1) + li] = ds[r];
      __syncthreads();
#pragma unroll
      for (int c = 0; c < NCTC; ++c) mma32(accK[c], P, 1, GT + 1, sQ + c * 32, CP + 1, 1, GT, li, lh);
    }

#pragma unroll
    for (int c = 0; c < NCTC; ++c) {
      const int cc = c * 32 + li;
      if (cc >= C) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jj = j0 + wave * 32 + acc_row(r, lh);
        if (jj >= N) continue;
        gp[(rb + jj) * ldp + HC + h * C + cc] = accK[c][r];
        gp[(rb + jj) * ldp + 2 * HC + h * C + cc] = accV[c][r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// sparse.  A group of G lanes per (destination i, head h); lane gl holds channels gl and gl + G (C <= 2 G).
// ---------------------------------------------------------------------------
// <a, row[h C ...]> over the group
template <int G>
__device__ __forceinline__ float group_dot(float a0, float a1, const float* __restrict__ row, int gl, int C) {
  float d = gl < C ? a0 * row[gl] : 0.f;
  if (gl + G < C) d = fmaf(a1, row[gl + G], d);
  return group_sum<G>(d);
}

// forward: one online-softmax pass over the CSR row
template <int G>
__global__ __launch_bounds__(256) void k_tr_csr_fwd(const int64_t* __restrict__ row_ptr,
                                                    const int64_t* __restrict__ col, const float* __restrict__ proj,
                                                    int ldp, float* __restrict__ o, float* __restrict__ row_m,
                                                    float* __restrict__ row_l, int64_t M, int H, int C, float scale) {
  const int64_t gid = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (gid >= M * H) return;
  const int gl = threadIdx.x & (G - 1), HC = H * C;
  const int64_t i = gid / H;
  const int h = (int)(gid - i * H);
  const float* qr = proj + (size_t)i * ldp + h * C;
  const float q0 = gl < C ? qr[gl] * scale : 0.f, q1 = gl + G < C ? qr[gl + G] * scale : 0.f;
  float m = -INFINITY, l = 0.f, a0 = 0.f, a1 = 0.f;
  for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
    const float* kr = proj + (size_t)col[e] * ldp + HC + h * C;
    const float* vr = kr + HC;
    const float s = group_dot<G>(q0, q1, kr, gl, C);
    const float m_new = fmaxf(m, s);
    const float rescale = expf(m - m_new), p = expf(s - m_new);
    l = fmaf(l, rescale, p);
    a0 = fmaf(a0, rescale, gl < C ? p * vr[gl] : 0.f);
    a1 = fmaf(a1, rescale, gl + G < C ? p * vr[gl + G] : 0.f);
    m = m_new;
  }
  float* orow = o + (size_t)i * HC + h * C;
  if (gl < C) orow[gl] = l > 0.f ? a0 / l : 0.f;
  if (gl + G < C) orow[gl + G] = l > 0.f ? a1 / l : 0.f;
  if (gl == 0) row_m[gid] = m, row_l[gid] = l;
}

// backward, per (destination i, head h): pass 1 delta = sum_e P dP; pass 2 alpha[e,h] = P, ds[e,h] = P (dP - delta)
// and dQ = scale sum_e dS k_src into gp[:, h C ...]
template <int G>
__global__ __launch_bounds__(256) void k_tr_csr_dq(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col,
                                                   const float* __restrict__ proj, int ldp,
                                                   const float* __restrict__ dO, const float* __restrict__ row_m,
                                                   const float* __restrict__ row_l, float* __restrict__ alpha,
                                                   float* __restrict__ ds, float* __restrict__ gp, int64_t M, int H,
                                                   int C, float scale) {
  const int64_t gid = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (gid >= M * H) return;
  const int gl = threadIdx.x & (G - 1), HC = H * C;
  const int64_t i = gid / H;
  const int h = (int)(gid - i * H);
  const float* qr = proj + (size_t)i * ldp + h * C;
  const float* gr = dO + (size_t)i * HC + h * C;
  const float q0 = gl < C ? qr[gl] * scale : 0.f, q1 = gl + G < C ? qr[gl + G] * scale : 0.f;
  const float g0 = gl < C ? gr[gl] : 0.f, g1 = gl + G < C ? gr[gl + G] : 0.f;
  const float m = row_m[gid], l = row_l[gid];
  const int64_t e0 = row_ptr[i], e1 = row_ptr[i + 1];
  float delta = 0.f;
  for (int64_t e = e0; e < e1; ++e) {
    const float* kr = proj + (size_t)col[e] * ldp + HC + h * C;
    const float p = expf(group_dot<G>(q0, q1, kr, gl, C) - m) / l;  // an entry of the row: l > 0
    delta = fmaf(p, group_dot<G>(g0, g1, kr + HC, gl, C), delta);
  }
  float a0 = 0.f, a1 = 0.f;
  for (int64_t e = e0; e < e1; ++e) {
    const float* kr = proj + (size_t)col[e] * ldp + HC + h * C;
    const float p = expf(group_dot<G>(q0, q1, kr, gl, C) - m) / l;
    const float d = p * (group_dot<G>(g0, g1, kr + HC, gl, C) - delta);
    if (gl == 0) alpha[e * H + h] = p, ds[e * H + h] = d;
    if (gl < C) a0 = fmaf(d, kr[gl], a0);
    if (gl + G < C) a1 = fmaf(d, kr[gl + G], a1);
  }
  float* out = gp + (size_t)i * ldp + h * C;
  if (gl < C) out[gl] = a0 * scale;
  if (gl + G < C) out[gl + G] = a1 * scale;
}

// backward, per (source j, column h*C + c) over its CSC column: dK = sum dS (scale q[dst]), dV = sum alpha dO[dst]
__global__ void k_tr_csr_dkv(const int64_t* __restrict__ col_ptr, const int64_t* __restrict__ rows,
                             const int64_t* __restrict__ perm, const float* __restrict__ alpha,
                             const float* __restrict__ ds, const float* __restrict__ proj, int ldp,
                             const float* __restrict__ dO, float* __restrict__ gp, int64_t M, int H, int C,
                             float scale) {
  const int HC = H * C;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= M * HC) return;
  const int64_t j = t / HC;
  const int cc = (int)(t - j * HC), h = cc / C;
  float ak = 0.f, av = 0.f;
  if (col_ptr)
    for (int64_t k = col_ptr[j]; k < col_ptr[j + 1]; ++k) {
      const int64_t e = perm[k], i = rows[k];
      ak = fmaf(ds[e * H + h], proj[(size_t)i * ldp + cc] * scale, ak);
      av = fmaf(alpha[e * H + h], dO[(size_t)i * HC + cc], av);
    }
  gp[(size_t)j * ldp + HC + cc] = ak;
  gp[(size_t)j * ldp + 2 * HC + cc] = av;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct Dims {
  int64_t R;
  int Fi, H, C, HC, D, P, root;
};

Dims dims(int64_t R, int Fi, int H, int C, int concat, int root) {
  Dims d;
  d.R = R, d.Fi = Fi, d.H = H, d.C = C, d.HC = H * C, d.D = concat ? H * C : C, d.root = root;
  d.P = 3 * d.HC + (root ? d.D : 0);
  return d;
}

bool unsupported(int64_t R, int Fi, int H, int C) {
  return Fi > 128 || (int64_t)H * C > 128 || R > (1 << 30);
}

// what the forward keeps for the backward: [q|k|v|r] [R,P], o [R,HC], row max / sum [R,H], gate [R], bits (dense)
struct Saved {
  size_t proj, o, m, l, gate, bits, total;
};
Saved saved_layout(const Dims& d, int64_t bit_words) {
  Saved s;
  Carve c;
  s.proj = c.take((size_t)d.R * d.P * 4), s.o = c.take((size_t)d.R * d.HC * 4);
  s.m = c.take((size_t)d.R * d.H * 4), s.l = c.take((size_t)d.R * d.H * 4);
  s.gate = c.take((size_t)d.R * 4), s.bits = c.take((size_t)bit_words * 4);
  s.total = c.at;
  return s;
}

// backward workspace: dO [R,HC], gp = [dQ|dK|dV|dR] [R,P], delta [R,H] (dense), t [R,3D] (gate), alpha, ds [E,H]
// (sparse), slabs for the weight gradient and the column sums
struct BwdWs {
  size_t dO, gp, delta, t, alpha, ds, slabs, total;
};
BwdWs bwd_ws(const Dims& d, int64_t E) {
  BwdWs w;
  int nsplit, kchunk;
  wgrad_split(d.R, &nsplit, &kchunk);
  const size_t slab_f = std::max<size_t>((size_t)nsplit * d.P * d.Fi,
                                         (size_t)colsum_slabs(d.R) * std::max(d.P, 3 * d.D));
  Carve c;
  w.dO = c.take((size_t)d.R * d.HC * 4), w.gp = c.take((size_t)d.R * d.P * 4);
  w.delta = c.take((size_t)d.R * d.H * 4), w.t = c.take((size_t)d.R * 3 * d.D * 4);
  w.alpha = c.take((size_t)E * d.H * 4), w.ds = c.take((size_t)E * d.H * 4);
  w.slabs = c.take(slab_f * 4);
  w.total = c.at;
  return w;
}

// [q|k|v|r] = x W_all^T + b_all
int project(const float* x, const float* w_all, const float* b_all, float* proj, const Dims& d, hipStream_t s) {
  return mm_xwt(x, w_all, b_all, proj, d.R, d.Fi, d.P, s);
}

int fwd_tail(const float* w_beta, float* out, const Saved& L, char* sv, const Dims& d, int concat, hipStream_t s) {
  hipLaunchKernelGGL(k_tr_out, dim3(blocks(d.R, 4)), dim3(256), 0, s, (const float*)(sv + L.o),
                     (const float*)(sv + L.proj), d.P, w_beta, out, (float*)(sv + L.gate), d.R, d.H, d.C, concat,
                     d.root);
  return gcm_launch_status();
}

int bwd_head(const float* g_out, const float* w_beta, float* g_w_beta, const Saved& L, const char* sv, const BwdWs& K,
             char* ws, const Dims& d, int concat, hipStream_t s) {
  float* t = (w_beta && g_w_beta) ? (float*)(ws + K.t) : nullptr;
  hipLaunchKernelGGL(k_tr_dout, dim3(blocks(d.R, 4)), dim3(256), 0, s, g_out, (const float*)(sv + L.o),
                     (const float*)(sv + L.proj), d.P, w_beta, (const float*)(sv + L.gate), (float*)(ws + K.dO),
                     (float*)(ws + K.gp), t, d.R, d.H, d.C, concat, d.root);
  int rc = gcm_launch_status();
  if (rc || !t) return rc;
  return colsum(t, d.R, 3 * d.D, g_w_beta, (float*)(ws + K.slabs), s);
}

// from the stacked projection gradient: g_b_all = its column sums, g_x = gp W_all, g_w_all = gp^T x
int bwd_tail(const float* x, const float* w_all, float* g_x, float* g_w_all, float* g_b_all, const BwdWs& K, char* ws,
             const Dims& d, hipStream_t s) {
  const float* gp = (const float*)(ws + K.gp);
  float* slabs = (float*)(ws + K.slabs);
  int rc;
  if (g_b_all && (rc = colsum(gp, d.R, d.P, g_b_all, slabs, s))) return rc;
  if (g_x && (rc = mm_gw(gp, w_all, g_x, d.R, d.Fi, d.P, s))) return rc;
  if (g_w_all && (rc = wgrad(gp, x, g_w_all, slabs, d.R, d.Fi, d.P, s))) return rc;
  return GCM_OK;
}

int dense_blocks(int N) { return (N + 127) / 128; }

// launch K<G> with the lane group of this C: n groups
#define TR_LAUNCH_GROUP(K, n, s, ...)                                                                       \
  if (C <= 8) hipLaunchKernelGGL(K<8>, dim3(blocks((n) * 8, 256)), dim3(256), 0, s, __VA_ARGS__);           \
  else if (C <= 16) hipLaunchKernelGGL(K<16>, dim3(blocks((n) * 16, 256)), dim3(256), 0, s, __VA_ARGS__);   \
  else if (C <= 32) hipLaunchKernelGGL(K<32>, dim3(blocks((n) * 32, 256)), dim3(256), 0, s, __VA_ARGS__);   \
  else hipLaunchKernelGGL(K<64>, dim3(blocks((n) * 64, 256)), dim3(256), 0, s, __VA_ARGS__);

}  // namespace
