// TransformerConv / DenseTransformerConv with edge features (PyG's edge_dim) forward and backward on gfx950.
//
// The layer of transformerconv.hip with e_k = W_e a_k (a_k [D] the feature of the term k = (j -> i), W_e [H*C, D])
// added to the key and to the value of every term:
//   s_k[h] = <q_i[h], k_j[h] + e_k[h]> / sqrt(C),  o_i[h] = sum_k alpha_k[h] (v_j[h] + e_k[h])
// W_e is linear and enters both lines linearly, so it is applied per node and never per term:
//   u_i[h] = W_e[h]^T q_i[h] / sqrt(C)          s_k[h] = <q_i[h], k_j[h]> / sqrt(C) + <u_i[h], a_k>
//   abar_i[h] = sum_k alpha_k[h] a_k            o_i[h] = sum_k alpha_k[h] v_j[h] + W_e[h] abar_i[h]
// and in the backward, with dO the gradient of o:
//   w_i[h] = W_e[h]^T dO_i[h]                   dP_k[h] = <dO_i[h], v_j[h]> + <w_i[h], a_k>
//   delta_i = sum_k P dP / sum_k P, dS = P (dP - delta)     b_i[h] = sum_k dS_k[h] a_k / sqrt(C)
//   dq_i[h] += W_e[h] b_i[h]                    g_a_k = sum_h (dS_k[h] u_i[h] + alpha_k[h] w_i[h])
//   g_W_e[h] = sum_i (dO_i[h] abar_i[h]^T + q_i[h] b_i[h]^T)
// dK and dV keep their form.  Nothing per term is wider than D: no e_k, no k_j + e_k, no v_j + e_k is formed, and
// the dense kernels write no score.  u, abar, w, b are [rows, H, D].
//
// The kernels are transformerconv.hip's (transformer_common.h) with the edge terms added where a lane holds a score:
// sparse: the group of G lanes of a (destination, head) spreads the D columns of a_k over its lanes, so <u, a_k>
//   joins the group's one sum per score and abar / b are up to four accumulators a lane; the row pass of the backward
//   writes alpha and dS [E,H] as before, a pass per (entry, column) forms g_edge_attr from them through the
//   permutation, and the CSC pass for dK, dV is the edge-free one unchanged (it reads alpha and dS).
// dense: the tiling and the matrix-core products of k_tr_dense_fwd/dq/dkv; <u, a> and <w, a> are added to the lane's
//   scores and dP at the set bits of the bit image only, u and w of the block's rows are staged in LDS (the dq kernel
//   has no registers to spare at C = 128), abar and b accumulate in LDS, each entry owned by one lane.  g_edge_attr is
//   written by the row-block kernel: head 0 stores every entry (zero where there is no term), the heads after it add
//   at the terms, the same lane in the same order every time.  LDS is dynamic: up to 101 KB at C = 128, D = 32.
// The node-level products (u, w, W_e abar, W_e b) are small kernels; g_W_e is summed over fixed row chunks, then over
// the chunks in order.  No atomics.  Fi, H*C <= 128, D <= 32; any N.
#include "transformer_common.h"

namespace {

constexpr int EMAX = GCM_TRE_MAX_EDGE_DIM;

// out[i,h,d] = fac * sum_c src[i, h C + c] W_e[h C + c, d]     (u from q, w from dO)
__global__ __launch_bounds__(256) void k_tre_node_t(const float* __restrict__ src, int lds_, const float* __restrict__ w_e,
                                                    float* __restrict__ out, int64_t R, int H, int C, int D,
                                                    float fac) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= R * H * D) return;
  const int d = (int)(t % D);
  const int64_t ih = t / D;
  const int h = (int)(ih % H);
  const int64_t i = ih / H;
  const float* sr = src + (size_t)i * lds_ + h * C;
  const float* wr = w_e + (size_t)h * C * D + d;
  float a = 0.f;
  for (int c = 0; c < C; ++c) a = fmaf(sr[c], wr[(size_t)c * D], a);
  out[t] = a * fac;
}

// dst[i, h C + c] += sum_d W_e[h C + c, d] src[i,h,d]          (o += W_e abar, dQ += W_e b)
__global__ __launch_bounds__(256) void k_tre_node_add(const float* __restrict__ src, const float* __restrict__ w_e,
                                                      float* __restrict__ dst, int ldd, int64_t R, int H, int C,
                                                      int D) {
  const int HC = H * C;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= R * HC) return;
  const int cc = (int)(t % HC);
  const int64_t i = t / HC;
  const float* sr = src + ((size_t)i * H + cc / C) * D;
  const float* wr = w_e + (size_t)cc * D;
  float a = 0.f;
  for (int d = 0; d < D; ++d) a = fmaf(wr[d], sr[d], a);
  dst[(size_t)i * ldd + cc] += a;
}

// g_W_e, stage 1: slab[chunk][h C + c, d] = sum over the chunk's rows of dO abar + q b
__global__ __launch_bounds__(256) void k_tre_gwe_part(const float* __restrict__ dO, const float* __restrict__ proj,
                                                      int ldp, const float* __restrict__ abar,
                                                      const float* __restrict__ b, float* __restrict__ slabs,
                                                      int64_t R, int64_t chunk, int H, int C, int D) {
  const int HC = H * C;
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = r0 + chunk < R ? r0 + chunk : R;
  for (int e = threadIdx.x; e < HC * D; e += 256) {
    const int cc = e / D, d = e - cc * D, h = cc / C;
    float a = 0.f;
    for (int64_t i = r0; i < r1; ++i) {
      const size_t n = ((size_t)i * H + h) * D + d;
      a = fmaf(dO[(size_t)i * HC + cc], abar[n], a);
      a = fmaf(proj[(size_t)i * ldp + cc], b[n], a);
    }
    slabs[(size_t)blockIdx.x * HC * D + e] = a;
  }
}

// stage 2: the chunks in order
__global__ __launch_bounds__(256) void k_tre_gwe_sum(const float* __restrict__ slabs, float* __restrict__ g, int n,
                                                     int nchunk) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float a = 0.f;
  for (int k = 0; k < nchunk; ++k) a += slabs[(size_t)k * n + e];
  g[e] = a;
}

// s += v with the rounding error of the sum carried in c (Kahan): the sum is s - c
__device__ __forceinline__ void comp_add(float& s, float& c, float v) {
  const float y = v - c, t = s + y;
  c = (t - s) - y;
  s = t;
}

// delta = sum P dP / sum P from compensated sums.  sum P is 1 but for the rounding of the forward's running sum l, of
// order sqrt(n) ulp over a row of n terms; dividing by the sum of the very P that multiply (dP - delta) makes
// sum dS cancel to the rounding of its terms - which is all the key bias gradient (exactly 0) consists of: with
// delta = sum P dP alone it missed the tests' bound at a hub of 70 in-edges (2.8e-7 against 2.2e-7).
__device__ __forceinline__ float delta_of(float sd, float sdc, float sp, float spc) {
  const float den = sp - spc;
  return den > 0.f ? (sd - sdc) / den : 0.f;
}

// ---------------------------------------------------------------------------
// sparse.  k_tr_csr_fwd<G> / k_tr_csr_dq<G> with the edge terms: lane gl of the group holds columns gl, gl + G, ... of
// u (w) and of abar (b).
// ---------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(256) void k_tre_csr_fwd(const int64_t* __restrict__ row_ptr,
                                                     const int64_t* __restrict__ col,
                                                     const int64_t* __restrict__ csr_perm,
                                                     const float* __restrict__ ea, const float* __restrict__ proj,
                                                     int ldp, const float* __restrict__ u, float* __restrict__ o,
                                                     float* __restrict__ abar, float* __restrict__ row_m,
                                                     float* __restrict__ row_l, int64_t M, int H, int C, int D,
                                                     float scale) {
  constexpr int NT = (EMAX + G - 1) / G;
  const int64_t gid = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (gid >= M * H) return;
  const int gl = threadIdx.x & (G - 1), HC = H * C;
  const int64_t i = gid / H;
  const int h = (int)(gid - i * H);
  const float* qr = proj + (size_t)i * ldp + h * C;
  const float q0 = gl < C ? qr[gl] * scale : 0.f, q1 = gl + G < C ? qr[gl + G] * scale : 0.f;
  float uu[NT], ab[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int d = gl + t * G;
    uu[t] = d < D ? u[(size_t)gid * D + d] : 0.f;
    ab[t] = 0.f;
  }
  float m = -INFINITY, l = 0.f, a0 = 0.f, a1 = 0.f;
  for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
    const float* kr = proj + (size_t)col[e] * ldp + HC + h * C;
    const float* vr = kr + HC;
    const float* ar = ea + (size_t)(csr_perm ? csr_perm[e] : e) * D;
    float av[NT];
    float part = gl < C ? q0 * kr[gl] : 0.f;
    if (gl + G < C) part = fmaf(q1, kr[gl + G], part);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int d = gl + t * G;
      av[t] = d < D ? ar[d] : 0.f;
      part = fmaf(uu[t], av[t], part);
    }
    const float s = group_sum<G>(part);
    const float m_new = fmaxf(m, s);
    const float rescale = expf(m - m_new), p = expf(s - m_new);
    l = fmaf(l, rescale, p);
    a0 = fmaf(a0, rescale, gl < C ? p * vr[gl] : 0.f);
    a1 = fmaf(a1, rescale, gl + G < C ? p * vr[gl + G] : 0.f);
#pragma unroll
    for (int t = 0; t < NT; ++t) ab[t] = fmaf(ab[t], rescale, p * av[t]);
    m = m_new;
  }
  float* orow = o + (size_t)i * HC + h * C;
  if (gl < C) orow[gl] = l > 0.f ? a0 / l : 0.f;
  if (gl + G < C) orow[gl + G] = l > 0.f ? a1 / l : 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int d = gl + t * G;
    if (d < D) abar[(size_t)gid * D + d] = l > 0.f ? ab[t] / l : 0.f;
  }
  if (gl == 0) row_m[gid] = m, row_l[gid] = l;
}

// backward, per (destination i, head h): pass 1 delta = sum_e P dP / sum_e P; pass 2 alpha[e,h] = P, ds[e,h] =
// P (dP - delta), dQ = scale sum_e dS k_src into gp[:, h C ...] and b = scale sum_e dS a_e
template <int G>
__global__ __launch_bounds__(256) void k_tre_csr_dq(const int64_t* __restrict__ row_ptr,
                                                    const int64_t* __restrict__ col,
                                                    const int64_t* __restrict__ csr_perm,
                                                    const float* __restrict__ ea, const float* __restrict__ proj,
                                                    int ldp, const float* __restrict__ dO,
                                                    const float* __restrict__ u, const float* __restrict__ w,
                                                    const float* __restrict__ row_m, const float* __restrict__ row_l,
                                                    float* __restrict__ alpha, float* __restrict__ ds,
                                                    float* __restrict__ gp, float* __restrict__ b, int64_t M, int H,
                                                    int C, int D, float scale) {
  constexpr int NT = (EMAX + G - 1) / G;
  const int64_t gid = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (gid >= M * H) return;
  const int gl = threadIdx.x & (G - 1), HC = H * C;
  const int64_t i = gid / H;
  const int h = (int)(gid - i * H);
  const float* qr = proj + (size_t)i * ldp + h * C;
  const float* gr = dO + (size_t)i * HC + h * C;
  const float q0 = gl < C ? qr[gl] * scale : 0.f, q1 = gl + G < C ? qr[gl + G] * scale : 0.f;
  const float g0 = gl < C ? gr[gl] : 0.f, g1 = gl + G < C ? gr[gl + G] : 0.f;
  float uu[NT], ww[NT], bb[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int d = gl + t * G;
    uu[t] = d < D ? u[(size_t)gid * D + d] : 0.f;
    ww[t] = d < D ? w[(size_t)gid * D + d] : 0.f;
    bb[t] = 0.f;
  }
  const float m = row_m[gid], l = row_l[gid];
  const int64_t e0 = row_ptr[i], e1 = row_ptr[i + 1];
  float delta = 0.f, sd = 0.f, sdc = 0.f, sp = 0.f, spc = 0.f;
  for (int pass = 0; pass < 2; ++pass) {
    float a0 = 0.f, a1 = 0.f;
    for (int64_t e = e0; e < e1; ++e) {
      const float* kr = proj + (size_t)col[e] * ldp + HC + h * C;
      const float* vr = kr + HC;
      const float* ar = ea + (size_t)(csr_perm ? csr_perm[e] : e) * D;
      float av[NT];
      float ps = gl < C ? q0 * kr[gl] : 0.f, pd = gl < C ? g0 * vr[gl] : 0.f;
      if (gl + G < C) ps = fmaf(q1, kr[gl + G], ps), pd = fmaf(g1, vr[gl + G], pd);
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int d = gl + t * G;
        av[t] = d < D ? ar[d] : 0.f;
        ps = fmaf(uu[t], av[t], ps);
        pd = fmaf(ww[t], av[t], pd);
      }
      const float p = expf(group_sum<G>(ps) - m) / l;  // an entry of the row: l > 0
      const float dp = group_sum<G>(pd);
      if (pass == 0) {
        comp_add(sd, sdc, p * dp);
        comp_add(sp, spc, p);
        continue;
      }
      const float dv = p * (dp - delta);
      if (gl == 0) alpha[e * H + h] = p, ds[e * H + h] = dv;
      if (gl < C) a0 = fmaf(dv, kr[gl], a0);
      if (gl + G < C) a1 = fmaf(dv, kr[gl + G], a1);
#pragma unroll
      for (int t = 0; t < NT; ++t) bb[t] = fmaf(dv, av[t], bb[t]);
    }
    if (pass == 0) {
      delta = delta_of(sd, sdc, sp, spc);
      continue;
    }
    float* out = gp + (size_t)i * ldp + h * C;
    if (gl < C) out[gl] = a0 * scale;
    if (gl + G < C) out[gl + G] = a1 * scale;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int d = gl + t * G;
      if (d < D) b[(size_t)gid * D + d] = bb[t] * scale;
    }
  }
}

// g_edge_attr, per (entry, column): entry k of the CSC is CSR entry perm[k] with sink rows[k]; its feature stands at
// csr_perm[perm[k]] of the caller's list.  g = sum_h dS u + alpha w.
__global__ __launch_bounds__(256) void k_tre_csr_gea(const int64_t* __restrict__ rows, const int64_t* __restrict__ perm,
                                                     const int64_t* __restrict__ csr_perm,
                                                     const float* __restrict__ alpha, const float* __restrict__ ds,
                                                     const float* __restrict__ u, const float* __restrict__ w,
                                                     float* __restrict__ g_ea, int64_t E, int H, int D) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= E * D) return;
  const int64_t k = t / D;
  const int d = (int)(t - k * D);
  const int64_t e = perm[k], i = rows[k];
  float a = 0.f;
  for (int h = 0; h < H; ++h) {
    const size_t n = ((size_t)i * H + h) * D + d;
    a = fmaf(ds[e * H + h], u[n], a);
    a = fmaf(alpha[e * H + h], w[n], a);
  }
  g_ea[(size_t)(csr_perm ? csr_perm[e] : e) * D + d] = a;
}

// ---------------------------------------------------------------------------
// dense.  The edge-free kernels' tiling; LDS is dynamic.  es = D | 1: the stride of a row of u / w / abar / b in LDS.
// ---------------------------------------------------------------------------
// <urow, a[0..D)>
__device__ __forceinline__ float edge_dot(const float* urow, const float* __restrict__ a, int D) {
  float t = 0.f;
  for (int d = 0; d < D; ++d) t = fmaf(urow[d], a[d], t);
  return t;
}

// stage the [128, D] rows i0.. of head h of a node array into LDS (zero past N)
__device__ __forceinline__ void stage_node(float* dst, const float* __restrict__ src, size_t rb, int i0, int nrows,
                                           int N, int H, int h, int D, int es) {
  for (int e = threadIdx.x; e < nrows * D; e += 256) {
    const int r = e / D, d = e - r * D;
    const int ii = i0 + r;
    dst[r * es + d] = ii < N ? src[((rb + ii) * H + h) * D + d] : 0.f;
  }
}

template <int NCTC>
__global__ __launch_bounds__(256) void k_tre_dense_fwd(const unsigned* __restrict__ bits,
                                                       const float* __restrict__ proj, int ldp,
                                                       const float* __restrict__ ea, const float* __restrict__ u,
                                                       float* __restrict__ o, float* __restrict__ abar,
                                                       float* __restrict__ row_m, float* __restrict__ row_l, int N,
                                                       int H, int C, int D, float scale) {
  constexpr int CP = 32 * NCTC;
  extern __shared__ float lds[];
  const int es = D | 1;
  float* sK = lds;                           // [j][c]
  float* sV = sK + GT * (CP + 1);            // [j][c]
  float* sP = sV + GT * (CP + 1);            // per wave [i][j]
  float* sScale = sP + 4 * GT * (GT + 1);    // per wave, per row: the rescale of this tile, then l
  float* sU = sScale + 4 * GT;               // [128][es]
  float* sA = sU + 128 * es;                 // [128][es]: abar, entry (row, d) owned by lane (row, d & 1)
  const int b = blockIdx.y, i0 = blockIdx.x * 128;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int HC = H * C, W = (N + 31) / 32;
  const int rl = wave * 32 + li;
  const int i = i0 + rl;  // the row this lane scores
  const bool row_ok = i < N;
  const size_t rb = (size_t)b * N;
  float* P = sP + wave * GT * (GT + 1);
  float* Sc = sScale + wave * GT;
  const float* urow = sU + rl * es;
  float* arow = sA + rl * es;

  for (int h = 0; h < H; ++h) {
    float qv[CP / 2];
#pragma unroll
    for (int s = 0; s < CP / 2; ++s) {
      const int k = 2 * s + lh;
      qv[s] = (row_ok && k < C) ? proj[(rb + i) * ldp + h * C + k] * scale : 0.f;
    }
    stage_node(sU, u, rb, i0, 128, N, H, h, D, es);
    for (int e = threadIdx.x; e < 128 * es; e += 256) sA[e] = 0.f;
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
      const float* at = ea + ((rb + (row_ok ? i : 0)) * N + j0) * D;  // read at set bits only
      __syncthreads();

      f32x16 st;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
      for (int s = 0; s < CP / 2; ++s)
        if (2 * s < C) st = __builtin_amdgcn_mfma_f32_32x32x2f32(sK[li * (CP + 1) + 2 * s + lh], qv[s], st, 0, 0, 0);

      float tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jj = acc_row(r, lh);
        if ((word >> jj) & 1u) {
          st[r] += edge_dot(urow, at + (size_t)jj * D, D);
          tmax = fmaxf(tmax, st[r]);
        }
      }
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

      for (int d = lh; d < D; d += 2) {
        float a = arow[d] * rescale;
        for (unsigned wv = word; wv; wv &= wv - 1) {
          const int jj = __ffs((int)wv) - 1;
          a = fmaf(P[li * (GT + 1) + jj], at[(size_t)jj * D + d], a);
        }
        arow[d] = a;
      }
#pragma unroll
      for (int c = 0; c < NCTC; ++c) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] *= Sc[acc_row(r, lh)];
        mma32(acc[c], P, GT + 1, 1, sV + c * 32, CP + 1, 1, GT, li, lh);
      }
    }

    if (row_ok)
      for (int d = lh; d < D; d += 2) abar[((rb + i) * H + h) * D + d] = l > 0.f ? arow[d] / l : 0.f;
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

// by row block: delta, dQ (without W_e b), b and g_edge_attr
template <int NCTC>
__global__ __launch_bounds__(256) void k_tre_dense_dq(const unsigned* __restrict__ bits, const float* __restrict__ proj,
                                                      int ldp, const float* __restrict__ ea,
                                                      const float* __restrict__ u, const float* __restrict__ w,
                                                      const float* __restrict__ dO, const float* __restrict__ row_m,
                                                      const float* __restrict__ row_l, float* __restrict__ delta,
                                                      float* __restrict__ gp, float* __restrict__ bout,
                                                      float* __restrict__ g_ea, int N, int H, int C, int D,
                                                      float scale) {
  constexpr int CP = 32 * NCTC;
  extern __shared__ float lds[];
  const int es = D | 1;
  float* sK = lds;                          // [j][c]
  float* sV = sK + GT * (CP + 1);           // [j][c]
  float* sDS = sV + GT * (CP + 1);          // per wave [i][j]
  float* sU = sDS + 4 * GT * (GT + 1);      // [128][es]
  float* sW = sU + 128 * es;                // [128][es]
  float* sB = sW + 128 * es;                // [128][es]: b, entry (row, d) owned by lane (row, d & 1)
  const int b = blockIdx.y, i0 = blockIdx.x * 128;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int HC = H * C, W = (N + 31) / 32;
  const int rl = wave * 32 + li;
  const int i = i0 + rl;
  const bool row_ok = i < N;
  const size_t rb = (size_t)b * N;
  float* DS = sDS + wave * GT * (GT + 1);
  const float* urow = sU + rl * es;
  const float* wrow = sW + rl * es;
  float* brow = sB + rl * es;

  for (int h = 0; h < H; ++h) {
    float qv[CP / 2], dov[CP / 2];
#pragma unroll
    for (int s = 0; s < CP / 2; ++s) {
      const int k = 2 * s + lh;
      const bool ok = row_ok && k < C;
      qv[s] = ok ? proj[(rb + i) * ldp + h * C + k] * scale : 0.f;
      dov[s] = ok ? dO[(rb + i) * HC + h * C + k] : 0.f;
    }
    __syncthreads();  // the previous head's u, w, b are done with
    stage_node(sU, u, rb, i0, 128, N, H, h, D, es);
    stage_node(sW, w, rb, i0, 128, N, H, h, D, es);
    for (int e = threadIdx.x; e < 128 * es; e += 256) sB[e] = 0.f;
    const float m = row_ok ? row_m[(rb + i) * H + h] : 0.f;
    const float l = row_ok ? row_l[(rb + i) * H + h] : 0.f;
    float dl = 0.f, dlc = 0.f, sp = 0.f, spc = 0.f;
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
        const size_t tile = ((rb + (row_ok ? i : 0)) * N + j0) * D;
        const float* at = ea + tile;  // read at set bits only
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
          const bool on = (word >> jj) & 1u;
          float p = 0.f, dpe = 0.f;
          if (on) {
            const float* a = at + (size_t)jj * D;
            p = expf(st[r] + edge_dot(urow, a, D) - m) / l;  // on: l > 0
            dpe = dp[r] + edge_dot(wrow, a, D);
          }
          if (sweep == 0) {
            if (on) comp_add(dl, dlc, p * dpe), comp_add(sp, spc, p);
            continue;
          }
          const float dv = p * (dpe - dl);
          DS[li * (GT + 1) + jj] = dv;
          if (g_ea && row_ok && j0 + jj < N) {
            float* gr = g_ea + tile + (size_t)jj * D;
            if (on)
              for (int d = 0; d < D; ++d) {
                const float v = fmaf(dv, urow[d], p * wrow[d]);
                gr[d] = h == 0 ? v : gr[d] + v;
              }
            else if (h == 0)
              for (int d = 0; d < D; ++d) gr[d] = 0.f;
          }
        }
        if (sweep == 0) continue;
        __syncthreads();
        for (int d = lh; d < D; d += 2) {
          float a = brow[d];
          for (unsigned wv = word; wv; wv &= wv - 1) {
            const int jj = __ffs((int)wv) - 1;
            a = fmaf(DS[li * (GT + 1) + jj], at[(size_t)jj * D + d], a);
          }
          brow[d] = a;
        }
#pragma unroll
        for (int c = 0; c < NCTC; ++c) mma32(acc[c], DS, GT + 1, 1, sK + c * 32, CP + 1, 1, GT, li, lh);
      }
      if (sweep == 0) {
        dl -= dlc, sp -= spc;
        dl += __shfl_xor(dl, 32), sp += __shfl_xor(sp, 32);
        dl = sp > 0.f ? dl / sp : 0.f;
        if (row_ok && lh == 0) delta[(rb + i) * H + h] = dl;
      }
    }

    if (row_ok)
      for (int d = lh; d < D; d += 2) bout[((rb + i) * H + h) * D + d] = brow[d] * scale;
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

// by neighbour block: dK, dV, with the edge terms in the recomputed P and dP
template <int NCTC>
__global__ __launch_bounds__(256) void k_tre_dense_dkv(const unsigned* __restrict__ bits,
                                                       const float* __restrict__ proj, int ldp,
                                                       const float* __restrict__ ea, const float* __restrict__ u,
                                                       const float* __restrict__ w, const float* __restrict__ dO,
                                                       const float* __restrict__ row_m,
                                                       const float* __restrict__ row_l,
                                                       const float* __restrict__ delta, float* __restrict__ gp, int N,
                                                       int H, int C, int D, float scale) {
  constexpr int CP = 32 * NCTC;
  extern __shared__ float lds[];
  const int es = D | 1;
  float* sQ = lds;                              // [i][c], scaled
  float* sDO = sQ + GT * (CP + 1);              // [i][c]
  float* sP = sDO + GT * (CP + 1);              // per wave [i][j]: P, then dS
  float* sRow = sP + 4 * GT * (GT + 1);         // per row of the tile: m, l, delta
  unsigned* sBits = (unsigned*)(sRow + 3 * GT); // [i][wave]
  float* sU = (float*)(sBits + GT * 4);         // [32][es]
  float* sW = sU + GT * es;                     // [32][es]
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
      stage_node(sU, u, rb, i0, GT, N, H, h, D, es);
      stage_node(sW, w, rb, i0, GT, N, H, h, D, es);
      if (threadIdx.x < GT) {
        const int i = i0 + threadIdx.x;
        const bool ok = i < N;
        const size_t t = (rb + (ok ? i : 0)) * H + h;
        sRow[threadIdx.x * 3 + 0] = ok ? row_m[t] : 0.f;
        sRow[threadIdx.x * 3 + 1] = ok ? row_l[t] : 0.f;
        sRow[threadIdx.x * 3 + 2] = ok ? delta[t] : 0.f;
      }
      if (threadIdx.x < GT * 4) {
        const int r = threadIdx.x >> 2, wq = threadIdx.x & 3;
        const int i = i0 + r, jw = j0 / 32 + wq;
        sBits[r * 4 + wq] = (i < N && jw < W) ? bits[(rb + i) * W + jw] : 0u;
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
        float p = 0.f, dpe = 0.f;
        if (on) {  // on: row i0 + rr < N, j < N, l > 0
          const float* a = ea + ((rb + i0 + rr) * N + j) * D;
          p = expf(st[r] + edge_dot(sU + rr * es, a, D) - row[0]) / row[1];
          dpe = dp[r] + edge_dot(sW + rr * es, a, D);
        }
        ds[r] = p * (dpe - row[2]);
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
// host side
// ---------------------------------------------------------------------------
bool unsupported_e(int64_t R, int Fi, int H, int C, int D) { return unsupported(R, Fi, H, C) || D > EMAX; }

// the edge-free layouts, then u and abar [R,H,D] (saved) / w and b [R,H,D] and the g_W_e slabs (workspace)
struct SavedE {
  Saved base;
  size_t u, abar, total;
};
SavedE saved_e(const Dims& d, int D, int64_t bit_words) {
  SavedE s;
  s.base = saved_layout(d, bit_words);
  Carve c;
  c.at = s.base.total;
  s.u = c.take((size_t)d.R * d.H * D * 4), s.abar = c.take((size_t)d.R * d.H * D * 4);
  s.total = c.at;
  return s;
}

// g_W_e is summed over chunks of at least 64 rows, at most 512 of them
void gwe_plan(int64_t R, int64_t* chunk, int* nchunk) {
  *chunk = std::max<int64_t>(64, (R + 511) / 512);
  *nchunk = (int)((R + *chunk - 1) / *chunk);
}

struct BwdWsE {
  BwdWs base;
  size_t w, b, slabs, wslabs, total;
};
BwdWsE bwd_ws_e(const Dims& d, int D, int64_t E) {
  BwdWsE k;
  k.base = bwd_ws(d, E);
  int64_t chunk;
  int nchunk;
  gwe_plan(d.R, &chunk, &nchunk);
  Carve c;
  c.at = k.base.total;
  k.w = c.take((size_t)d.R * d.H * D * 4), k.b = c.take((size_t)d.R * d.H * D * 4);
  k.slabs = c.take((size_t)nchunk * d.HC * D * 4);
  int nsplit, kchunk;
  wgrad_split64(d.R, &nsplit, &kchunk);
  k.wslabs = c.take((size_t)nsplit * d.P * d.Fi * 4);
  k.total = c.at;
  return k;
}

int node_t(const float* src, int ld, const float* w_e, float* out, const Dims& d, int D, float fac, hipStream_t s) {
  hipLaunchKernelGGL(k_tre_node_t, dim3(blocks(d.R * d.H * D, 256)), dim3(256), 0, s, src, ld, w_e, out, d.R, d.H, d.C,
                     D, fac);
  return gcm_launch_status();
}

int node_add(const float* src, const float* w_e, float* dst, int ldd, const Dims& d, int D, hipStream_t s) {
  hipLaunchKernelGGL(k_tre_node_add, dim3(blocks(d.R * d.HC, 256)), dim3(256), 0, s, src, w_e, dst, ldd, d.R, d.H, d.C,
                     D);
  return gcm_launch_status();
}

int gwe(const float* dO, const float* proj, const float* abar, const float* b, float* slabs, float* g_w_e,
        const Dims& d, int D, hipStream_t s) {
  int64_t chunk;
  int nchunk;
  gwe_plan(d.R, &chunk, &nchunk);
  hipLaunchKernelGGL(k_tre_gwe_part, dim3(nchunk), dim3(256), 0, s, dO, proj, d.P, abar, b, slabs, d.R, chunk, d.H, d.C,
                     D);
  int rc = gcm_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(k_tre_gwe_sum, dim3(blocks(d.HC * D, 256)), dim3(256), 0, s, (const float*)slabs, g_w_e,
                     d.HC * D, nchunk);
  return gcm_launch_status();
}

// bwd_tail with the weight gradient split into chains of 64 rows (wgrad_split64): one chain over the 260 rows of a
// test shape put g_w_query at 1.01 of the tests' bound (1.43e-5 against 1.42e-5)
int bwd_tail_e(const float* x, const float* w_all, float* g_x, float* g_w_all, float* g_b_all, const BwdWsE& K, char* ws,
               const Dims& d, hipStream_t s) {
  const float* gp = (const float*)(ws + K.base.gp);
  int rc;
  if (g_b_all && (rc = colsum(gp, d.R, d.P, g_b_all, (float*)(ws + K.base.slabs), s))) return rc;
  if (g_x && (rc = mm_gw(gp, w_all, g_x, d.R, d.Fi, d.P, s))) return rc;
  if (g_w_all && (rc = wgrad(gp, x, g_w_all, (float*)(ws + K.wslabs), d.R, d.Fi, d.P, s, wgrad_split64))) return rc;
  return GCM_OK;
}

// dynamic LDS of the dense kernels, in bytes
size_t lds_fwd(int nctc, int D) {
  return 4 * ((size_t)2 * GT * (32 * nctc + 1) + 4 * GT * (GT + 1) + 4 * GT + 2 * 128 * (D | 1));
}
size_t lds_dq(int nctc, int D) {
  return 4 * ((size_t)2 * GT * (32 * nctc + 1) + 4 * GT * (GT + 1) + 3 * 128 * (D | 1));
}
size_t lds_dkv(int nctc, int D) {
  return 4 * ((size_t)2 * GT * (32 * nctc + 1) + 4 * GT * (GT + 1) + 3 * GT + 4 * GT + 2 * GT * (D | 1));
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: DenseTransformerConv with edge features
// ---------------------------------------------------------------------------
#define TRE_DIMS_OK(R0) ((R0) > 0 && Fi > 0 && H > 0 && C > 0 && D > 0)

extern "C" size_t gcm_dense_transformer_edge_fwd_workspace_bytes(int B, int N, int Fi, int H, int C, int D, int concat,
                                                                 int root) {
  if (B <= 0 || N <= 0 || Fi <= 0 || H <= 0 || C <= 0 || D <= 0) return 0;
  const int64_t R = (int64_t)B * N;
  return saved_e(dims(R, Fi, H, C, concat, root), D, R * ((N + 31) / 32)).total;
}

extern "C" int gcm_dense_transformer_edge_fwd(const float* x, const float* adj, const float* edge_attr,
                                              const float* w_all, const float* b_all, const float* w_e,
                                              const float* w_beta, float* out, void* saved, size_t saved_bytes, int B,
                                              int N, int Fi, int H, int C, int D, int concat, int root, int add_loop,
                                              gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && edge_attr && w_all && b_all && w_e && out && saved);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && H > 0 && C > 0 && D > 0);
  GCM_REQUIRE(root || !w_beta);
  const int64_t R = (int64_t)B * N;
  if (unsupported_e(R, Fi, H, C, D) || B > 65535) return GCM_EUNSUPPORTED;
  const Dims d = dims(R, Fi, H, C, concat, root);
  const int W = (N + 31) / 32;
  const SavedE L = saved_e(d, D, R * W);
  GCM_REQUIRE(saved_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* sv = (char*)saved;
  unsigned* bits = (unsigned*)(sv + L.base.bits);
  float* proj = (float*)(sv + L.base.proj);
  float* u = (float*)(sv + L.u);
  float* abar = (float*)(sv + L.abar);
  float* o = (float*)(sv + L.base.o);
  const float scale = 1.f / sqrtf((float)C);
  int rc = mask_bits(adj, bits, R, N, W, add_loop, s);
  if (rc || (rc = project(x, w_all, b_all, proj, d, s))) return rc;
  if ((rc = node_t(proj, d.P, w_e, u, d, D, scale, s))) return rc;
  const dim3 grid(dense_blocks(N), B);
  dispatch_nct((C + 31) / 32, [&](auto n) {
    auto kern = k_tre_dense_fwd<n()>;
    const size_t lds = lds_fwd(n(), D);
    gcm_allow_dynamic_lds((const void*)kern, lds);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, (const unsigned*)bits, (const float*)proj, d.P, edge_attr,
                       (const float*)u, o, abar, (float*)(sv + L.base.m), (float*)(sv + L.base.l), N, H, C, D, scale);
  });
  if ((rc = gcm_launch_status())) return rc;
  if ((rc = node_add(abar, w_e, o, d.HC, d, D, s))) return rc;
  return fwd_tail(w_beta, out, L.base, sv, d, concat, s);
}

extern "C" size_t gcm_dense_transformer_edge_bwd_workspace_bytes(int B, int N, int Fi, int H, int C, int D, int concat,
                                                                 int root) {
  if (B <= 0 || N <= 0 || Fi <= 0 || H <= 0 || C <= 0 || D <= 0) return 0;
  return bwd_ws_e(dims((int64_t)B * N, Fi, H, C, concat, root), D, 0).total;
}

extern "C" int gcm_dense_transformer_edge_bwd(const float* g_out, const float* x, const float* edge_attr,
                                              const float* w_all, const float* w_e, const float* w_beta,
                                              const void* saved, float* g_x, float* g_w_all, float* g_b_all,
                                              float* g_w_e, float* g_w_beta, float* g_edge_attr, void* workspace,
                                              size_t workspace_bytes, int B, int N, int Fi, int H, int C, int D,
                                              int concat, int root, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && edge_attr && w_all && w_e && saved && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && H > 0 && C > 0 && D > 0);
  GCM_REQUIRE((root || !w_beta) && (w_beta || !g_w_beta));
  const int64_t R = (int64_t)B * N;
  if (unsupported_e(R, Fi, H, C, D) || B > 65535) return GCM_EUNSUPPORTED;
  const Dims d = dims(R, Fi, H, C, concat, root);
  const int W = (N + 31) / 32;
  const SavedE L = saved_e(d, D, R * W);
  const BwdWsE K = bwd_ws_e(d, D, 0);
  GCM_REQUIRE(workspace_bytes >= K.total);
  if (!g_x && !g_w_all && !g_b_all && !g_w_e && !g_w_beta && !g_edge_attr) return GCM_OK;
  hipStream_t s = (hipStream_t)stream;
  const char* sv = (const char*)saved;
  char* ws = (char*)workspace;
  int rc = bwd_head(g_out, w_beta, g_w_beta, L.base, sv, K.base, ws, d, concat, s);
  if (rc) return rc;
  const unsigned* bits = (const unsigned*)(sv + L.base.bits);
  const float* proj = (const float*)(sv + L.base.proj);
  const float* row_m = (const float*)(sv + L.base.m);
  const float* row_l = (const float*)(sv + L.base.l);
  const float* u = (const float*)(sv + L.u);
  const float* abar = (const float*)(sv + L.abar);
  const float* dO = (const float*)(ws + K.base.dO);
  float* delta = (float*)(ws + K.base.delta);
  float* gp = (float*)(ws + K.base.gp);
  float* w = (float*)(ws + K.w);
  float* b = (float*)(ws + K.b);
  const float scale = 1.f / sqrtf((float)C);
  if ((rc = node_t(dO, d.HC, w_e, w, d, D, 1.f, s))) return rc;
  const dim3 grid(dense_blocks(N), B);
  dispatch_nct((C + 31) / 32, [&](auto n) {
    auto kern = k_tre_dense_dq<n()>;
    const size_t lds = lds_dq(n(), D);
    gcm_allow_dynamic_lds((const void*)kern, lds);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, bits, proj, d.P, edge_attr, u, (const float*)w, dO, row_m, row_l,
                       delta, gp, b, g_edge_attr, N, H, C, D, scale);
  });
  if ((rc = gcm_launch_status())) return rc;
  if ((rc = node_add(b, w_e, gp, d.P, d, D, s))) return rc;
  if (g_x || g_w_all || g_b_all) {
    dispatch_nct((C + 31) / 32, [&](auto n) {
      auto kern = k_tre_dense_dkv<n()>;
      const size_t lds = lds_dkv(n(), D);
      gcm_allow_dynamic_lds((const void*)kern, lds);
      hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, bits, proj, d.P, edge_attr, u, (const float*)w, dO, row_m,
                         row_l, (const float*)delta, gp, N, H, C, D, scale);
    });
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_w_e && (rc = gwe(dO, proj, abar, b, (float*)(ws + K.slabs), g_w_e, d, D, s))) return rc;
  return bwd_tail_e(x, w_all, g_x, g_w_all, g_b_all, K, ws, d, s);
}

// ---------------------------------------------------------------------------
// C ABI: TransformerConv with edge features
// ---------------------------------------------------------------------------
extern "C" size_t gcm_csr_transformer_edge_fwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int D,
                                                               int concat, int root) {
  if (M <= 0 || E < 0 || Fi <= 0 || H <= 0 || C <= 0 || D <= 0) return 0;
  return saved_e(dims(M, Fi, H, C, concat, root), D, 0).total;
}

extern "C" int gcm_csr_transformer_edge_fwd(const float* x, const float* edge_attr, const int64_t* row_ptr,
                                            const int64_t* col, const int64_t* csr_perm, const float* w_all,
                                            const float* b_all, const float* w_e, const float* w_beta, float* out,
                                            void* saved, size_t saved_bytes, int64_t M, int64_t E, int Fi, int H,
                                            int C, int D, int concat, int root, gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && w_all && b_all && w_e && out && saved);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && H > 0 && C > 0 && D > 0);
  GCM_REQUIRE(E == 0 || (col && edge_attr));
  GCM_REQUIRE(root || !w_beta);
  if (unsupported_e(M, Fi, H, C, D)) return GCM_EUNSUPPORTED;
  const Dims d = dims(M, Fi, H, C, concat, root);
  const SavedE L = saved_e(d, D, 0);
  GCM_REQUIRE(saved_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* sv = (char*)saved;
  float* proj = (float*)(sv + L.base.proj);
  float* u = (float*)(sv + L.u);
  float* abar = (float*)(sv + L.abar);
  float* o = (float*)(sv + L.base.o);
  const float scale = 1.f / sqrtf((float)C);
  int rc = project(x, w_all, b_all, proj, d, s);
  if (rc || (rc = node_t(proj, d.P, w_e, u, d, D, scale, s))) return rc;
  TR_LAUNCH_GROUP(k_tre_csr_fwd, M * H, s, row_ptr, col, csr_perm, edge_attr, (const float*)proj, d.P,
                  (const float*)u, o, abar, (float*)(sv + L.base.m), (float*)(sv + L.base.l), M, H, C, D, scale)
  if ((rc = gcm_launch_status())) return rc;
  if ((rc = node_add(abar, w_e, o, d.HC, d, D, s))) return rc;
  return fwd_tail(w_beta, out, L.base, sv, d, concat, s);
}

extern "C" size_t gcm_csr_transformer_edge_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int H, int C, int D,
                                                               int concat, int root) {
  if (M <= 0 || E < 0 || Fi <= 0 || H <= 0 || C <= 0 || D <= 0) return 0;
  return bwd_ws_e(dims(M, Fi, H, C, concat, root), D, E).total;
}

extern "C" int gcm_csr_transformer_edge_bwd(const float* g_out, const float* x, const float* edge_attr,
                                            const int64_t* row_ptr, const int64_t* col, const int64_t* csr_perm,
                                            const int64_t* col_ptr, const int64_t* rows, const int64_t* perm,
                                            const float* w_all, const float* w_e, const float* w_beta,
                                            const void* saved, float* g_x, float* g_w_all, float* g_b_all,
                                            float* g_w_e, float* g_w_beta, float* g_edge_attr, void* workspace,
                                            size_t workspace_bytes, int64_t M, int64_t E, int Fi, int H, int C, int D,
                                            int concat, int root, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && row_ptr && w_all && w_e && saved && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && H > 0 && C > 0 && D > 0);
  GCM_REQUIRE(E == 0 || (col && edge_attr && col_ptr && rows && perm));
  GCM_REQUIRE((root || !w_beta) && (w_beta || !g_w_beta));
  if (unsupported_e(M, Fi, H, C, D)) return GCM_EUNSUPPORTED;
  const Dims d = dims(M, Fi, H, C, concat, root);
  const SavedE L = saved_e(d, D, 0);
  const BwdWsE K = bwd_ws_e(d, D, E);
  GCM_REQUIRE(workspace_bytes >= K.total);
  if (!g_x && !g_w_all && !g_b_all && !g_w_e && !g_w_beta && !g_edge_attr) return GCM_OK;
  hipStream_t s = (hipStream_t)stream;
  const char* sv = (const char*)saved;
  char* ws = (char*)workspace;
  int rc = bwd_head(g_out, w_beta, g_w_beta, L.base, sv, K.base, ws, d, concat, s);
  if (rc) return rc;
  const float* proj = (const float*)(sv + L.base.proj);
  const float* u = (const float*)(sv + L.u);
  const float* abar = (const float*)(sv + L.abar);
  const float* dO = (const float*)(ws + K.base.dO);
  float* alpha = (float*)(ws + K.base.alpha);
  float* ds = (float*)(ws + K.base.ds);
  float* gp = (float*)(ws + K.base.gp);
  float* w = (float*)(ws + K.w);
  float* b = (float*)(ws + K.b);
  const float scale = 1.f / sqrtf((float)C);
  if ((rc = node_t(dO, d.HC, w_e, w, d, D, 1.f, s))) return rc;
  TR_LAUNCH_GROUP(k_tre_csr_dq, M * H, s, row_ptr, col, csr_perm, edge_attr, proj, d.P, dO, u, (const float*)w,
                  (const float*)(sv + L.base.m), (const float*)(sv + L.base.l), alpha, ds, gp, b, M, H, C, D, scale)
  if ((rc = gcm_launch_status())) return rc;
  if ((rc = node_add(b, w_e, gp, d.P, d, D, s))) return rc;
  if (g_edge_attr && E > 0) {
    hipLaunchKernelGGL(k_tre_csr_gea, dim3(blocks(E * D, 256)), dim3(256), 0, s, rows, perm, csr_perm,
                       (const float*)alpha, (const float*)ds, u, (const float*)w, g_edge_attr, E, H, D);
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_x || g_w_all || g_b_all) {
    hipLaunchKernelGGL(k_tr_csr_dkv, dim3(blocks(M * H * C, 256)), dim3(256), 0, s, E ? col_ptr : nullptr, rows, perm,
                       (const float*)alpha, (const float*)ds, proj, d.P, dO, gp, M, H, C, scale);
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_w_e && (rc = gwe(dO, proj, abar, b, (float*)(ws + K.slabs), g_w_e, d, D, s))) return rc;
  return bwd_tail_e(x, w_all, g_x, g_w_all, g_b_all, K, ws, d, s);
}
