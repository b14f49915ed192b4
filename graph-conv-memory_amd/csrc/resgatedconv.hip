// ResGatedGraphConv / DenseResGatedGraphConv (PyG, without edge features) forward and backward on gfx950.
//
//   [k | q | v | r] = x W_all^T + b_all (one tile GEMM over the stacked weights; the skip's bias slots are zero)
//   out[i,:] = r[i,:] + sum_{j -> i} a_ij sigmoid(k[i,:] + q[j,:]) * v[j,:] + bias
//
// The gate is per edge AND per channel, so there is no contraction for the matrix cores: the sweeps are VALU work,
// one exp and one division per gate, and the point of the kernels is to visit only the edges that exist and to keep
// every gate in a register.  No gate is ever stored: the backward recomputes them from [k|q|v].
//
// Lanes and channels.  A group of G lanes owns a row; lane gl of the group holds channels gl (and gl + 64 when
// C > 64).  G is the power of two >= C from 8 to 64, so at C = 32 a wave carries two rows and no lane idles.  A group
// owns RG_RPG = 4 rows, a workgroup of 256 threads therefore 4 * 256 / G rows of one graph (32 at C = 32).
//
// dense: the bit image of the pattern (attn_bits.h; set: adj != 0, or the diagonal when add_loop) is built once.
// Neighbours come in tiles of 32 = one word of the image.  A workgroup whose rows have no bit in a word skips the tile
// altogether (one __syncthreads_or); otherwise q and v of the 32 neighbours are staged in LDS, [neighbour][channel],
// channel fastest: the lanes of a group read consecutive words, conflict-free for G >= 32 under ds_read_b32's
// 32-bank rule, two-way for G = 16 and four-way for G = 8 when two groups of a half-wave sit on different neighbours.
// Each group then walks the set bits of its rows' words; adj's value is read for set bits only.
//   k_rg_dense_fwd  by row block: out.
//   k_rg_dense_drow by row block: g_k[i] = sum_j a g_i v_j s (1 - s), and g_adj[i,j] = sum_c g_i s v_j when asked for
//                   (a group sum per entry; then every entry of the row is visited, set or not).
//   k_rg_dense_dcol by neighbour block over the transposed image (k_mask_bits_t): the group owns neighbours, tiles of 32
//                   rows (k and g_out staged): g_q[j] = sum_i a g_i v_j s (1 - s), g_v[j] = sum_i a g_i s.
// Neither backward sweep sums across workgroups.
// sparse: a lane group per destination walks its CSR row (forward, and g_k in the backward); g_q and g_v are gathered
// per (source, channel) over the CSC column.
// The stacked projection gradient [dK | dQ | dV | dR] gives g_x, g_w_all and g_b_all in one GEMM, one split-K weight
// gradient and one column sum (gcn_mm.h); g_bias is the column sum of g_out.  Nothing accumulates with atomics: every
// sum runs in a fixed order.  Fi, C <= 128; any N.
#include <cmath>

#include "attn_bits.h"

namespace {

constexpr int RG_RPG = 4;  // rows (dense) of a lane group

// finite for every argument: z -> -inf gives 1 / (1 + inf) = 0, z -> +inf gives 1 / (1 + 0) = 1, and s (1 - s) = 0
__device__ __forceinline__ float rg_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// the bits of word w that name a neighbour < N
__device__ __forceinline__ unsigned rg_valid_word(int w, int N) {
  const int n = N - w * 32;
  return n >= 32 ? 0xffffffffu : (n <= 0 ? 0u : (1u << n) - 1u);
}

// stage columns [c0, c0 + C) and [c1, c1 + C) of the 32 rows from `first` of src (row stride ld) as [row][CP]
template <int CP>
__device__ __forceinline__ void rg_stage(float* __restrict__ s0, float* __restrict__ s1, const float* __restrict__ src0,
                                         int ld0, const float* __restrict__ src1, int ld1, size_t rb, int first, int N,
                                         int C) {
  for (int e = threadIdx.x; e < GT * CP; e += 256) {
    const int t = e / CP, c = e - t * CP;
    const int n = first + t;
    const bool ok = n < N && c < C;
    s0[e] = ok ? src0[(rb + n) * ld0 + c] : 0.f;
    s1[e] = ok ? src1[(rb + n) * ld1 + c] : 0.f;
  }
}

// ---------------------------------------------------------------------------
// dense forward
// ---------------------------------------------------------------------------
template <int G, int NCH>
__global__ __launch_bounds__(256) void k_rg_dense_fwd(const unsigned* __restrict__ bits, const float* __restrict__ adj,
                                                      const float* __restrict__ proj, int ldp,
                                                      const float* __restrict__ bias, float* __restrict__ out, int N,
                                                      int C, int root, int add_loop) {
  constexpr int CP = G * NCH, S = 256 / G;
  __shared__ float sQ[GT * CP];  // [j][c]
  __shared__ float sV[GT * CP];  // [j][c]
  const int b = blockIdx.y, i0 = blockIdx.x * (S * RG_RPG);
  const int slot = threadIdx.x / G, gl = threadIdx.x % G;
  const int W = (N + 31) / 32;
  const size_t rb = (size_t)b * N;

  float kk[RG_RPG][NCH], acc[RG_RPG][NCH];
#pragma unroll
  for (int r = 0; r < RG_RPG; ++r) {
    const int i = i0 + r * S + slot;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      kk[r][ch] = (i < N && c < C) ? proj[(rb + i) * ldp + c] : 0.f;
      acc[r][ch] = 0.f;
    }
  }

  for (int w = 0; w < W; ++w) {
    unsigned word[RG_RPG], any = 0u;
#pragma unroll
    for (int r = 0; r < RG_RPG; ++r) {
      const int i = i0 + r * S + slot;
      word[r] = i < N ? bits[(rb + i) * W + w] : 0u;
      any |= word[r];
    }
    if (!__syncthreads_or(any != 0u)) continue;  // also: the previous tile is consumed
    rg_stage<CP>(sQ, sV, proj + C, ldp, proj + 2 * C, ldp, rb, w * 32, N, C);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RG_RPG; ++r) {
      const int i = i0 + r * S + slot;
      const float* arow = adj + (rb + i) * N + w * 32;
      unsigned m = word[r];
      while (m) {
        const int jj = __ffs(m) - 1;
        m &= m - 1u;
        const float a = (add_loop && w * 32 + jj == i) ? 1.f : arow[jj];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int o = jj * CP + gl + ch * G;
          acc[r][ch] = fmaf(a * rg_sigmoid(kk[r][ch] + sQ[o]), sV[o], acc[r][ch]);
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < RG_RPG; ++r) {
    const int i = i0 + r * S + slot;
    if (i >= N) continue;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      if (c >= C) continue;
      float v = acc[r][ch];
      if (root) v += proj[(rb + i) * ldp + 3 * C + c];
      if (bias) v += bias[c];
      out[(rb + i) * C + c] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// dense backward by row block: dK into gp[:, 0 ...], dR = g_out into gp[:, 3 C ...] (root), g_adj when asked for
// ---------------------------------------------------------------------------
template <int G, int NCH>
__global__ __launch_bounds__(256) void k_rg_dense_drow(const unsigned* __restrict__ bits, const float* __restrict__ adj,
                                                       const float* __restrict__ proj, int ldp,
                                                       const float* __restrict__ g_out, float* __restrict__ gp,
                                                       float* __restrict__ g_adj, int N, int C, int root,
                                                       int add_loop) {
  constexpr int CP = G * NCH, S = 256 / G;
  __shared__ float sQ[GT * CP];
  __shared__ float sV[GT * CP];
  const int b = blockIdx.y, i0 = blockIdx.x * (S * RG_RPG);
  const int slot = threadIdx.x / G, gl = threadIdx.x % G;
  const int W = (N + 31) / 32;
  const size_t rb = (size_t)b * N;

  float kk[RG_RPG][NCH], go[RG_RPG][NCH], gk[RG_RPG][NCH];
#pragma unroll
  for (int r = 0; r < RG_RPG; ++r) {
    const int i = i0 + r * S + slot;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      const bool ok = i < N && c < C;
      kk[r][ch] = ok ? proj[(rb + i) * ldp + c] : 0.f;
      go[r][ch] = ok ? g_out[(rb + i) * C + c] : 0.f;
      gk[r][ch] = 0.f;
    }
  }

  for (int w = 0; w < W; ++w) {
    unsigned word[RG_RPG], any = 0u;
#pragma unroll
    for (int r = 0; r < RG_RPG; ++r) {
      const int i = i0 + r * S + slot;
      word[r] = i >= N ? 0u : (g_adj ? rg_valid_word(w, N) : bits[(rb + i) * W + w]);
      any |= word[r];
    }
    if (!__syncthreads_or(any != 0u)) continue;
    rg_stage<CP>(sQ, sV, proj + C, ldp, proj + 2 * C, ldp, rb, w * 32, N, C);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RG_RPG; ++r) {
      const int i = i0 + r * S + slot;
      const size_t abase = (rb + i) * N + w * 32;
      unsigned m = word[r];
      while (m) {
        const int jj = __ffs(m) - 1;
        m &= m - 1u;
        const bool loop = add_loop && w * 32 + jj == i;
        const float a = loop ? 1.f : adj[abase + jj];
        float ga = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int o = jj * CP + gl + ch * G;
          const float s = rg_sigmoid(kk[r][ch] + sQ[o]);
          const float t = go[r][ch] * sV[o];
          ga = fmaf(t, s, ga);
          gk[r][ch] = fmaf(a * t, s * (1.f - s), gk[r][ch]);
        }
        if (g_adj) {
          ga = group_sum<G>(ga);
          if (gl == 0) g_adj[abase + jj] = loop ? 0.f : ga;
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < RG_RPG; ++r) {
    const int i = i0 + r * S + slot;
    if (i >= N) continue;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      if (c >= C) continue;
      gp[(rb + i) * ldp + c] = gk[r][ch];
      if (root) gp[(rb + i) * ldp + 3 * C + c] = go[r][ch];
    }
  }
}

// ---------------------------------------------------------------------------
// dense backward by neighbour block: dQ into gp[:, C ...], dV into gp[:, 2 C ...].  The group owns neighbours j and
// walks the rows i that have j (the transposed image); k and g_out of 32 rows are staged.
// ---------------------------------------------------------------------------
template <int G, int NCH>
__global__ __launch_bounds__(256) void k_rg_dense_dcol(const unsigned* __restrict__ bitsT,
                                                       const float* __restrict__ adj, const float* __restrict__ proj,
                                                       int ldp, const float* __restrict__ g_out,
                                                       float* __restrict__ gp, int N, int C, int add_loop) {
  constexpr int CP = G * NCH, S = 256 / G;
  __shared__ float sK[GT * CP];  // [i][c]
  __shared__ float sG[GT * CP];  // [i][c]
  const int b = blockIdx.y, j0 = blockIdx.x * (S * RG_RPG);
  const int slot = threadIdx.x / G, gl = threadIdx.x % G;
  const int W = (N + 31) / 32;
  const size_t rb = (size_t)b * N;

  float qq[RG_RPG][NCH], vv[RG_RPG][NCH], gq[RG_RPG][NCH], gv[RG_RPG][NCH];
#pragma unroll
  for (int r = 0; r < RG_RPG; ++r) {
    const int j = j0 + r * S + slot;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      const bool ok = j < N && c < C;
      qq[r][ch] = ok ? proj[(rb + j) * ldp + C + c] : 0.f;
      vv[r][ch] = ok ? proj[(rb + j) * ldp + 2 * C + c] : 0.f;
      gq[r][ch] = gv[r][ch] = 0.f;
    }
  }

  for (int w = 0; w < W; ++w) {
    unsigned word[RG_RPG], any = 0u;
#pragma unroll
    for (int r = 0; r < RG_RPG; ++r) {
      const int j = j0 + r * S + slot;
      word[r] = j < N ? bitsT[(rb + j) * W + w] : 0u;
      any |= word[r];
    }
    if (!__syncthreads_or(any != 0u)) continue;
    rg_stage<CP>(sK, sG, proj, ldp, g_out, C, rb, w * 32, N, C);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RG_RPG; ++r) {
      const int j = j0 + r * S + slot;
      unsigned m = word[r];
      while (m) {
        const int ii = __ffs(m) - 1;
        m &= m - 1u;
        const int i = w * 32 + ii;
        const float a = (add_loop && i == j) ? 1.f : adj[(rb + i) * N + j];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int o = ii * CP + gl + ch * G;
          const float s = rg_sigmoid(sK[o] + qq[r][ch]);
          const float ag = a * sG[o];
          gv[r][ch] = fmaf(ag, s, gv[r][ch]);
          gq[r][ch] = fmaf(ag * vv[r][ch], s * (1.f - s), gq[r][ch]);
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < RG_RPG; ++r) {
    const int j = j0 + r * S + slot;
    if (j >= N) continue;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      if (c >= C) continue;
      gp[(rb + j) * ldp + C + c] = gq[r][ch];
      gp[(rb + j) * ldp + 2 * C + c] = gv[r][ch];
    }
  }
}

// ---------------------------------------------------------------------------
// sparse.  A group of G lanes per destination i walks its CSR row.
// ---------------------------------------------------------------------------
template <int G, int NCH>
__global__ __launch_bounds__(256) void k_rg_csr_fwd(const int64_t* __restrict__ row_ptr,
                                                    const int64_t* __restrict__ col, const float* __restrict__ proj,
                                                    int ldp, const float* __restrict__ bias, float* __restrict__ out,
                                                    int64_t M, int C, int root) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (i >= M) return;
  const int gl = threadIdx.x % G;
  float kk[NCH], acc[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + ch * G;
    kk[ch] = c < C ? proj[(size_t)i * ldp + c] : 0.f;
    acc[ch] = 0.f;
  }
  for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
    const float* qr = proj + (size_t)col[e] * ldp + C;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      if (c < C) acc[ch] = fmaf(rg_sigmoid(kk[ch] + qr[c]), qr[C + c], acc[ch]);
    }
  }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + ch * G;
    if (c >= C) continue;
    float v = acc[ch];
    if (root) v += proj[(size_t)i * ldp + 3 * C + c];
    if (bias) v += bias[c];
    out[(size_t)i * C + c] = v;
  }
}

// backward, per destination: dK into gp[:, 0 ...], dR = g_out into gp[:, 3 C ...] (root)
template <int G, int NCH>
__global__ __launch_bounds__(256) void k_rg_csr_dk(const int64_t* __restrict__ row_ptr, const int64_t* __restrict__ col,
                                                   const float* __restrict__ proj, int ldp,
                                                   const float* __restrict__ g_out, float* __restrict__ gp, int64_t M,
                                                   int C, int root) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (i >= M) return;
  const int gl = threadIdx.x % G;
  float kk[NCH], go[NCH], gk[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + ch * G;
    kk[ch] = c < C ? proj[(size_t)i * ldp + c] : 0.f;
    go[ch] = c < C ? g_out[(size_t)i * C + c] : 0.f;
    gk[ch] = 0.f;
  }
  for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
    const float* qr = proj + (size_t)col[e] * ldp + C;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = gl + ch * G;
      if (c >= C) continue;
      const float s = rg_sigmoid(kk[ch] + qr[c]);
      gk[ch] = fmaf(go[ch] * qr[C + c], s * (1.f - s), gk[ch]);
    }
  }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c = gl + ch * G;
    if (c >= C) continue;
    gp[(size_t)i * ldp + c] = gk[ch];
    if (root) gp[(size_t)i * ldp + 3 * C + c] = go[ch];
  }
}

// backward, per (source j, channel c) over its CSC column: dQ into gp[:, C ...], dV into gp[:, 2 C ...]
__global__ __launch_bounds__(256) void k_rg_csr_dqv(const int64_t* __restrict__ col_ptr,
                                                    const int64_t* __restrict__ rows, const float* __restrict__ proj,
                                                    int ldp, const float* __restrict__ g_out, float* __restrict__ gp,
                                                    int64_t M, int C) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * C) return;
  const int64_t j = t / C;
  const int c = (int)(t - j * C);
  const float q = proj[(size_t)j * ldp + C + c], v = proj[(size_t)j * ldp + 2 * C + c];
  float gq = 0.f, gv = 0.f;
  if (col_ptr)
    for (int64_t k = col_ptr[j]; k < col_ptr[j + 1]; ++k) {
      const int64_t i = rows[k];
      const float s = rg_sigmoid(proj[(size_t)i * ldp + c] + q);
      const float g = g_out[(size_t)i * C + c];
      gv = fmaf(g, s, gv);
      gq = fmaf(g * v, s * (1.f - s), gq);
    }
  gp[(size_t)j * ldp + C + c] = gq;
  gp[(size_t)j * ldp + 2 * C + c] = gv;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct Dims {
  int64_t R;
  int Fi, C, P, root;
};

Dims dims(int64_t R, int Fi, int C, int root) {
  Dims d;
  d.R = R, d.Fi = Fi, d.C = C, d.root = root, d.P = (root ? 4 : 3) * C;
  return d;
}

bool unsupported(int64_t R, int Fi, int C) { return Fi > 128 || C > 128 || R > (1 << 30); }

// what the forward keeps for the backward: [k|q|v|r] [R,P] and, dense, the bit image
struct Saved {
  size_t proj, bits, total;
};
Saved saved_layout(const Dims& d, int64_t bit_words) {
  Saved s;
  Carve c;
  s.proj = c.take((size_t)d.R * d.P * 4);
  s.bits = c.take((size_t)bit_words * 4);
  s.total = c.at;
  return s;
}

// backward workspace: gp = [dK|dQ|dV|dR] [R,P], the transposed image (dense), slabs for the weight gradient and the
// column sums
struct BwdWs {
  size_t gp, bitsT, slabs, total;
};
BwdWs bwd_ws(const Dims& d, int64_t bit_words) {
  BwdWs w;
  int nsplit, kchunk;
  wgrad_split64(d.R, &nsplit, &kchunk);
  const size_t slab_f = std::max<size_t>((size_t)nsplit * d.P * d.Fi, (size_t)colsum_slabs(d.R) * d.P);
  Carve c;
  w.gp = c.take((size_t)d.R * d.P * 4);
  w.bitsT = c.take((size_t)bit_words * 4);
  w.slabs = c.take(slab_f * 4);
  w.total = c.at;
  return w;
}

// [k|q|v|r] = x W_all^T + b_all
int project(const float* x, const float* w_all, const float* b_all, float* proj, const Dims& d, hipStream_t s) {
  return mm_xwt(x, w_all, b_all, proj, d.R, d.Fi, d.P, s);
}

// from the stacked projection gradient: g_b_all = its column sums, g_x = gp W_all, g_w_all = gp^T x; g_bias = the
// column sums of g_out
int bwd_tail(const float* g_out, const float* x, const float* w_all, float* g_x, float* g_w_all, float* g_b_all,
             float* g_bias, const BwdWs& K, char* ws, const Dims& d, hipStream_t s) {
  const float* gp = (const float*)(ws + K.gp);
  float* slabs = (float*)(ws + K.slabs);
  int rc;
  if (g_bias && (rc = colsum(g_out, d.R, d.C, g_bias, slabs, s))) return rc;
  if (g_b_all && (rc = colsum(gp, d.R, d.P, g_b_all, slabs, s))) return rc;
  if (g_x && (rc = mm_gw(gp, w_all, g_x, d.R, d.Fi, d.P, s))) return rc;
  if (g_w_all && (rc = wgrad(gp, x, g_w_all, slabs, d.R, d.Fi, d.P, s, wgrad_split64))) return rc;
  return GCM_OK;
}

// launch K<G, NCH> with the lane group of this C on the grid GRID(G)
#define RG_DENSE_GRID(G) dim3(blocks(N, (256 / (G)) * RG_RPG), B)
#define RG_CSR_GRID(G) dim3(blocks(M * (G), 256))
#define RG_LAUNCH(K, GRID, s, ...)                                                              \
  if (C <= 8) hipLaunchKernelGGL((K<8, 1>), GRID(8), dim3(256), 0, s, __VA_ARGS__);             \
  else if (C <= 16) hipLaunchKernelGGL((K<16, 1>), GRID(16), dim3(256), 0, s, __VA_ARGS__);     \
  else if (C <= 32) hipLaunchKernelGGL((K<32, 1>), GRID(32), dim3(256), 0, s, __VA_ARGS__);     \
  else if (C <= 64) hipLaunchKernelGGL((K<64, 1>), GRID(64), dim3(256), 0, s, __VA_ARGS__);     \
  else hipLaunchKernelGGL((K<64, 2>), GRID(64), dim3(256), 0, s, __VA_ARGS__);

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: DenseResGatedGraphConv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_dense_resgatedconv_fwd_workspace_bytes(int B, int N, int Fi, int C, int root) {
  if (B <= 0 || N <= 0 || Fi <= 0 || C <= 0) return 0;
  const int64_t R = (int64_t)B * N;
  return saved_layout(dims(R, Fi, C, root), R * ((N + 31) / 32)).total;
}

extern "C" int gcm_dense_resgatedconv_fwd(const float* x, const float* adj, const float* w_all, const float* b_all,
                                          const float* bias, float* out, void* saved, size_t saved_bytes, int B, int N,
                                          int Fi, int C, int root, int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && w_all && b_all && out && saved);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && C > 0);
  const int64_t R = (int64_t)B * N;
  if (unsupported(R, Fi, C) || B > 65535) return GCM_EUNSUPPORTED;
  const Dims d = dims(R, Fi, C, root);
  const int W = (N + 31) / 32;
  const Saved L = saved_layout(d, R * W);
  GCM_REQUIRE(saved_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* sv = (char*)saved;
  unsigned* bits = (unsigned*)(sv + L.bits);
  float* proj = (float*)(sv + L.proj);
  int rc = mask_bits(adj, bits, R, N, W, add_loop, s);
  if (rc || (rc = project(x, w_all, b_all, proj, d, s))) return rc;
  RG_LAUNCH(k_rg_dense_fwd, RG_DENSE_GRID, s, (const unsigned*)bits, adj, (const float*)proj, d.P, bias, out, N, C,
            root, add_loop)
  return gcm_launch_status();
}

extern "C" size_t gcm_dense_resgatedconv_bwd_workspace_bytes(int B, int N, int Fi, int C, int root) {
  if (B <= 0 || N <= 0 || Fi <= 0 || C <= 0) return 0;
  const int64_t R = (int64_t)B * N;
  return bwd_ws(dims(R, Fi, C, root), R * ((N + 31) / 32)).total;
}

extern "C" int gcm_dense_resgatedconv_bwd(const float* g_out, const float* x, const float* adj, const float* w_all,
                                          const void* saved, float* g_x, float* g_w_all, float* g_b_all, float* g_bias,
                                          float* g_adj, void* workspace, size_t workspace_bytes, int B, int N, int Fi,
                                          int C, int root, int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && adj && w_all && saved && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && C > 0);
  const int64_t R = (int64_t)B * N;
  if (unsupported(R, Fi, C) || B > 65535) return GCM_EUNSUPPORTED;
  const Dims d = dims(R, Fi, C, root);
  const int W = (N + 31) / 32;
  const Saved L = saved_layout(d, R * W);
  const BwdWs K = bwd_ws(d, R * W);
  GCM_REQUIRE(workspace_bytes >= K.total);
  if (!g_x && !g_w_all && !g_b_all && !g_bias && !g_adj) return GCM_OK;
  hipStream_t s = (hipStream_t)stream;
  const char* sv = (const char*)saved;
  char* ws = (char*)workspace;
  const unsigned* bits = (const unsigned*)(sv + L.bits);
  const float* proj = (const float*)(sv + L.proj);
  float* gp = (float*)(ws + K.gp);
  int rc;
  if (g_x || g_w_all || g_b_all || g_adj) {
    RG_LAUNCH(k_rg_dense_drow, RG_DENSE_GRID, s, bits, adj, proj, d.P, g_out, gp, g_adj, N, C, root, add_loop)
    if ((rc = gcm_launch_status())) return rc;
  }
  if (g_x || g_w_all || g_b_all) {
    unsigned* bitsT = (unsigned*)(ws + K.bitsT);
    if ((rc = mask_bits_t(bits, bitsT, R, N, W, s))) return rc;
    RG_LAUNCH(k_rg_dense_dcol, RG_DENSE_GRID, s, (const unsigned*)bitsT, adj, proj, d.P, g_out, gp, N, C, add_loop)
    if ((rc = gcm_launch_status())) return rc;
  }
  return bwd_tail(g_out, x, w_all, g_x, g_w_all, g_b_all, g_bias, K, ws, d, s);
}

// ---------------------------------------------------------------------------
// C ABI: ResGatedGraphConv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_csr_resgatedconv_fwd_workspace_bytes(int64_t M, int64_t E, int Fi, int C, int root) {
  if (M <= 0 || E < 0 || Fi <= 0 || C <= 0) return 0;
  return saved_layout(dims(M, Fi, C, root), 0).total;
}

extern "C" int gcm_csr_resgatedconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* w_all,
                                        const float* b_all, const float* bias, float* out, void* saved,
                                        size_t saved_bytes, int64_t M, int64_t E, int Fi, int C, int root,
                                        gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && w_all && b_all && out && saved);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && C > 0);
  GCM_REQUIRE(E == 0 || col);
  if (unsupported(M, Fi, C)) return GCM_EUNSUPPORTED;
  const Dims d = dims(M, Fi, C, root);
  const Saved L = saved_layout(d, 0);
  GCM_REQUIRE(saved_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  float* proj = (float*)((char*)saved + L.proj);
  int rc = project(x, w_all, b_all, proj, d, s);
  if (rc) return rc;
  RG_LAUNCH(k_rg_csr_fwd, RG_CSR_GRID, s, row_ptr, col, (const float*)proj, d.P, bias, out, M, C, root)
  return gcm_launch_status();
}

extern "C" size_t gcm_csr_resgatedconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int C, int root) {
  if (M <= 0 || E < 0 || Fi <= 0 || C <= 0) return 0;
  return bwd_ws(dims(M, Fi, C, root), 0).total;
}

extern "C" int gcm_csr_resgatedconv_bwd(const float* g_out, const float* x, const int64_t* row_ptr, const int64_t* col,
                                        const int64_t* col_ptr, const int64_t* rows, const float* w_all,
                                        const void* saved, float* g_x, float* g_w_all, float* g_b_all, float* g_bias,
                                        void* workspace, size_t workspace_bytes, int64_t M, int64_t E, int Fi, int C,
                                        int root, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && row_ptr && w_all && saved && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && C > 0);
  GCM_REQUIRE(E == 0 || (col && col_ptr && rows));
  if (unsupported(M, Fi, C)) return GCM_EUNSUPPORTED;
  const Dims d = dims(M, Fi, C, root);
  const Saved L = saved_layout(d, 0);
  const BwdWs K = bwd_ws(d, 0);
  GCM_REQUIRE(workspace_bytes >= K.total);
  if (!g_x && !g_w_all && !g_b_all && !g_bias) return GCM_OK;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const float* proj = (const float*)((const char*)saved + L.proj);
  float* gp = (float*)(ws + K.gp);
  int rc;
  if (g_x || g_w_all || g_b_all) {
    RG_LAUNCH(k_rg_csr_dk, RG_CSR_GRID, s, row_ptr, col, proj, d.P, g_out, gp, M, C, root)
    if ((rc = gcm_launch_status())) return rc;
    hipLaunchKernelGGL(k_rg_csr_dqv, dim3(blocks(M * C, 256)), dim3(256), 0, s, E ? col_ptr : nullptr, rows, proj, d.P,
                       g_out, gp, M, C);
    if ((rc = gcm_launch_status())) return rc;
  }
  return bwd_tail(g_out, x, w_all, g_x, g_w_all, g_b_all, g_bias, K, ws, d, s);
}
