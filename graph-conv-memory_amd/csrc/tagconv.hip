// TAGConv / DenseTAGConv (PyG's TAGConv, Du et al.; include/gcm_hip_tag.h) forward and backward on gfx950.
//
//   h_0 = x;  h_k = A^ h_{k-1};  out = sum_{k=0..K} h_k W_k^T + bias;   A^ = D^-1/2 A D^-1/2 (normalize) or A
//   r_K = g W_K;  r_k = g W_k + A^^T r_{k+1};  g_x = r_0;  g_W_k = g^T h_k;  g_A^ = sum_{k>=1} r_k h_{k-1}^T
//
// Dense, N <= 128: ONE launch runs every hop, one workgroup per graph (k_tag_dense_fwd).  The adjacency is read from
// memory once, the row degrees are taken from the registers it arrives in and A^ goes to LDS scaled; the hop state
// lives in one LDS image: a wave accumulates its 32 rows of h_k in registers, and the image is overwritten only after
// every wave has finished reading h_{k-1}, so no second image is needed and N = 128 with 128 channels still fits.  Both
// products (A^ h and h_k W_k^T) run on v_mfma_f32_32x32x2_f32; the accumulator of `out` stays in registers across the
// hops.  32 x 32 tiles of A^ that hold no entry are skipped (a bit per tile, set while the image is stored).  The
// backward's Horner chain (k_tag_dense_chain) has the same form over A^^T.  N > 128: one k_gcn_mm launch per hop.
// Sparse: one launch per hop (k_tag_csr_hop): the gather of h_k over the destination CSR into LDS, then h_k W_k^T
// accumulated into out; the chain gathers over the CSC.
//
// The degree term of the adjacency / edge-weight gradient needs no pass over the N x N gradient: with G = g_A^,
//   sum_j G_ij A^_ij = sum_k <r_k[i], h_k[i]>   and   sum_j G_ji A^_ji = sum_k <u_k[i], h_{k-1}[i]>,  u_k = A^^T r_k,
// so g_deg_i = -1/2 d_i^2 * (those two sums), row-local (k_tag_rowterm).  No float atomics anywhere.
#include <cstdlib>

#include "gcn_mm.h"

namespace {

__device__ __forceinline__ float tag_dinv(float deg) { return deg == 0.f ? 0.f : 1.f / sqrtf(deg); }

// ---------------------------------------------------------------------------
// dense, N <= 128: the LDS image of A^ shared by the forward and the chain
// ---------------------------------------------------------------------------
// sum over the 32 lanes of the caller's half wave, in every lane of it (DPP and row swap: no LDS)
__device__ __forceinline__ float tag_half_sum(float v) {
  v += GCM_DPP_F(v, 0xB1, 0xF, 0.f);    // quad_perm [1,0,3,2]
  v += GCM_DPP_F(v, 0x4E, 0xF, 0.f);    // quad_perm [2,3,0,1]
  v += GCM_DPP_F(v, 0x141, 0xF, 0.f);   // row_half_mirror
  v += GCM_DPP_F(v, 0x140, 0xF, 0.f);   // row_mirror
  return gcm_xor16_add(v);
}

// The image of A^ from memory in one pass: sA[i * lda + j] = d_i adj[i, j] d_j (diagonal of adj 1 with add_loop), zero
// padded to NP x NP.  A group of 32 lanes owns the rows tr, tr + 8, ...: at most 16 rows of 4 values per thread, all
// loaded (16 bytes a lane when VEC) before anything else happens, so the whole graph is in flight at once.  The row
// degrees are sums over the group's registers (d_in == nullptr; written to sD and d_out) or come from d_in; the values
// are scaled in the registers and stored once - the image is never read back.  (Loading element by element, summing the
// rows out of LDS and scaling the image in place cost 50 us of fixed time at N = 128; this form 22 us less.)
// Returns the tiles in which this thread holds a non-zero: bit 4 * (i / 32) + (j / 32).
template <bool VEC>
__device__ __forceinline__ unsigned tag_stage_adj_t(float* sA, float* sD, const float* __restrict__ adjb,
                                                    const float* __restrict__ d_in, float* __restrict__ d_out, int N,
                                                    int NP, int lda, int normalize, int add_loop) {
  constexpr int RMAX = 16;   // rows per group: NP / 8
  const int tj = threadIdx.x & 31, tr = threadIdx.x >> 5;
  float v[RMAX][4];
#pragma unroll
  for (int u = 0; u < RMAX; ++u) {
    const int i = tr + 8 * u;
    if (VEC) {
      f32x4 t = {0.f, 0.f, 0.f, 0.f};
      if (i < N && 4 * tj < N) t = ((const f32x4*)(adjb + (size_t)i * N))[tj];
#pragma unroll
      for (int c = 0; c < 4; ++c) v[u][c] = t[c];
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = tj + 32 * c;
        v[u][c] = (i < N && j < N) ? adjb[(size_t)i * N + j] : 0.f;
      }
    }
  }
  if (add_loop) {
#pragma unroll
    for (int u = 0; u < RMAX; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = tr + 8 * u, j = VEC ? 4 * tj + c : tj + 32 * c;
        if (i == j && i < N) v[u][c] = 1.f;
      }
  }
  if (normalize) {
    if (d_in) {
      if (threadIdx.x < NP) sD[threadIdx.x] = threadIdx.x < N ? d_in[threadIdx.x] : 0.f;
    } else {
#pragma unroll
      for (int u = 0; u < RMAX; ++u) {
        const int i = tr + 8 * u;
        const float d = tag_dinv(tag_half_sum((v[u][0] + v[u][1]) + (v[u][2] + v[u][3])));
        if (tj == 0 && i < NP) {
          sD[i] = d;
          if (i < N) d_out[i] = d;
        }
      }
    }
    __syncthreads();
    float dj[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = VEC ? 4 * tj + c : tj + 32 * c;
      dj[c] = j < NP ? sD[j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < RMAX; ++u) {
      const int i = tr + 8 * u;
      const float di = i < NP ? sD[i] : 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) v[u][c] = di * v[u][c] * dj[c];
    }
  } else if (d_out && threadIdx.x < N) {
    d_out[threadIdx.x] = 1.f;
  }
  unsigned m = 0;
#pragma unroll
  for (int u = 0; u < RMAX; ++u)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = tr + 8 * u, j = VEC ? 4 * tj + c : tj + 32 * c;
      if (i >= NP || j >= NP) continue;
      sA[i * lda + j] = v[u][c];
      if (v[u][c] != 0.f) m |= 1u << (4 * (i >> 5) + (j >> 5));
    }
  return m;
}

__device__ __forceinline__ unsigned tag_stage_adj(float* sA, float* sD, const float* __restrict__ adjb,
                                                  const float* __restrict__ d_in, float* __restrict__ d_out, int N,
                                                  int NP, int lda, int normalize, int add_loop) {
  if ((N & 3) == 0 && ((uintptr_t)adjb & 15) == 0)
    return tag_stage_adj_t<true>(sA, sD, adjb, d_in, d_out, N, NP, lda, normalize, add_loop);
  return tag_stage_adj_t<false>(sA, sD, adjb, d_in, d_out, N, NP, lda, normalize, add_loop);
}

// occ[t] |= bit u for every 32 x 32 tile (row tile t, column tile u; of the transpose when `transposed`) in which a
// thread saw a non-zero: the masks are OR-ed over the wave first, then one lane publishes them (integer OR: order-free)
__device__ __forceinline__ void tag_publish_occ(unsigned m, unsigned* occ, int transposed) {
  unsigned wm = 0;
#pragma unroll
  for (int bit = 0; bit < 16; ++bit)
    if (__ballot((m >> bit) & 1u)) wm |= 1u << bit;
  if ((threadIdx.x & 63) != 0) return;
  for (int bit = 0; bit < 16; ++bit)
    if ((wm >> bit) & 1u) {
      const int it = bit >> 2, jt = bit & 3;
      if (transposed) atomicOr(&occ[jt], 1u << it);
      else atomicOr(&occ[it], 1u << jt);
    }
}

// every hop of the forward for one graph
template <int NCI, int NCO>
__global__ __launch_bounds__(256) void k_tag_dense_fwd(const float* __restrict__ x, const float* __restrict__ adj,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out, float* __restrict__ hs,
                                                       float* __restrict__ dinv, int N, int Fi, int Fo, int K,
                                                       int normalize, int add_loop, int skip) {
  constexpr int FiP = 32 * NCI, ldh = FiP + 1;
  extern __shared__ float smem[];
  const int NP = (N + 31) & ~31, lda = NP + 1;
  float* sA = smem;               // [NP][lda]  A^
  float* sH = sA + NP * lda;      // [NP][ldh]  h_k
  float* sW = sH + NP * ldh;      // [FiP][33]  W_k^T, 32 output columns at a time
  float* sD = sW + FiP * 33;      // [NP]
  unsigned* sOcc = (unsigned*)(sD + NP);  // [4]
  const int b = blockIdx.x;
  const int64_t R = (int64_t)gridDim.x * N;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const bool active = wave * 32 < NP;

  const float* xb = x + (size_t)b * N * Fi;
  for (int e = threadIdx.x; e < NP * FiP; e += 256) {
    const int i = e / FiP, f = e - i * FiP;
    sH[i * ldh + f] = (i < N && f < Fi) ? xb[(size_t)i * Fi + f] : 0.f;
  }
  if (threadIdx.x < 4) sOcc[threadIdx.x] = skip ? 0u : 0xfu;
  const unsigned seen = tag_stage_adj(sA, sD, adj + (size_t)b * N * N, nullptr, dinv + (size_t)b * N, N, NP, lda,
                                      normalize, add_loop);
  __syncthreads();
  if (skip) tag_publish_occ(seen, sOcc, 0);
  __syncthreads();

  f32x16 oacc[NCO];
#pragma unroll
  for (int c = 0; c < NCO; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[c][r] = 0.f;

  for (int k = 0; k <= K; ++k) {
    if (k > 0) {   // h_k = A^ h_{k-1}: the wave's 32 rows in registers, then over the image
      f32x16 hacc[NCI];
#pragma unroll
      for (int c = 0; c < NCI; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) hacc[c][r] = 0.f;
      if (active) {
        const unsigned occ = sOcc[wave];
        for (int kt = 0; kt < NP / 32; ++kt) {
          if (!((occ >> kt) & 1u)) continue;
#pragma unroll
          for (int c = 0; c < NCI; ++c)
            mma32_tiles(hacc[c], sA + wave * 32 * lda + kt * 32, lda, 1, sH + kt * 32 * ldh + c * 32, ldh, 1, 32, li,
                        lh);
        }
      }
      __syncthreads();
      if (active) {
        float* hk = hs + ((size_t)(k - 1) * R + (size_t)b * N) * Fi;
#pragma unroll
        for (int c = 0; c < NCI; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = wave * 32 + acc_row(r, lh), col = c * 32 + li;
            sH[row * ldh + col] = hacc[c][r];
            if (row < N && col < Fi) hk[(size_t)row * Fi + col] = hacc[c][r];
          }
      }
      __syncthreads();
    }
    const float* wk = w + (size_t)k * Fo * Fi;
#pragma unroll
    for (int c = 0; c < NCO; ++c) {   // out += h_k W_k^T
      for (int e = threadIdx.x; e < 32 * FiP; e += 256) {   // sW[f][n] = W_k[c * 32 + n][f]
        const int n = e / FiP, f = e - n * FiP;
        sW[f * 33 + n] = (c * 32 + n < Fo && f < Fi) ? wk[(size_t)(c * 32 + n) * Fi + f] : 0.f;
      }
      __syncthreads();
      if (active) mma32_tiles(oacc[c], sH + wave * 32 * ldh, ldh, 1, sW, 33, 1, FiP, li, lh);
      __syncthreads();
    }
  }

  if (!active) return;
  float* ob = out + (size_t)b * N * Fo;
#pragma unroll
  for (int c = 0; c < NCO; ++c) {
    const int col = c * 32 + li;
    if (col >= Fo) continue;
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wave * 32 + acc_row(r, lh);
      if (row < N) ob[(size_t)row * Fo + col] = oacc[c][r] + bv;
    }
  }
}

// the Horner chain of the backward for one graph: T [K+1,R,Fi] holds g W_k on entry and r_k on exit (r_0 goes to g_x
// when it is given); U [K,R,Fi] (optional) receives u_k = A^^T r_k at slot k - 1
template <int NCI>
__global__ __launch_bounds__(256) void k_tag_dense_chain(const float* __restrict__ adj,
                                                         const float* __restrict__ dinv, float* __restrict__ T,
                                                         float* __restrict__ U, float* __restrict__ g_x, int N,
                                                         int Fi, int K, int normalize, int add_loop, int skip) {
  constexpr int FiP = 32 * NCI, ldh = FiP + 1;
  extern __shared__ float smem[];
  const int NP = (N + 31) & ~31, lda = NP + 1;
  float* sA = smem;
  float* sR = sA + NP * lda;
  float* sD = sR + NP * ldh;
  unsigned* sOcc = (unsigned*)(sD + NP);
  const int b = blockIdx.x;
  const int64_t R = (int64_t)gridDim.x * N;
  const size_t hop = (size_t)R * Fi, base = (size_t)b * N * Fi;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const bool active = wave * 32 < NP;

  const float* tK = T + (size_t)K * hop + base;
  for (int e = threadIdx.x; e < NP * FiP; e += 256) {
    const int i = e / FiP, f = e - i * FiP;
    sR[i * ldh + f] = (i < N && f < Fi) ? tK[(size_t)i * Fi + f] : 0.f;
  }
  if (threadIdx.x < 4) sOcc[threadIdx.x] = skip ? 0u : 0xfu;
  const unsigned seen = tag_stage_adj(sA, sD, adj + (size_t)b * N * N, dinv + (size_t)b * N, nullptr, N, NP, lda,
                                      normalize, add_loop);
  __syncthreads();
  if (skip) tag_publish_occ(seen, sOcc, 1);
  __syncthreads();

  for (int k = K; k >= 1; --k) {   // r_{k-1} = T_{k-1} + A^^T r_k
    f32x16 acc[NCI];
#pragma unroll
    for (int c = 0; c < NCI; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    if (active) {
      const unsigned occ = sOcc[wave];
      for (int it = 0; it < NP / 32; ++it) {
        if (!((occ >> it) & 1u)) continue;
#pragma unroll
        for (int c = 0; c < NCI; ++c)
          mma32_tiles(acc[c], sA + it * 32 * lda + wave * 32, 1, lda, sR + it * 32 * ldh + c * 32, ldh, 1, 32, li,
                      lh);
      }
    }
    __syncthreads();
    if (active) {
      const float* tp = T + (size_t)(k - 1) * hop + base;
      float* dest = (k == 1 && g_x) ? g_x + base : T + (size_t)(k - 1) * hop + base;
      float* uk = U ? U + (size_t)(k - 1) * hop + base : nullptr;
#pragma unroll
      for (int c = 0; c < NCI; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wave * 32 + acc_row(r, lh), col = c * 32 + li;
          float v = 0.f;
          if (row < N && col < Fi) {
            const size_t o = (size_t)row * Fi + col;
            if (uk) uk[o] = acc[c][r];
            v = tp[o] + acc[c][r];
            dest[o] = v;
          }
          sR[row * ldh + col] = v;
        }
    }
    __syncthreads();
  }
}

size_t tag_fwd_lds(int N, int Fi) {
  const int NP = (N + 31) & ~31, FiP = (Fi + 31) & ~31;
  return sizeof(float) * ((size_t)NP * (NP + 1) + (size_t)NP * (FiP + 1) + (size_t)FiP * 33 + NP + 4);
}
size_t tag_chain_lds(int N, int Fi) {
  const int NP = (N + 31) & ~31, FiP = (Fi + 31) & ~31;
  return sizeof(float) * ((size_t)NP * (NP + 1) + (size_t)NP * (FiP + 1) + NP + 4);
}

// measuring switch only: GCM_TAG_NO_SKIP=1 visits the empty tiles too (same results)
int tag_skip() {
  static const int skip = !(std::getenv("GCM_TAG_NO_SKIP") && std::getenv("GCM_TAG_NO_SKIP")[0] == '1');
  return skip;
}

// ---------------------------------------------------------------------------
// dense, any N: degrees, the linear part, an elementwise sum (the per-hop path)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tag_deg(const float* __restrict__ adj, float* __restrict__ dinv,
                                                 int64_t rows, int N, int normalize, int add_loop) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int i = (int)(row % N);
  const float* a = adj + (size_t)row * N;
  float s = 0.f;
  for (int j = lane; j < N; j += 64) s += (add_loop && j == i) ? 1.f : a[j];
  s = gcm_wave_sum(s);
  if (lane == 0) dinv[row] = normalize ? tag_dinv(s) : 1.f;
}

// out[r, :] = sum_k h_k[r, :] W_k^T + bias, h_0 = x, h_k = hs[k - 1]; 128 rows x 32 columns per workgroup
__global__ __launch_bounds__(256) void k_tag_lin(const float* __restrict__ x, const float* __restrict__ hs,
                                                 const float* __restrict__ w, const float* __restrict__ bias,
                                                 float* __restrict__ out, int64_t R, int Fi, int Fo, int K) {
  __shared__ float sX[MB * 33];
  __shared__ float sW[32 * 33];
  const int64_t r0 = (int64_t)blockIdx.x * MB;
  const int o0 = blockIdx.y * 32;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k = 0; k <= K; ++k) {
    const float* hk = k == 0 ? x : hs + (size_t)(k - 1) * R * Fi;
    const float* wk = w + (size_t)k * Fo * Fi;
    for (int f0 = 0; f0 < Fi; f0 += 32) {
      for (int e = threadIdx.x; e < MB * 32; e += 256) {
        const int r = e >> 5, f = e & 31;
        sX[r * 33 + f] = (r0 + r < R && f0 + f < Fi) ? hk[(size_t)(r0 + r) * Fi + f0 + f] : 0.f;
      }
      for (int e = threadIdx.x; e < 32 * 32; e += 256) {
        const int n = e >> 5, f = e & 31;
        sW[f * 33 + n] = (o0 + n < Fo && f0 + f < Fi) ? wk[(size_t)(o0 + n) * Fi + f0 + f] : 0.f;
      }
      __syncthreads();
      mma32_tiles(acc, sX + wave * 32 * 33, 33, 1, sW, 33, 1, 32, li, lh);
      __syncthreads();
    }
  }
  const int col = o0 + li;
  if (col >= Fo) return;
  const float bv = bias ? bias[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = r0 + wave * 32 + acc_row(r, lh);
    if (row < R) out[(size_t)row * Fo + col] = acc[r] + bv;
  }
}

__global__ void k_tag_add(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ dest,
                          int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dest[i] = a[i] + b[i];
}

// ---------------------------------------------------------------------------
// shared by dense and sparse: the degree term, row-local (one wave per row)
//   c_i = -1/2 d_i^2 sum_{k=1..K} ( <r_k[i], h_k[i]> + <u_k[i], h_{k-1}[i]> )
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tag_rowterm(const float* __restrict__ T, const float* __restrict__ U,
                                                     const float* __restrict__ x, const float* __restrict__ hs,
                                                     const float* __restrict__ dinv, float* __restrict__ c,
                                                     int64_t R, int Fi, int K) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int lane = threadIdx.x & 63;
  const size_t hop = (size_t)R * Fi, o = (size_t)row * Fi;
  float s = 0.f;
  for (int k = 1; k <= K; ++k) {
    const float* rk = T + (size_t)k * hop + o;
    const float* uk = U + (size_t)(k - 1) * hop + o;
    const float* hk = hs + (size_t)(k - 1) * hop + o;
    const float* hp = k == 1 ? x + o : hs + (size_t)(k - 2) * hop + o;
    for (int f = lane; f < Fi; f += 64) {
      s = fmaf(rk[f], hk[f], s);
      s = fmaf(uk[f], hp[f], s);
    }
  }
  s = gcm_wave_sum(s);
  const float d = dinv[row];
  if (lane == 0) c[row] = d == 0.f ? 0.f : -0.5f * d * d * s;
}

// g_adj[b, i, j] = d_i d_j sum_{k=1..K} <r_k[b, i], h_{k-1}[b, j]> + c_i, 0 on an overwritten diagonal.
// 128 x 128 entries per workgroup, every hop and channel tile summed in the accumulators: written once.
__global__ __launch_bounds__(256) void k_tag_gadj(const float* __restrict__ T, const float* __restrict__ x,
                                                  const float* __restrict__ hs, const float* __restrict__ dinv,
                                                  const float* __restrict__ c, float* __restrict__ g_adj, int N,
                                                  int Fi, int K, int add_loop) {
  __shared__ float sR[MB * 33];   // [i][f]
  __shared__ float sHt[32 * (MB + 1)];  // [f][j]
  const int b = blockIdx.z;
  const int i0 = blockIdx.x * MB, j0 = blockIdx.y * MB;
  const int64_t R = (int64_t)gridDim.z * N;
  const size_t hop = (size_t)R * Fi, base = (size_t)b * N * Fi;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int nct = min(4, (N - j0 + 31) / 32);
  f32x16 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  for (int k = 1; k <= K; ++k) {
    const float* rk = T + (size_t)k * hop + base;
    const float* hp = (k == 1 ? x : hs + (size_t)(k - 2) * hop) + base;
    for (int f0 = 0; f0 < Fi; f0 += 32) {
      for (int e = threadIdx.x; e < MB * 32; e += 256) {
        const int r = e >> 5, f = e & 31;
        sR[r * 33 + f] = (i0 + r < N && f0 + f < Fi) ? rk[(size_t)(i0 + r) * Fi + f0 + f] : 0.f;
        sHt[f * (MB + 1) + r] = (j0 + r < N && f0 + f < Fi) ? hp[(size_t)(j0 + r) * Fi + f0 + f] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nct) mma32_tiles(acc[t], sR + wave * 32 * 33, 33, 1, sHt + t * 32, MB + 1, 1, 32, li, lh);
      __syncthreads();
    }
  }
  float* gb = g_adj + (size_t)b * N * N;
  const float* db = dinv + (size_t)b * N;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int j = j0 + t * 32 + li;
    if (t >= nct || j >= N) continue;
    const float dj = db[j];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wave * 32 + acc_row(r, lh);
      if (i >= N) continue;
      float v = db[i] * acc[t][r] * dj;
      if (c) v += c[(size_t)b * N + i];
      if (add_loop && i == j) v = 0.f;
      gb[(size_t)i * N + j] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// sparse
// ---------------------------------------------------------------------------
// one hop: with w0, out = hprev w0^T + bias first (the k = 0 term); with wk, h = gather(hprev) over the CSR, written
// to hnext, and out += h wk^T.  128 rows per workgroup; an element of out belongs to one thread throughout.
template <int NCT>
__global__ __launch_bounds__(256) void k_tag_csr_hop(const float* __restrict__ hprev,
                                                     const int64_t* __restrict__ row_ptr,
                                                     const int64_t* __restrict__ col, const float* __restrict__ coef,
                                                     const float* __restrict__ w0, const float* __restrict__ bias,
                                                     const float* __restrict__ wk, float* __restrict__ out,
                                                     float* __restrict__ hnext, int64_t M, int Fi, int Fo) {
  constexpr int FiP = 32 * NCT;
  const int64_t r0 = (int64_t)blockIdx.x * MB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  __shared__ float sAgg[MB * (FiP + 1)];
  __shared__ float sW[FiP * 33];

  for (int phase = 0; phase < 2; ++phase) {
    const float* wp = phase == 0 ? w0 : wk;
    if (!wp) continue;
    __syncthreads();
    for (int idx = threadIdx.x; idx < MB * FiP; idx += 256) {
      const int r = idx / FiP, f = idx - r * FiP;
      const int64_t row = r0 + r;
      float a = 0.f;
      if (row < M && f < Fi) {
        if (phase == 0) {
          a = hprev[(size_t)row * Fi + f];
        } else {
          const int64_t e1 = row_ptr[row + 1];
          for (int64_t e = row_ptr[row]; e < e1; ++e) a = fmaf(coef[e], hprev[(size_t)col[e] * Fi + f], a);
          hnext[(size_t)row * Fi + f] = a;
        }
      }
      sAgg[r * (FiP + 1) + f] = a;
    }
    for (int o0 = 0; o0 < Fo; o0 += 32) {
      __syncthreads();
      for (int e = threadIdx.x; e < 32 * FiP; e += 256) {  // sW[k][n] = w[o0 + n][k]
        const int n = e / FiP, k = e - n * FiP;
        sW[k * 33 + n] = (o0 + n < Fo && k < Fi) ? wp[(size_t)(o0 + n) * Fi + k] : 0.f;
      }
      __syncthreads();
      f32x16 o;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = 0.f;
      mma32_tiles(o, sAgg + wave * 32 * (FiP + 1), FiP + 1, 1, sW, 33, 1, FiP, li, lh);
      const int c = o0 + li;
      const float bv = (phase == 0 && bias && c < Fo) ? bias[c] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = r0 + wave * 32 + acc_row(r, lh);
        if (row >= M || c >= Fo) continue;
        const size_t off = (size_t)row * Fo + c;
        out[off] = phase == 0 ? o[r] + bv : out[off] + o[r];
      }
    }
  }
}

// dest[j] = tprev[j] + u[j],  u[j] = sum over the CSC column j of coef * rk[dst]   (u also to uk when given)
__global__ void k_tag_csr_chain(const float* __restrict__ rk, const float* __restrict__ tprev,
                                float* __restrict__ dest, float* __restrict__ uk,
                                const int64_t* __restrict__ col_ptr, const int64_t* __restrict__ rows,
                                const int64_t* __restrict__ perm, const float* __restrict__ coef, int64_t M, int Fi) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * Fi) return;
  const int64_t j = i / Fi;
  const int f = (int)(i - j * Fi);
  float a = 0.f;
  if (col_ptr)
    for (int64_t k = col_ptr[j]; k < col_ptr[j + 1]; ++k) a = fmaf(coef[perm[k]], rk[(size_t)rows[k] * Fi + f], a);
  if (uk) uk[i] = a;
  dest[i] = tprev[i] + a;
}

// one wave per CSR edge e (src -> dst): g = sum_k <r_k[dst], h_{k-1}[src]>;  g_w[e] = g d_src d_dst + c[dst]
__global__ __launch_bounds__(256) void k_tag_csr_gedge(const float* __restrict__ T, const float* __restrict__ x,
                                                       const float* __restrict__ hs,
                                                       const int64_t* __restrict__ col,
                                                       const int64_t* __restrict__ dst,
                                                       const float* __restrict__ dinv, const float* __restrict__ c,
                                                       float* __restrict__ g_w, int64_t M, int64_t E, int Fi, int K,
                                                       int normalize) {
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= E) return;
  const int lane = threadIdx.x & 63;
  const int64_t s = col[e], t = dst[e];
  const size_t hop = (size_t)M * Fi;
  float g = 0.f;
  for (int k = 1; k <= K; ++k) {
    const float* rk = T + (size_t)k * hop + (size_t)t * Fi;
    const float* hp = (k == 1 ? x : hs + (size_t)(k - 2) * hop) + (size_t)s * Fi;
    for (int f = lane; f < Fi; f += 64) g = fmaf(rk[f], hp[f], g);
  }
  g = gcm_wave_sum(g);
  if (lane == 0) g_w[e] = normalize ? fmaf(g, dinv[s] * dinv[t], c[t]) : g;
}

// ---------------------------------------------------------------------------
// host side shared by the two backwards
// ---------------------------------------------------------------------------
// split-K plan of the weight gradients: chunks of about 64 rows (a longer fp32 chain misses the tests' bound on a few
// hundred rows), at most 256 slabs
void tag_wsplit(int64_t R, int K, int* nsplit, int* kchunk) {
  int64_t n = std::min<int64_t>((R + 63) / 64, 256);
  n = std::max<int64_t>(1, std::min<int64_t>(n, 65535 / std::max(K, 1)));
  int64_t c = (R + n - 1) / n;
  c = (c + KT - 1) / KT * KT;
  *kchunk = (int)c;
  *nsplit = (int)((R + c - 1) / c);
}

struct TagBwdWs {
  size_t t, u, c, slabs, total;
};
TagBwdWs tag_bwd_ws(int64_t R, int Fi, int Fo, int K) {
  TagBwdWs w;
  int nsplit, kchunk;
  tag_wsplit(R, K, &nsplit, &kchunk);
  const size_t slab_f =
      std::max<size_t>((size_t)nsplit * (K + 1) * Fo * Fi, (size_t)colsum_slabs(R) * Fo);
  const size_t hop = align256((size_t)R * Fi * sizeof(float));
  Carve cv;
  w.t = cv.take((size_t)(K + 1) * R * Fi * sizeof(float));
  w.u = cv.take(std::max<size_t>(K, 1) * hop);
  w.c = cv.take(R * sizeof(float));
  w.slabs = cv.at;  // the last field: not rounded up
  w.total = w.slabs + slab_f * sizeof(float);
  return w;
}

// g_bias = column sums of g;  g_weight[k] = g^T h_k for every k: two split-K launches and one ordered slab sum
int tag_param_grads(const float* g, const float* x, const float* hs, float* g_weight, float* g_bias, float* slabs,
                    int64_t R, int Fi, int Fo, int K, hipStream_t s) {
  int rc;
  if (g_bias && (rc = colsum(g, R, Fo, g_bias, slabs, s))) return rc;
  if (!g_weight) return GCM_OK;
  int nsplit, kchunk;
  tag_wsplit(R, K, &nsplit, &kchunk);
  const int64_t wsz = (int64_t)Fo * Fi;
  MmArgs p = mm_args();
  p.A = g, p.a_is = 1, p.a_ks = Fo;
  p.B = x, p.b_ks = Fi, p.b_js = 1;
  p.C = slabs, p.c_is = Fi, p.c_js = 1, p.c_ss = (K + 1) * wsz;
  p.M = Fo, p.N = Fi, p.K = (int)R, p.kchunk = kchunk;
  if ((rc = launch_mm(p, nsplit, s))) return rc;
  if (K > 0) {
    p.B = hs, p.b_bs = R * Fi;
    p.C = slabs + wsz, p.c_bs = wsz;
    p.batch = K;
    if ((rc = launch_mm(p, nsplit, s))) return rc;
  }
  return gcm_sum_slabs(slabs, nsplit, (int)((K + 1) * wsz), g_weight, s);
}

// T[k] = g W_k for k = 0..K in one batched launch (K == 0: straight into dest0)
int tag_gw(const float* g, const float* w, float* T, int64_t R, int Fi, int Fo, int K, hipStream_t s) {
  return mm_gw(g, w, T, R, Fi, Fo, s, K + 1, (int64_t)Fo * Fi, R * Fi);
}

bool tag_unsupported(int64_t R, int Fi, int Fo, int K) {
  return Fi > 128 || Fo > 128 || R > (1 << 30) || K > 4096;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI: DenseTAGConv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_dense_tagconv_fwd_workspace_bytes(int B, int N, int Fi, int K) {
  if (B <= 0 || N <= 0 || Fi <= 0 || K < 0) return 0;
  return sizeof(float) * ((size_t)K * B * N * Fi + (size_t)B * N);
}

extern "C" int gcm_dense_tagconv_fwd(const float* x, const float* adj, const float* weight, const float* bias,
                                     float* out, void* saved, size_t saved_bytes, int B, int N, int Fi, int Fo, int K,
                                     int normalize, int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(x && adj && weight && out && saved);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && Fo > 0 && K >= 0);
  const int64_t R = (int64_t)B * N;
  if (tag_unsupported(R, Fi, Fo, K) || B > 65535) return GCM_EUNSUPPORTED;
  GCM_REQUIRE(saved_bytes >= gcm_dense_tagconv_fwd_workspace_bytes(B, N, Fi, K));
  hipStream_t s = (hipStream_t)stream;
  float* hs = (float*)saved;
  float* dinv = hs + (size_t)K * R * Fi;
  if (N <= 128) {
    const size_t lds = tag_fwd_lds(N, Fi);
    const int nci = (Fi + 31) / 32, nco = (Fo + 31) / 32;
#define TAG_FWD(I, O)                                                                                          \
  if (nci == I && nco == O) {                                                                                  \
    auto kern = k_tag_dense_fwd<I, O>;                                                                         \
    gcm_allow_dynamic_lds((const void*)kern, lds);                                                             \
    hipLaunchKernelGGL(kern, dim3(B), dim3(256), lds, s, x, adj, weight, bias, out, hs, dinv, N, Fi, Fo, K,    \
                       normalize, add_loop, tag_skip());                                                       \
  }
#define TAG_FWD_ROW(I) TAG_FWD(I, 1) TAG_FWD(I, 2) TAG_FWD(I, 3) TAG_FWD(I, 4)
    TAG_FWD_ROW(1) TAG_FWD_ROW(2) TAG_FWD_ROW(3) TAG_FWD_ROW(4)
#undef TAG_FWD_ROW
#undef TAG_FWD
    return gcm_launch_status();
  }
  hipLaunchKernelGGL(k_tag_deg, dim3(blocks(R, 4)), dim3(256), 0, s, adj, dinv, R, N, normalize, add_loop);
  int rc = gcm_launch_status();
  if (rc) return rc;
  for (int k = 1; k <= K; ++k) {   // h_k = d_i sum_j A_ij d_j h_{k-1}
    MmArgs p = mm_args();
    p.A = adj, p.a_bs = (int64_t)N * N, p.a_is = N, p.a_ks = 1, p.a_diag = add_loop, p.diag_val = 1.f;
    p.B = k == 1 ? x : hs + (size_t)(k - 2) * R * Fi, p.b_bs = (int64_t)N * Fi, p.b_ks = Fi, p.b_js = 1;
    p.b_kscale = dinv;
    p.C = hs + (size_t)(k - 1) * R * Fi, p.c_bs = (int64_t)N * Fi, p.c_is = Fi, p.c_js = 1;
    p.c_rscale = dinv, p.s_bs = N;
    p.M = N, p.N = Fi, p.K = N, p.batch = B;
    if ((rc = launch_mm(p, 1, s))) return rc;
  }
  hipLaunchKernelGGL(k_tag_lin, dim3(blocks(R, MB), (Fo + 31) / 32), dim3(256), 0, s, x, hs, weight, bias, out, R,
                     Fi, Fo, K);
  return gcm_launch_status();
}

extern "C" size_t gcm_dense_tagconv_bwd_workspace_bytes(int B, int N, int Fi, int Fo, int K) {
  if (B <= 0 || N <= 0 || Fi <= 0 || Fo <= 0 || K < 0) return 0;
  return tag_bwd_ws((int64_t)B * N, Fi, Fo, K).total;
}

extern "C" int gcm_dense_tagconv_bwd(const float* g_out, const float* x, const float* adj, const float* weight,
                                     const void* saved, float* g_x, float* g_adj, float* g_weight, float* g_bias,
                                     void* workspace, size_t workspace_bytes, int B, int N, int Fi, int Fo, int K,
                                     int normalize, int add_loop, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && adj && weight && saved && workspace);
  GCM_REQUIRE(B > 0 && N > 0 && Fi > 0 && Fo > 0 && K >= 0);
  const int64_t R = (int64_t)B * N;
  if (tag_unsupported(R, Fi, Fo, K) || B > 65535) return GCM_EUNSUPPORTED;
  const TagBwdWs L = tag_bwd_ws(R, Fi, Fo, K);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* T = (float*)(ws + L.t);
  float* U = (float*)(ws + L.u);
  float* c = (float*)(ws + L.c);
  float* slabs = (float*)(ws + L.slabs);
  const float* hs = (const float*)saved;
  const float* dinv = hs + (size_t)K * R * Fi;
  const size_t hop = (size_t)R * Fi;
  int rc;
  if ((rc = tag_param_grads(g_out, x, hs, g_weight, g_bias, slabs, R, Fi, Fo, K, s))) return rc;
  if (K == 0) {
    if (g_x && (rc = tag_gw(g_out, weight, g_x, R, Fi, Fo, 0, s))) return rc;
    if (g_adj && (rc = (int)hipMemsetAsync(g_adj, 0, sizeof(float) * (size_t)R * N, s))) return rc;
    return GCM_OK;
  }
  if (!g_x && !g_adj) return GCM_OK;
  if ((rc = tag_gw(g_out, weight, T, R, Fi, Fo, K, s))) return rc;
  const bool want_u = g_adj && normalize;
  if (N <= 128) {
    const size_t lds = tag_chain_lds(N, Fi);
    const int nci = (Fi + 31) / 32;
#define TAG_CHAIN(I)                                                                                              \
  if (nci == I) {                                                                                                 \
    auto kern = k_tag_dense_chain<I>;                                                                             \
    gcm_allow_dynamic_lds((const void*)kern, lds);                                                                \
    hipLaunchKernelGGL(kern, dim3(B), dim3(256), lds, s, adj, dinv, T, want_u ? U : nullptr, g_x, N, Fi, K,       \
                       normalize, add_loop, tag_skip());                                                          \
  }
    TAG_CHAIN(1) TAG_CHAIN(2) TAG_CHAIN(3) TAG_CHAIN(4)
#undef TAG_CHAIN
    if ((rc = gcm_launch_status())) return rc;
  } else {
    for (int k = K; k >= 1; --k) {   // u_k = A^^T r_k, r_{k-1} = T_{k-1} + u_k
      MmArgs p = mm_args();
      p.A = adj, p.a_bs = (int64_t)N * N, p.a_is = 1, p.a_ks = N, p.a_diag = add_loop, p.diag_val = 1.f;
      p.B = T + (size_t)k * hop, p.b_bs = (int64_t)N * Fi, p.b_ks = Fi, p.b_js = 1, p.b_kscale = dinv;
      p.C = U + (size_t)(k - 1) * hop, p.c_bs = (int64_t)N * Fi, p.c_is = Fi, p.c_js = 1;
      p.c_rscale = dinv, p.s_bs = N;
      p.M = N, p.N = Fi, p.K = N, p.batch = B;
      if ((rc = launch_mm(p, 1, s))) return rc;
      float* dest = (k == 1 && g_x) ? g_x : T + (size_t)(k - 1) * hop;
      hipLaunchKernelGGL(k_tag_add, dim3(blocks((int64_t)hop, 256)), dim3(256), 0, s, T + (size_t)(k - 1) * hop,
                         U + (size_t)(k - 1) * hop, dest, (int64_t)hop);
      if ((rc = gcm_launch_status())) return rc;
    }
  }
  if (!g_adj) return GCM_OK;
  if (normalize) {
    hipLaunchKernelGGL(k_tag_rowterm, dim3(blocks(R, 4)), dim3(256), 0, s, T, U, x, hs, dinv, c, R, Fi, K);
    if ((rc = gcm_launch_status())) return rc;
  }
  hipLaunchKernelGGL(k_tag_gadj, dim3((N + MB - 1) / MB, (N + MB - 1) / MB, B), dim3(256), 0, s, T, x, hs, dinv,
                     normalize ? c : nullptr, g_adj, N, Fi, K, add_loop);
  return gcm_launch_status();
}

// ---------------------------------------------------------------------------
// C ABI: TAGConv
// ---------------------------------------------------------------------------
extern "C" size_t gcm_csr_tagconv_fwd_workspace_bytes(int64_t M, int Fi, int K) {
  if (M <= 0 || Fi <= 0 || K < 0) return 0;
  return std::max<size_t>(sizeof(float) * (size_t)K * M * Fi, 256);
}

extern "C" int gcm_csr_tagconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* coef,
                                   const float* weight, const float* bias, float* out, void* saved,
                                   size_t saved_bytes, int64_t M, int64_t E, int Fi, int Fo, int K,
                                   gcm_stream_t stream) {
  GCM_REQUIRE(x && row_ptr && weight && out && saved);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && Fo > 0 && K >= 0);
  GCM_REQUIRE(E == 0 || (col && coef));
  if (tag_unsupported(M, Fi, Fo, K)) return GCM_EUNSUPPORTED;
  GCM_REQUIRE(saved_bytes >= gcm_csr_tagconv_fwd_workspace_bytes(M, Fi, K));
  hipStream_t s = (hipStream_t)stream;
  float* hs = (float*)saved;
  const dim3 grid(blocks(M, MB));
  const size_t wsz = (size_t)Fo * Fi, hop = (size_t)M * Fi;
  for (int k = (K == 0 ? 0 : 1); k <= K; ++k) {
    const float* hprev = k <= 1 ? x : hs + (size_t)(k - 2) * hop;
    const float* w0 = k <= 1 ? weight : nullptr;
    const float* wk = k == 0 ? nullptr : weight + (size_t)k * wsz;
    float* hnext = k == 0 ? nullptr : hs + (size_t)(k - 1) * hop;
    dispatch_nct((Fi + 31) / 32, [&](auto n) {
      hipLaunchKernelGGL(k_tag_csr_hop<n()>, grid, dim3(256), 0, s, hprev, row_ptr, col, coef, w0, bias, wk, out, hnext,
                         M, Fi, Fo);
    });
    const int rc = gcm_launch_status();
    if (rc) return rc;
  }
  return GCM_OK;
}

extern "C" size_t gcm_csr_tagconv_bwd_workspace_bytes(int64_t M, int64_t E, int Fi, int Fo, int K) {
  if (M <= 0 || E < 0 || Fi <= 0 || Fo <= 0 || K < 0) return 0;
  return tag_bwd_ws(M, Fi, Fo, K).total;
}

extern "C" int gcm_csr_tagconv_bwd(const float* g_out, const float* x, const int64_t* row_ptr, const int64_t* col,
                                   const int64_t* dst, const int64_t* col_ptr, const int64_t* rows,
                                   const int64_t* perm, const float* coef, const float* dinv, const float* weight,
                                   const void* saved, float* g_x, float* g_edge_weight, float* g_weight,
                                   float* g_bias, void* workspace, size_t workspace_bytes, int64_t M, int64_t E,
                                   int Fi, int Fo, int K, int normalize, gcm_stream_t stream) {
  GCM_REQUIRE(g_out && x && row_ptr && dinv && weight && saved && workspace);
  GCM_REQUIRE(M > 0 && E >= 0 && Fi > 0 && Fo > 0 && K >= 0);
  GCM_REQUIRE(E == 0 || (col && dst && coef && col_ptr && rows && perm) || (!g_x && !g_edge_weight));
  if (tag_unsupported(M, Fi, Fo, K)) return GCM_EUNSUPPORTED;
  const TagBwdWs L = tag_bwd_ws(M, Fi, Fo, K);
  GCM_REQUIRE(workspace_bytes >= L.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  float* T = (float*)(ws + L.t);
  float* U = (float*)(ws + L.u);
  float* c = (float*)(ws + L.c);
  float* slabs = (float*)(ws + L.slabs);
  const float* hs = (const float*)saved;
  const size_t hop = (size_t)M * Fi;
  const bool has_e = E > 0;
  int rc;
  if ((rc = tag_param_grads(g_out, x, hs, g_weight, g_bias, slabs, M, Fi, Fo, K, s))) return rc;
  if (K == 0) {
    if (g_x && (rc = tag_gw(g_out, weight, g_x, M, Fi, Fo, 0, s))) return rc;
    if (g_edge_weight && has_e && (rc = (int)hipMemsetAsync(g_edge_weight, 0, sizeof(float) * (size_t)E, s)))
      return rc;
    return GCM_OK;
  }
  const bool want_e = g_edge_weight && has_e;
  if (!g_x && !want_e) return GCM_OK;
  if ((rc = tag_gw(g_out, weight, T, M, Fi, Fo, K, s))) return rc;
  const bool want_u = want_e && normalize;
  for (int k = K; k >= 1; --k) {
    float* dest = (k == 1 && g_x) ? g_x : T + (size_t)(k - 1) * hop;
    hipLaunchKernelGGL(k_tag_csr_chain, dim3(blocks((int64_t)hop, 256)), dim3(256), 0, s, T + (size_t)k * hop,
                       T + (size_t)(k - 1) * hop, dest, want_u ? U + (size_t)(k - 1) * hop : nullptr,
                       has_e ? col_ptr : nullptr, rows, perm, coef, M, Fi);
    if ((rc = gcm_launch_status())) return rc;
  }
  if (!want_e) return GCM_OK;
  if (normalize) {
    hipLaunchKernelGGL(k_tag_rowterm, dim3(blocks(M, 4)), dim3(256), 0, s, T, U, x, hs, dinv, c, M, Fi, K);
    if ((rc = gcm_launch_status())) return rc;
  }
  hipLaunchKernelGGL(k_tag_csr_gedge, dim3(blocks(E, 4)), dim3(256), 0, s, T, x, hs, col, dst, dinv, c,
                     g_edge_weight, M, E, Fi, K, normalize);
  return gcm_launch_status();
}
