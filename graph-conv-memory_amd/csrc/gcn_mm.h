// The fp32 tile GEMM of the GCN and GAT layers (csrc/gcnconv.hip, csrc/gatconv.hip) and the reductions built on it:
// k_gcn_mm - C = epi(A B), strided and batched, 128 rows x 32*NCT columns per workgroup on v_mfma_f32_32x32x2_f32,
// K in tiles of 32 staged through LDS with zero padding, masked stores; wgrad - a weight gradient as split-K slabs
// summed in order; colsum - column sums as slabs summed in order.  Deterministic: no atomics.
#pragma once
#include <algorithm>

#include "fused_common.h"

namespace {

using gcm_fused::acc_row;
using gcm_fused::mma32;

constexpr int KT = 32;   // K tile
constexpr int MB = 128;  // rows of C per workgroup (4 waves x 32)

// C(b, i, j) = epi( sum_k A(b, i, k) * B(b, k, j) ),   k in [kbeg, kend) of split z
struct MmArgs {
  const float* A;
  int64_t a_bs, a_is, a_ks;
  const float* B;
  int64_t b_bs, b_ks, b_js;
  float* C;
  int64_t c_bs, c_is, c_js;
  float* C2;              // optional: the raw sum (before the epilogue), same layout as C
  int M, N, K, batch;
  int kchunk;             // split-K: blockIdx.z = split * batch + b; split s writes C + s * c_ss
  int64_t c_ss;
  int a_diag;             // A(i, i) := diag_val
  float diag_val;
  const float* b_kscale;  // B(k, j) *= b_kscale[b * s_bs + k]
  const float* c_rscale;  // C(i, j) *= c_rscale[b * s_bs + i]
  const float* c_cscale;  // C(i, j) *= c_cscale[b * s_bs + j]
  const float* c_radd;    // C(i, j) += c_radd[b * s_bs + i]
  const float* c_bias;    // C(i, j) += c_bias[j]
  int64_t s_bs;
  int c_zero_diag;        // C(i, i) := 0
};

template <int NCT>
__global__ __launch_bounds__(256) void k_gcn_mm(MmArgs p) {
  constexpr int NC = 32 * NCT;
  __shared__ float sA[MB * (KT + 1)];  // [i][k]
  __shared__ float sB[KT * (NC + 1)];  // [k][j]
  const int b = blockIdx.z % p.batch, split = blockIdx.z / p.batch;
  const int i0 = blockIdx.x * MB, j0 = blockIdx.y * NC;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
  const int kbeg = split * p.kchunk;
  const int kend = min(p.K, kbeg + p.kchunk);
  const float* Ab = p.A + (size_t)b * p.a_bs;
  const float* Bb = p.B + (size_t)b * p.b_bs;
  const float* ks = p.b_kscale ? p.b_kscale + (size_t)b * p.s_bs : nullptr;
  const bool a_rfast = p.a_is == 1 && p.a_ks != 1;  // coalesced order of the global reads
  const bool b_kfast = p.b_ks == 1 && p.b_js != 1;

  f32x16 acc[NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  for (int k0 = kbeg; k0 < kend; k0 += KT) {
    for (int e = threadIdx.x; e < MB * KT; e += 256) {
      const int r = a_rfast ? e % MB : e / KT, k = a_rfast ? e / MB : e % KT;
      const int gi = i0 + r, gk = k0 + k;
      float v = 0.f;
      if (gi < p.M && gk < kend)
        v = (p.a_diag && gi == gk) ? p.diag_val : Ab[(size_t)gi * p.a_is + (size_t)gk * p.a_ks];
      sA[r * (KT + 1) + k] = v;
    }
    for (int e = threadIdx.x; e < KT * NC; e += 256) {
      const int k = b_kfast ? e % KT : e / NC, j = b_kfast ? e / KT : e % NC;
      const int gk = k0 + k, gj = j0 + j;
      float v = 0.f;
      if (gk < kend && gj < p.N) {
        v = Bb[(size_t)gk * p.b_ks + (size_t)gj * p.b_js];
        if (ks) v *= ks[gk];
      }
      sB[k * (NC + 1) + j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCT; ++c)
      mma32(acc[c], sA + wave * 32 * (KT + 1), KT + 1, 1, sB + c * 32, NC + 1, 1, KT, li, lh);
    __syncthreads();
  }

  float* Cb = p.C + (size_t)b * p.c_bs + (size_t)split * p.c_ss;
  const size_t so = (size_t)b * p.s_bs;
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    const int j = j0 + c * 32 + li;
    if (j >= p.N) continue;
    const float cs = p.c_cscale ? p.c_cscale[so + j] : 1.f;
    const float bias = p.c_bias ? p.c_bias[j] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + wave * 32 + acc_row(r, lh);
      if (i >= p.M) continue;
      const size_t off = (size_t)i * p.c_is + (size_t)j * p.c_js;
      float v = acc[c][r];
      if (p.C2) p.C2[(size_t)b * p.c_bs + off] = v;
      if (p.c_rscale) v *= p.c_rscale[so + i];
      v *= cs;
      if (p.c_radd) v += p.c_radd[so + i];
      v += bias;
      if (p.c_zero_diag && i == j) v = 0.f;
      Cb[off] = v;
    }
  }
}

MmArgs mm_args() {
  MmArgs p = {};
  p.batch = 1;
  return p;
}

int launch_mm(MmArgs p, int nsplit, hipStream_t s) {
  if (p.kchunk <= 0) p.kchunk = p.K;
  const int nct = p.N > 96 ? 4 : (p.N > 64 ? 3 : (p.N > 32 ? 2 : 1));
  const int NC = 32 * nct;
  if ((int64_t)p.batch * nsplit > 65535) return GCM_EUNSUPPORTED;
  dim3 grid((p.M + MB - 1) / MB, (p.N + NC - 1) / NC, p.batch * nsplit);
  switch (nct) {
    case 1: hipLaunchKernelGGL(k_gcn_mm<1>, grid, dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL(k_gcn_mm<2>, grid, dim3(256), 0, s, p); break;
    case 3: hipLaunchKernelGGL(k_gcn_mm<3>, grid, dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL(k_gcn_mm<4>, grid, dim3(256), 0, s, p); break;
  }
  return gcm_launch_status();
}

// y[R, Fo] = x[R, Fi] W^T (+ bias),  W [Fo, Fi]
int mm_xwt(const float* x, const float* w, const float* bias, float* y, int64_t R, int Fi, int Fo, hipStream_t s) {
  MmArgs p = mm_args();
  p.A = x, p.a_is = Fi, p.a_ks = 1;
  p.B = w, p.b_ks = 1, p.b_js = Fi;
  p.C = y, p.c_is = Fo, p.c_js = 1, p.c_bias = bias;
  p.M = (int)R, p.N = Fo, p.K = Fi;
  return launch_mm(p, 1, s);
}

// c[R, Fi] = g[R, Fo] W,  W [Fo, Fi];  batch > 1: c + b * c_bs = g (W + b * w_bs), the one g against a stack of W
int mm_gw(const float* g, const float* w, float* c, int64_t R, int Fi, int Fo, hipStream_t s, int batch = 1,
          int64_t w_bs = 0, int64_t c_bs = 0) {
  MmArgs p = mm_args();
  p.A = g, p.a_is = Fo, p.a_ks = 1;
  p.B = w, p.b_bs = w_bs, p.b_ks = Fi, p.b_js = 1;
  p.C = c, p.c_bs = c_bs, p.c_is = Fi, p.c_js = 1;
  p.M = (int)R, p.N = Fi, p.K = Fo, p.batch = batch;
  return launch_mm(p, 1, s);
}

// split-K plan of a weight gradient summed over R rows: (splits, rows per split)
void wgrad_split(int64_t R, int* nsplit, int* kchunk) {
  int n = (int)std::min<int64_t>(256, (R + 511) / 512);
  n = std::max(n, 1);
  int64_t c = (R + n - 1) / n;
  c = (c + KT - 1) / KT * KT;
  *kchunk = (int)c;
  *nsplit = (int)((R + c - 1) / c);
}

// The plan of the layers whose gradients pass through a gate (ResGated, GatedGraph): chunks of 64 rows (of more once
// that would be over 512 slabs).  wgrad_split keeps a few hundred rows in one fp32 accumulation chain, whose rounding
// error grows with the chain's length: at 300 rows it is six times that of chains of 64.
void wgrad_split64(int64_t R, int* nsplit, int* kchunk) {
  int64_t c = std::max<int64_t>(64, (R + 511) / 512);
  c = (c + KT - 1) / KT * KT;
  *kchunk = (int)c;
  *nsplit = (int)((R + c - 1) / c);
}

using SplitPlan = void (*)(int64_t R, int* nsplit, int* kchunk);

// g[Fo, Fi] = sum_r gy[r, :]^T x[r, :]   (rows r < R), via split-K slabs of the given plan and gcm_sum_slabs
int wgrad(const float* gy, const float* x, float* g, float* slabs, int64_t R, int Fi, int Fo, hipStream_t s,
          SplitPlan plan = wgrad_split) {
  int nsplit, kchunk;
  plan(R, &nsplit, &kchunk);
  MmArgs p = mm_args();
  p.A = gy, p.a_is = 1, p.a_ks = Fo;
  p.B = x, p.b_ks = Fi, p.b_js = 1;
  p.C = slabs, p.c_is = Fi, p.c_js = 1, p.c_ss = (int64_t)Fo * Fi;
  p.M = Fo, p.N = Fi, p.K = (int)R, p.kchunk = kchunk;
  int rc = launch_mm(p, nsplit, s);
  if (rc) return rc;
  return gcm_sum_slabs(slabs, nsplit, Fo * Fi, g, s);
}

constexpr int COLSUM_ROWS = 32;   // rows summed in sequence per slab; the slabs are then summed by gcm_sum_slabs

// slabs[s, f] = sum of src[r, f] over the rows of block s
__global__ __launch_bounds__(256) void k_colsum_slabs(const float* __restrict__ src, int64_t R, int F,
                                                      float* __restrict__ slabs) {
  const int64_t r0 = (int64_t)blockIdx.x * COLSUM_ROWS;
  const int64_t r1 = min(R, r0 + COLSUM_ROWS);
  for (int f = threadIdx.x; f < F; f += 256) {
    float a = 0.f;
    for (int64_t r = r0; r < r1; ++r) a += src[(size_t)r * F + f];
    slabs[(size_t)blockIdx.x * F + f] = a;
  }
}

int colsum(const float* src, int64_t R, int F, float* out, float* slabs, hipStream_t s) {
  const int n = (int)((R + COLSUM_ROWS - 1) / COLSUM_ROWS);
  hipLaunchKernelGGL(k_colsum_slabs, dim3(n), dim3(256), 0, s, src, R, F, slabs);
  const int rc = gcm_launch_status();
  return rc ? rc : gcm_sum_slabs(slabs, n, F, out, s);
}

int64_t colsum_slabs(int64_t R) { return (R + COLSUM_ROWS - 1) / COLSUM_ROWS; }

unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// offsets of the fields of a workspace, each rounded up to 256 bytes: `at` is the total once every field is taken
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at += align256(bytes);
    return o;
  }
};

}  // namespace
