// The fp32 tile step every conv layer builds its dense products on, and the reductions built on it.
//
// The tile step, as device templates (below): a workgroup of 4 waves owns 128 rows x 32*NCT columns of C, K is staged
// through LDS in tiles of 32 with zero padding, the products run as mma32 on v_mfma_f32_32x32x2_f32, the stores are
// masked.  A layer's kernel is its element loaders, its epilogue and three calls:
//
//     __shared__ float sA[MB * (KT + 1)], sB[KT * (32 * NCT + 1)];
//     const TileLane t = tile_lane();
//     f32x16 acc[NCT];
//     tile_zero(acc);
//     tile_mma<NCT, false>(acc, t, sA, sB, i0, j0, M, N, kbeg, kend, a_rfast, b_kfast,
//                          [=](int gi, int gk) { return A(gi, gk); }, [=](int gk, int gj) { return B(gk, gj); });
//     tile_store(acc, t, i0, j0, M, N, [=](int j) { return [=](int i, float v) { C(i, j) = epi(v); }; });
//
// and its launcher picks NCT with dispatch_nct.  Everything inlines: a kernel pays only for the operands it has.  The
// functors capture by value ([=]): the inner functor of the epilogue outlives the call that made it, and kernel
// arguments reached through a [&] capture are no longer seen as unclobbered, which costs registers and reloads.
//
// What csrc/gcn_mm.hip defines once for the whole library (declared here): k_gcn_mm - C = epi(A B), strided and
// batched, behind launch_mm / mm_xwt / mm_gw; wgrad - a weight gradient as split-K slabs summed in order; colsum -
// column sums as slabs summed in order.  Deterministic: no atomics.
#pragma once
#include <algorithm>
#include <type_traits>

#include "fused_common.h"

namespace gcm_mm {

using gcm_fused::acc_row;
using gcm_fused::mma32;

constexpr int KT = 32;   // K tile
constexpr int MB = 128;  // rows of C per workgroup (4 waves x 32)

// acc += A(32 x KK) B(KK x 32), operands in LDS as mma32's, in K tiles of 32 that each start from a zero accumulator:
// no fp32 chain is longer than 32 products before it meets the running sum (one chain over every hop and channel of
// TAGConv's `out` - 320 products at K = 4, 64 channels - missed the tests' bound: 3.1e-6 against 2.4e-6)
__device__ __forceinline__ void mma32_tiles(f32x16& acc, const float* a, int ais, int aks, const float* b, int bks,
                                            int bjs, int KK, int li, int lh) {
  for (int k0 = 0; k0 < KK; k0 += 32) {
    f32x16 t;
#pragma unroll
    for (int r = 0; r < 16; ++r) t[r] = 0.f;
    mma32(t, a + k0 * aks, ais, aks, b + k0 * bks, bks, bjs, 32, li, lh);
    acc += t;
  }
}

// where this thread's lane stands in the workgroup's tile: wave w owns rows 32 w .. 32 w + 31
struct TileLane {
  int wave, li, lh;
};
__device__ __forceinline__ TileLane tile_lane() {
  const int lane = threadIdx.x & 63;
  return {(int)(threadIdx.x >> 6), lane & 31, lane >> 5};
}

template <int NCT>
__device__ __forceinline__ void tile_zero(f32x16 (&acc)[NCT]) {
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
}

// sA[i][k] = A(i0 + i, k0 + k) of the K tile at k0, zero outside M x kend; a_rfast: the row is the fast thread index
// (the coalesced order when A's rows are contiguous in memory)
template <typename LoadA>
__device__ __forceinline__ void tile_stage_a(float* sA, int i0, int M, int k0, int kend, bool a_rfast, LoadA load_a) {
  for (int e = threadIdx.x; e < MB * KT; e += 256) {
    const int r = a_rfast ? e % MB : e / KT, k = a_rfast ? e / MB : e % KT;
    const int gi = i0 + r, gk = k0 + k;
    float v = 0.f;
    if (gi < M && gk < kend) v = load_a(gi, gk);
    sA[r * (KT + 1) + k] = v;
  }
}

// acc += A(i0.., k) B(k, j0..) over k in [kbeg, kend), K tiles in ascending order.  sA [MB][KT + 1], sB [KT][NC + 1].
// FRESH: every K tile starts from a zero accumulator and is then added to acc (mma32_tiles); else one chain.
template <int NCT, bool FRESH, typename LoadA, typename LoadB>
__device__ __forceinline__ void tile_mma(f32x16 (&acc)[NCT], TileLane t, float* sA, float* sB, int i0, int j0, int M,
                                         int N, int kbeg, int kend, bool a_rfast, bool b_kfast, LoadA load_a,
                                         LoadB load_b) {
  constexpr int NC = 32 * NCT;
  for (int k0 = kbeg; k0 < kend; k0 += KT) {
    tile_stage_a(sA, i0, M, k0, kend, a_rfast, load_a);
    for (int e = threadIdx.x; e < KT * NC; e += 256) {
      const int k = b_kfast ? e % KT : e / NC, j = b_kfast ? e / KT : e % NC;
      const int gk = k0 + k, gj = j0 + j;
      float v = 0.f;
      if (gk < kend && gj < N) v = load_b(gk, gj);
      sB[k * (NC + 1) + j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      if constexpr (FRESH)
        mma32_tiles(acc[c], sA + t.wave * 32 * (KT + 1), KT + 1, 1, sB + c * 32, NC + 1, 1, KT, t.li, t.lh);
      else
        mma32(acc[c], sA + t.wave * 32 * (KT + 1), KT + 1, 1, sB + c * 32, NC + 1, 1, KT, t.li, t.lh);
    }
    __syncthreads();
  }
}

// The store walk: col(j) once per column j < N this lane owns - it returns the functor called with (i, value) for
// every row i < M of that column, so what depends on j alone is read once.
template <int NCT, typename Col>
__device__ __forceinline__ void tile_store(const f32x16 (&acc)[NCT], TileLane t, int i0, int j0, int M, int N,
                                           Col col) {
#pragma unroll
  for (int c = 0; c < NCT; ++c) {
    const int j = j0 + c * 32 + t.li;
    if (j >= N) continue;
    auto row = col(j);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = i0 + t.wave * 32 + acc_row(r, t.lh);
      if (i >= M) continue;
      row(i, acc[c][r]);
    }
  }
}

// the NCT of a kernel that covers n columns per workgroup (up to 128), or tiles of 128 over more
inline int nct_of(int n) { return std::clamp((n + 31) / 32, 1, 4); }

// f(std::integral_constant<int, NCT>) for NCT = min(nct, 4): the launch of a kernel's <1>..<4> instantiation
template <typename F>
void dispatch_nct(int nct, F f) {
  gcm_pick(
      [&](auto n) {
        f(n);
        return GCM_OK;
      },
      OneOf<1, 2, 3, 4>{nct >= 1 && nct <= 3 ? nct : 4});
}

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

inline MmArgs mm_args() {
  MmArgs p = {};
  p.batch = 1;
  return p;
}

int launch_mm(MmArgs p, int nsplit, hipStream_t s);

// y[R, Fo] = x[R, Fi] W^T (+ bias),  W [Fo, Fi]
int mm_xwt(const float* x, const float* w, const float* bias, float* y, int64_t R, int Fi, int Fo, hipStream_t s);

// c[R, Fi] = g[R, Fo] W,  W [Fo, Fi];  batch > 1: c + b * c_bs = g (W + b * w_bs), the one g against a stack of W
int mm_gw(const float* g, const float* w, float* c, int64_t R, int Fi, int Fo, hipStream_t s, int batch = 1,
          int64_t w_bs = 0, int64_t c_bs = 0);

// split-K plan of a weight gradient summed over R rows: (splits, rows per split)
void wgrad_split(int64_t R, int* nsplit, int* kchunk);

// The plan of the layers whose gradients pass through a gate (ResGated, GatedGraph): chunks of 64 rows (of more once
// that would be over 512 slabs).  wgrad_split keeps a few hundred rows in one fp32 accumulation chain, whose rounding
// error grows with the chain's length: at 300 rows it is six times that of chains of 64.
void wgrad_split64(int64_t R, int* nsplit, int* kchunk);

using SplitPlan = void (*)(int64_t R, int* nsplit, int* kchunk);

// g[Fo, Fi] = sum_r gy[r, :]^T x[r, :]   (rows r < R), via split-K slabs of the given plan and gcm_sum_slabs
int wgrad(const float* gy, const float* x, float* g, float* slabs, int64_t R, int Fi, int Fo, hipStream_t s,
          SplitPlan plan = wgrad_split);

constexpr int COLSUM_ROWS = 32;   // rows summed in sequence per slab; the slabs are then summed by gcm_sum_slabs

// out[f] = sum over r < R of src[r, f];  slabs: colsum_slabs(R) * F floats
int colsum(const float* src, int64_t R, int F, float* out, float* slabs, hipStream_t s);

int64_t colsum_slabs(int64_t R);

inline unsigned blocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// offsets of the fields of a workspace, each rounded up to 256 bytes: `at` is the total once every field is taken
struct Carve {
  size_t at = 0;
  size_t take(size_t bytes) {
    const size_t o = at;
    at += align256(bytes);
    return o;
  }
};

}  // namespace gcm_mm

using namespace gcm_mm;
