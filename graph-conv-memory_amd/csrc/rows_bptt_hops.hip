// GEMM-form backward over the records of cached steps whose live rows follow from FORWARD TEMPORAL HOPS and a row the
// host knows (cfg2's chain: DenseGCM + TemporalBackedge from empty graphs, and DenseGCM.rollout from empty graphs).
//
// Such a chain has no recurrence in its parameter gradient: layer-1 rows are final once written, and which
// rows a step aggregated follows from the row it wrote and the hop set.  So k_bptt_cached_graph's walk over the steps -
// every step behind its record's live list and coefficients, 1 KB per graph-step of which five entries mean something -
// is not needed.  With s a step of this call, j = cur[s] the row it wrote and `self` = hop 0 present, per graph
//
//     D2[s,:]    = g_mx[s,:] * act2'(mx[s,:])                                   [T x H2]
//     U[s,:]     = D2[s,:] . [W_rel2 | W_root2]      = [dAgg2 | dH1c]           [T x 64]
//     dW_rel2    = D2^T . AGG2     dW_root2 = D2^T . H1CUR     db2 = colsum D2  (AGG2 | H1CUR: the record's v section)
//     G1pre[j,:] = sum over hops h > 0 (ascending) with a step s of this call at cur[s] = j + h:  dAgg2[s,:]
//                  + (a step s' of this call wrote row j ?  dH1c[s',:] + self dAgg2[s',:]  :  0)
//     G1[j,:]    = G1pre[j,:] * act1'(cH[j,:])                                  [rows x 32]
//     dW_rel1    = G1^T . cA       dW_root1 = G1^T . cX        db1 = colsum G1
//
// - what k_bptt_cached_graph accumulates row by row from live / coef / l_cur, summed over rows instead of over steps.
//
// Two kernels compute it.  k_bptt_hops_graph_fold (further down, with its own description) is what
// gcm_dense_rows_bptt_cached_hops launches; k_bptt_hops_graph, described here, is the form before the hop sum was folded
// into the product and stays behind gcm_dense_rows_bptt_cached_hops_unfolded for the A/B.
//
// One workgroup of eight waves per graph.  Wave w owns steps 16 w .. 16 w + 15 and cache rows 16 w .. 16 w + 15: lanes
// 0-31 take the even one of a pair, lanes 32-63 the odd one, element q = lane & 31 - the operand layout of
// v_mfma_f32_32x32x2_f32 (k = the half), so D2, the v section and the cache rows go from global memory into the
// matrix cores' operands without a trip through LDS.  Phases:
//   stage  every load of the wave (its steps' mx / g_mx / v, its rows of cH / cA / cX, its tile's weights) is issued
//          before the first wait: one round of independent loads.  Rows at or beyond rows_written (uninitialised memory)
//          and steps at or beyond n_steps are read from a clamped address and replaced by zero with a SELECT
//   D2     in registers -> dW2 / db2 partials of the wave's 16 steps (16 MFMAs), and D2 into LDS [128][33]
//   U      eight 32 x 32 tiles (wave w: steps 32 (w >> 1) .., columns 32 (w & 1) ..), K = 32 (16 MFMAs) -> LDS [128][65]
//   G1     a gather through the row -> step map (LDS, from the host's table): ascending hop, then the own-step term;
//          dW1 / db1 partials of the wave's 16 rows (16 MFMAs)
//   out    the waves' partial slabs meet in LDS and are summed in wave order (eight partial sums per graph, as
//          k_bptt_cached_graph's tile_out), one slab per graph; gcm_sum_slabs_acc is the second launch.
// 48 MFMAs a wave, 384 a graph.  No atomics, no scatter: bit-reproducible.
//
// LDS: max(D2 + U + map = 128 * 33 + 128 * 65 + 128 floats = 50,688 B,  8 partial slabs of
// Pg = 2 * 1024 + 32 + 64 H2 + H2 floats <= 4160 floats = 133,120 B)  -  130 KB at H2 = 32, inside the 160 KB of a CU
// (one workgroup per CU: B graphs on 256 CUs, eight waves = two per SIMD).
#include "fused_common.h"
#include "gcm_common.h"
#include "rows_common.h"

#ifdef GCM_STAMPS   // diagnostic build only (make stamps12, tools/kstamp_bptt_hops.py): STAMP(n) = workgroup 0, wave 0
__device__ unsigned long long g_stamps[32];
extern "C" int gcm_debug_read_stamps(unsigned long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * n);
}
#endif

namespace gcm_rows {

struct HopsTable {
  unsigned char row2step[128];   // the step of this call that wrote row j, 0xff: none
  int hop[4];                    // the distinct hops 0 < h < 128, ascending; n_hops of them
  int n_hops, self;
};

__global__ __launch_bounds__(512) void k_bptt_hops_graph(StepTable tab, HopsTable ht, int T, int rows_written, long gmx_sb,
                                                         long gmx_sh, const float* __restrict__ w_rel2,
                                                         const float* __restrict__ w_root2, int act1, int act2,
                                                         unsigned o_v, const float* __restrict__ cH,
                                                         const float* __restrict__ cA, const float* __restrict__ cX,
                                                         float* __restrict__ slabs, int N, int H2) {
  constexpr int NMAX = 128, H1 = 32, F = 32, DS = 33, US = 65, NW = 8;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, q = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int act1_v = gcm_vgpr(act1), act2_v = gcm_vgpr(act2);
  extern __shared__ float sMem[];
  float* sD2 = sMem;                                      // [NMAX][DS]
  float* sU = sD2 + NMAX * DS;                            // [NMAX][US]  dAgg2 | dH1c
  int* sMap = reinterpret_cast<int*>(sU + NMAX * US);     // [NMAX]      row -> step, -1: none
  STAMP(0);

  // ---- stage: every load of this wave, issued before the first wait ---------------------------------------------------
  const int oq = q < H2 ? q : H2 - 1;
  float mxv[8], gv[8], va[8], vb[8];
  // (the steps' pointers as scalar loads of the arguments, four pairs of steps per wait, then a select per half: left to
  //  itself the compiler selects the ADDRESS and fetches the pointer with a vector load - a dependent memory round trip
  //  in front of every record load)
#pragma unroll
  for (int i4 = 0; i4 < 8; i4 += 4) {
    unsigned long long ps[4][2], pg[4][2];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int s = min(16 * wave + 2 * (i4 + k) + h, T - 1);   // (clamped: T >= 1)
        ps[k][h] = (unsigned long long)tab.saved[s];
        pg[k][h] = (unsigned long long)tab.gmx[s];
      }
    asm volatile("" : "+s"(ps[0][0]), "+s"(ps[0][1]), "+s"(ps[1][0]), "+s"(ps[1][1]), "+s"(ps[2][0]), "+s"(ps[2][1]),
                      "+s"(ps[3][0]), "+s"(ps[3][1]), "+s"(pg[0][0]), "+s"(pg[0][1]), "+s"(pg[1][0]), "+s"(pg[1][1]),
                      "+s"(pg[2][0]), "+s"(pg[2][1]), "+s"(pg[3][0]), "+s"(pg[3][1]));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = i4 + k;
      const float* sv = reinterpret_cast<const float*>(half ? ps[k][1] : ps[k][0]);
      const float* gp = reinterpret_cast<const float*>(half ? pg[k][1] : pg[k][0]);
      mxv[i] = sv[(size_t)b * H2 + oq];
      gv[i] = gp[(long)b * gmx_sb + (long)oq * gmx_sh];
      va[i] = sv[o_v + (size_t)b * 64 + q];          // agg2
      vb[i] = sv[o_v + (size_t)b * 64 + 32 + q];     // h1cur
    }
  }
  float hr[8], ar[8], xr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = 16 * wave + 2 * i + half;
    const size_t rj = ((size_t)b * N + min(j, rows_written - 1)) * 32 + q;   // (clamped: 1 <= rows_written <= N)
    hr[i] = cH[rj];
    ar[i] = cA[rj];
    xr[i] = cX[rj];
  }
  // the wave's U tile: steps 32 sb .., columns 32 ch .. of [W_rel2 | W_root2]; B operand of MFMA kk: W[2 kk + half][q]
  const int sb = wave >> 1, ch = wave & 1;
  float w2[16];
  {
    const float* src = (ch ? w_root2 : w_rel2) + q;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) w2[kk] = src[(size_t)min(2 * kk + half, H2 - 1) * H1];
  }
  int mapv = 0xff;
  if (tid < NMAX) mapv = ht.row2step[tid];
  asm volatile("" ::: "memory");
  STAMP(1);   // every load issued
#ifdef GCM_STAMPS_WAIT   // (the stamps build's second form: the round trip alone, nothing computed under it)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  STAMP(8);
#endif
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) w2[kk] = 2 * kk + half < H2 ? w2[kk] : 0.f;
  if (tid < NMAX) sMap[tid] = (mapv < T) ? mapv : -1;

  // ---- D2 of the wave's steps; dW2 / db2 partials straight from the registers ----------------------------------------
  f32x16 aR2, aT2;   // dW_rel2 [o][k], dW_root2 [o][k]
#pragma unroll
  for (int r = 0; r < 16; ++r) { aR2[r] = 0.f; aT2[r] = 0.f; }
  float db2 = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int s = 16 * wave + 2 * i + half;
    const bool on = s < T;
    const float d2 = (on && q < H2) ? gv[i] * gcm_act_grad_sel(mxv[i], act2_v) : 0.f;
    db2 += d2;
    sD2[s * DS + q] = d2;
    aR2 = __builtin_amdgcn_mfma_f32_32x32x2f32(d2, on ? va[i] : 0.f, aR2, 0, 0, 0);   // d2 (x) agg2
    aT2 = __builtin_amdgcn_mfma_f32_32x32x2f32(d2, on ? vb[i] : 0.f, aT2, 0, 0, 0);   // d2 (x) h1cur
  }
  __syncthreads();
  STAMP(2);   // D2, dW2 / db2 partials; barrier

  // ---- U = D2 . [W_rel2 | W_root2]: one 32 x 32 tile per wave (rows of steps >= T are never read: skipped) -----------
  if (32 * sb < T) {
    f32x16 aU;
#pragma unroll
    for (int r = 0; r < 16; ++r) aU[r] = 0.f;
    const float* ap = sD2 + (32 * sb + q) * DS + half;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) aU = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * kk], w2[kk], aU, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) sU[(32 * sb + gcm_fused::acc_row(r, half)) * US + 32 * ch + q] = aU[r];
  }
  __syncthreads();
  STAMP(3);   // U; barrier

  // ---- G1 of the wave's rows: the gather (ascending hop, then the own step), then dW1 / db1 partials -----------------
  f32x16 aR, aT;   // dW_rel1 [h][f], dW_root1 [h][f]
#pragma unroll
  for (int r = 0; r < 16; ++r) { aR[r] = 0.f; aT[r] = 0.f; }
  float db1 = 0.f;
  const int nh = ht.n_hops;
  const bool self = ht.self != 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int j = 16 * wave + 2 * i + half;   // (<= 127)
    const bool written = j < rows_written;
    float gpre = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int jh = j + ht.hop[k];
      bool ok = k < nh && jh >= 0 && jh < NMAX;
      const int s = sMap[ok ? jh : 0];
      ok = ok && s >= 0;
      const float t = sU[(ok ? (s & (NMAX - 1)) : 0) * US + q];
      gpre += ok ? t : 0.f;
    }
    {
      const int s = sMap[j];
      const bool ok = s >= 0;
      const int sc = ok ? (s & (NMAX - 1)) : 0;
      const float dh = sU[sc * US + 32 + q], da = sU[sc * US + q];
      gpre += ok ? dh + (self ? da : 0.f) : 0.f;
    }
    const float g1 = written ? gpre * gcm_act_grad_sel(hr[i], act1_v) : 0.f;
    db1 += g1;
    aR = __builtin_amdgcn_mfma_f32_32x32x2f32(g1, written ? ar[i] : 0.f, aR, 0, 0, 0);
    aT = __builtin_amdgcn_mfma_f32_32x32x2f32(g1, written ? xr[i] : 0.f, aT, 0, 0, 0);
  }
  __syncthreads();   // (D2 / U / the map are dead: the partial slabs take their place)
  STAMP(4);   // gather, G1, dW1 / db1 partials; barrier

  // ---- one slab per graph: dW_rel1 [H1*F] | dW_root1 [H1*F] | db1 [H1] | dW_rel2 [H2*H1] | dW_root2 [H2*H1] | db2 [H2] ----
  const int Pg = 2 * H1 * F + H1 + 2 * H2 * H1 + H2;
  const int m_root1 = H1 * F, m_b1 = 2 * H1 * F, m_rel2 = m_b1 + H1, m_root2 = m_rel2 + H2 * H1, m_b2 = m_root2 + H2 * H1;
  float* mine = sMem + (size_t)wave * Pg;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = gcm_fused::acc_row(r, half);
    mine[i * 32 + q] = aR[r];
    mine[m_root1 + i * 32 + q] = aT[r];
    if (i < H2) {
      mine[m_rel2 + i * 32 + q] = aR2[r];
      mine[m_root2 + i * 32 + q] = aT2[r];
    }
  }
  {
    const float s1 = gcm_xor32_add(db1), s2 = gcm_xor32_add(db2);
    if (lane < 32) mine[m_b1 + lane] = s1;
    if (lane < H2) mine[m_b2 + lane] = s2;
  }
  __syncthreads();
  STAMP(5);   // the eight partial slabs in LDS; barrier
  float* slab = slabs + (size_t)b * Pg;
  for (int e = tid; e < Pg; e += 512) {
    float t_ = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) t_ += sMem[(size_t)w * Pg + e];
    slab[e] = t_;
  }
  STAMP(6);   // summed in wave order, the graph's slab stored
}

// ---- the folded form ----------------------------------------------------------------------------------------------------
// The hop sum commutes with the product, so U is never formed:
//
//     D2s[j,:]   = sum over hops h > 0 (ascending) with a step s of this call at cur[s] = j + h:  D2[s,:]
//                  (+ D2[s',:] with self, s' the step of this call that wrote row j)
//     G1pre[j,:] = D2s[j,:] . W_rel2 + D2[s',:] . W_root2                       one 32 x 32 tile, K = 2 H2
//
// and the waves take ROLES instead of sixteen steps and sixteen rows each:
//   waves 0-3  (layer 2)  wave w owns steps 32 w .. 32 w + 31: their mx / g_mx / v loads, D2 -> LDS, barrier, then the
//              dW2 / db2 partials of those steps (32 MFMAs) from the registers, beside the layer-1 waves' work
//   waves 4-7  (layer 1)  wave 4 + t owns cache rows 32 t .. 32 t + 31: their cH / cA / cX loads, both weight tiles and
//              the row -> step map entries of its sources (byte loads of the kernel arguments: no map in LDS) are
//              issued before the barrier.  Behind it the A operand of the tile product is FORMED WHILE IT IS READ from
//              sD2: lane (q, half) owns row 32 t + q and the K entries 2 kk + half, which sD2 keeps contiguous
//              ([step][half][kk], 36 floats a step: four ds_read_b128 per source step, conflict-free), a source that
//              does not exist reads the zero row 128 - no select, no dependent read.  32 MFMAs leave lane (q, half)
//              holding G1pre[32 t + acc_row(r, half)][q], r = 0..15: times act1' that IS the A operand of the outer
//              products G1^T . cA and G1^T . cX, MFMA r pairing row acc_row(r, 0) with row acc_row(r, 1) (any pairing
//              of rows is a valid K order), so the lane loads its cH / cA / cX rows by that pairing and the tile goes
//              into dW1 / db1 (32 MFMAs) without a trip through LDS.
// One SIMD holds wave w and wave w + 4: a layer-2 and a layer-1 wave, 32 + 64 of the graph's 384 MFMAs.  Two barriers
// (D2 in LDS; the partial slabs in LDS) where the unfolded form has four; the partial slabs have a place of their own
// (four layer-1 partials of dW1 | db1, four layer-2 partials of dW2 | db2: each element is a sum of four, in wave order).
// LDS: 129 * 36 + 4 * 2080 + 4 * (64 H2 + H2) floats <= 85,136 B.
#ifdef GCM_STAMPS
#define STAMP_L1(i)                                                                  \
  do {                                                                               \
    if (blockIdx.x == 0 && threadIdx.x == 256) {                                     \
      unsigned long long t_;                                                         \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");    \
      g_stamps[i] = t_;                                                              \
    }                                                                                \
  } while (0)
#else
#define STAMP_L1(i)
#endif

__global__ __launch_bounds__(512) void k_bptt_hops_graph_fold(StepTable tab, HopsTable ht, int T, int rows_written,
                                                              long gmx_sb, long gmx_sh, const float* __restrict__ w_rel2,
                                                              const float* __restrict__ w_root2, int act1, int act2,
                                                              unsigned o_v, const float* __restrict__ cH,
                                                              const float* __restrict__ cA, const float* __restrict__ cX,
                                                              float* __restrict__ slabs, int N, int H2) {
  constexpr int NMAX = 128, H1 = 32, F = 32, DF = 36, NR = 4;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, q = lane & 31, half = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool layer2 = wave < NR;
  const int act1_v = gcm_vgpr(act1), act2_v = gcm_vgpr(act2);
  extern __shared__ __attribute__((aligned(16))) float sFold[];
  float* sD2 = sFold;                        // [NMAX + 1][DF]: D2[s][o] at s DF + 16 (o & 1) + (o >> 1); row NMAX: zeros
  float* sPart = sD2 + (NMAX + 1) * DF;      // NR partials of dW1 | db1, then NR partials of dW2 | db2
  const int P1 = 2 * H1 * F + H1, P2 = 2 * H2 * H1 + H2;
  STAMP(0);
  STAMP_L1(16);

  float mxv[16], gv[16], va[16], vb[16];     // layer 2: the wave's 16 pairs of steps
  float hr[16], ar[16], xr[16], wr[16], wt[16];   // layer 1: the tile's rows by the accumulator's pairing; the weight tiles
  int src[5];                                // layer 1: the sD2 row of each source of row 32 t + q (hops ascending, own step)
  const int t = wave - NR;

  // ---- stage: every load of this wave, issued before the first wait ---------------------------------------------------
  if (layer2) {
    const int oq = q < H2 ? q : H2 - 1;
    // (the steps' pointers as scalar loads of the arguments, four pairs of steps per wait, then a select per half: see
    //  k_bptt_hops_graph.  The selected pointer is cast to the GLOBAL address space: as a generic pointer it makes flat
    //  loads, which count as LDS traffic too and are waited for all at once)
    typedef const float __attribute__((address_space(1))) * gptr;
#pragma unroll
    for (int i4 = 0; i4 < 16; i4 += 4) {
      unsigned long long ps[4][2], pg[4][2];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int s = min(32 * wave + 2 * (i4 + k) + h, T - 1);   // (clamped: T >= 1)
          ps[k][h] = (unsigned long long)tab.saved[s];
          pg[k][h] = (unsigned long long)tab.gmx[s];
        }
      asm volatile("" : "+s"(ps[0][0]), "+s"(ps[0][1]), "+s"(ps[1][0]), "+s"(ps[1][1]), "+s"(ps[2][0]), "+s"(ps[2][1]),
                        "+s"(ps[3][0]), "+s"(ps[3][1]), "+s"(pg[0][0]), "+s"(pg[0][1]), "+s"(pg[1][0]), "+s"(pg[1][1]),
                        "+s"(pg[2][0]), "+s"(pg[2][1]), "+s"(pg[3][0]), "+s"(pg[3][1]));
      // (per pair mx, g_mx, then v: the waits in front of D2 are counted, so D2 of a pair starts under the later loads.
      //  mx / g_mx of ALL pairs first was measured and not kept: DESIGN 3.2)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i4 + k;
        const gptr sv = (gptr)(half ? ps[k][1] : ps[k][0]);
        const gptr gp = (gptr)(half ? pg[k][1] : pg[k][0]);
        mxv[i] = sv[(size_t)b * H2 + oq];
        gv[i] = gp[(long)b * gmx_sb + (long)oq * gmx_sh];
        va[i] = sv[o_v + (size_t)b * 64 + q];          // agg2
        vb[i] = sv[o_v + (size_t)b * 64 + 32 + q];     // h1cur
      }
    }
  } else {
    const float* hb = cH + (size_t)b * N * 32;   // (uniform bases, one 32-bit offset per lane and row)
    const float* ab = cA + (size_t)b * N * 32;
    const float* xb = cX + (size_t)b * N * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = 32 * t + gcm_fused::acc_row(r, half);
      const unsigned rj = (unsigned)min(j, rows_written - 1) * 32u + (unsigned)q;   // (clamped: 1 <= rows_written <= N)
      hr[r] = hb[rj];
      ar[r] = ab[rj];
      xr[r] = xb[rj];
    }
    // B operands of MFMA kk: W[2 kk + half][q]
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const unsigned wo = (unsigned)min(2 * kk + half, H2 - 1) * H1 + (unsigned)q;
      wr[kk] = w_rel2[wo];
      wt[kk] = w_root2[wo];
    }
    const int j = 32 * t + q;   // (<= 127)
    int mv[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int jh = j + ht.hop[k];
      mv[k] = ht.row2step[(k < ht.n_hops && jh < NMAX) ? jh : j];
    }
    mv[4] = ht.row2step[j];
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int jh = j + ht.hop[k];
      src[k] = (k < ht.n_hops && jh < NMAX && mv[k] < T) ? mv[k] : NMAX;   // (0xff: no step wrote that row)
    }
    src[4] = mv[4] < T ? mv[4] : NMAX;
  }
  asm volatile("" ::: "memory");
  STAMP(1);   // every load issued
  STAMP_L1(17);

  // ---- layer 2: D2 of the wave's steps into LDS (kept in registers for dW2 / db2); layer 1: the zero row ---------------
  if (layer2) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int s = 32 * wave + 2 * i + half;
      const bool on = s < T;
      const float d2 = (on && q < H2) ? gv[i] * gcm_act_grad_sel(mxv[i], act2_v) : 0.f;
      sD2[s * DF + 16 * (q & 1) + (q >> 1)] = d2;
      gv[i] = d2;
      va[i] = on ? va[i] : 0.f;
      vb[i] = on ? vb[i] : 0.f;
    }
  } else if (tid - 64 * NR < DF) {
    sD2[NMAX * DF + tid - 64 * NR] = 0.f;
  }
  __syncthreads();
  STAMP(2);   // D2 in LDS; barrier
  STAMP_L1(18);

  if (layer2) {
    // ---- dW2 / db2 partials straight from the registers --------------------------------------------------------------
    f32x16 aR2, aT2;   // dW_rel2 [o][k], dW_root2 [o][k]
#pragma unroll
    for (int r = 0; r < 16; ++r) { aR2[r] = 0.f; aT2[r] = 0.f; }
    float db2 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      db2 += gv[i];
      aR2 = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[i], va[i], aR2, 0, 0, 0);   // d2 (x) agg2
      aT2 = __builtin_amdgcn_mfma_f32_32x32x2f32(gv[i], vb[i], aT2, 0, 0, 0);   // d2 (x) h1cur
    }
    STAMP(3);   // dW2 / db2 partials
    float* mine = sPart + NR * P1 + wave * P2;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = gcm_fused::acc_row(r, half);
      if (i < H2) {
        mine[i * 32 + q] = aR2[r];
        mine[H2 * H1 + i * 32 + q] = aT2[r];
      }
    }
    const float s2 = gcm_xor32_add(db2);
    if (lane < H2) mine[2 * H2 * H1 + lane] = s2;
  } else {
    // ---- the tile's A operands, formed from sD2 while read: rel = the sources' sum, root = the own step ---------------
    f32x16 aR, aT;   // dW_rel1 [h][f], dW_root1 [h][f]
#pragma unroll
    for (int r = 0; r < 16; ++r) { aR[r] = 0.f; aT[r] = 0.f; }
    float db1 = 0.f;
    if (32 * t < rows_written) {   // (a tile without a written row: G1 = 0)
      float4 own[4], sum[4];
      {
        const float4* p = reinterpret_cast<const float4*>(sD2 + src[4] * DF + 16 * half);
#pragma unroll
        for (int c = 0; c < 4; ++c) own[c] = p[c];
      }
      // (a hop beyond n_hops reads the zero row like a source that does not exist: no branch between the reads)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float4* p = reinterpret_cast<const float4*>(sD2 + src[k] * DF + 16 * half);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float4 v = p[c];
          if (k == 0) {
            sum[c] = v;
          } else {
            sum[c].x += v.x; sum[c].y += v.y; sum[c].z += v.z; sum[c].w += v.w;
          }
        }
      }
      if (ht.self != 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          sum[c].x += own[c].x; sum[c].y += own[c].y; sum[c].z += own[c].z; sum[c].w += own[c].w;
        }
      }
      STAMP_L1(19);   // the A operands read and summed
      // ---- G1pre = D2s . W_rel2 + D2 . W_root2: K = 2 H2 into one accumulator ------------------------------------------
      f32x16 aG;
#pragma unroll
      for (int r = 0; r < 16; ++r) aG[r] = 0.f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float a4[4] = {sum[c].x, sum[c].y, sum[c].z, sum[c].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kk = 4 * c + e;
          aG = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], 2 * kk + half < H2 ? wr[kk] : 0.f, aG, 0, 0, 0);
        }
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float a4[4] = {own[c].x, own[c].y, own[c].z, own[c].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int kk = 4 * c + e;
          aG = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[e], 2 * kk + half < H2 ? wt[kk] : 0.f, aG, 0, 0, 0);
        }
      }
      STAMP_L1(20);   // the tile product
      // ---- G1 = G1pre * act1'(cH); the accumulator's register r is the A operand of outer product r --------------------
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool written = 32 * t + gcm_fused::acc_row(r, half) < rows_written;
        const float g1 = written ? aG[r] * gcm_act_grad_sel(hr[r], act1_v) : 0.f;
        db1 += g1;
        aR = __builtin_amdgcn_mfma_f32_32x32x2f32(g1, written ? ar[r] : 0.f, aR, 0, 0, 0);
        aT = __builtin_amdgcn_mfma_f32_32x32x2f32(g1, written ? xr[r] : 0.f, aT, 0, 0, 0);
      }
    }
    STAMP_L1(21);   // G1, dW1 / db1 partials
    float* mine = sPart + t * P1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = gcm_fused::acc_row(r, half);
      mine[i * 32 + q] = aR[r];
      mine[H1 * F + i * 32 + q] = aT[r];
    }
    const float s1 = gcm_xor32_add(db1);
    if (lane < 32) mine[2 * H1 * F + lane] = s1;
  }
  __syncthreads();
  STAMP(5);   // the partial slabs in LDS; barrier
  STAMP_L1(22);

  // ---- one slab per graph, the layout of k_bptt_hops_graph: four partials per element, in wave order ------------------
  float* slab = slabs + (size_t)b * (P1 + P2);
  for (int e = tid; e < P1 + P2; e += 512) {
    const float* p = e < P1 ? sPart + e : sPart + NR * P1 + (e - P1);
    const int st = e < P1 ? P1 : P2;
    float t_ = 0.f;
#pragma unroll
    for (int w = 0; w < NR; ++w) t_ += p[w * st];
    slab[e] = t_;
  }
  STAMP(6);   // summed in wave order, the graph's slab stored
  STAMP_L1(23);
}

}  // namespace gcm_rows

// the entries' body; fold: k_bptt_hops_graph_fold, else k_bptt_hops_graph (same arguments, same slab)
static int launch_bptt_hops(bool fold, const float* const* saved_host, const float* const* gmx_host, int n_steps,
                            long gmx_stride_b, long gmx_stride_h, const float* params, int has_bias, int act1, int act2,
                            const float* cache_nodes, const float* cache_h1, const float* cache_agg1,
                            const uint8_t* cur_host, const gcm_selector_desc* selectors, int n_selectors, int rows_written,
                            const float* g_params_prev, float* g_params, void* workspace, size_t workspace_bytes, int B,
                            int N, int F, int H1, int H2, gcm_stream_t stream) {
  GCM_REQUIRE(saved_host && gmx_host && params && g_params && workspace && cache_nodes && cache_h1 && cache_agg1 && cur_host);
  GCM_REQUIRE(n_steps > 0 && B > 0 && (selectors || n_selectors == 0));
  if (F != 32 || H1 != 32 || H2 <= 0 || H2 > 32 || N <= 0 || N > 128 || n_steps > GCM_ROWS_MAX_STEPS) return GCM_EUNSUPPORTED;
  if (has_bias & ~3) return GCM_EUNSUPPORTED;   // (no deg term, no PE table, no A/B bits)
  if (rows_written <= 0 || rows_written > N) return GCM_EUNSUPPORTED;
  gcm_rows::HopsTable ht{};
  for (int i = 0; i < n_selectors; ++i) {
    const gcm_selector_desc& d = selectors[i];
    if (d.kind != GCM_SEL_TEMPORAL || d.direction != GCM_DIR_FORWARD || d.n_hops < 0 || d.n_hops > 16) return GCM_EUNSUPPORTED;
    for (int k = 0; k < d.n_hops; ++k) {
      const int h = d.hops[k];
      if (h < 0) return GCM_EUNSUPPORTED;
      if (h == 0) { ht.self = 1; continue; }
      if (h >= 128) continue;   // (no source in a graph of <= 128 nodes: the forward skips it too)
      bool seen = false;
      for (int a = 0; a < ht.n_hops; ++a) seen = seen || ht.hop[a] == h;
      if (seen) continue;
      if (ht.n_hops == 4) return GCM_EUNSUPPORTED;
      int a = ht.n_hops++;
      for (; a > 0 && ht.hop[a - 1] > h; --a) ht.hop[a] = ht.hop[a - 1];   // ascending
      ht.hop[a] = h;
    }
  }
  for (int j = 0; j < 128; ++j) ht.row2step[j] = 0xff;
  gcm_rows::StepTable tab{};
  for (int i = 0; i < n_steps; ++i) {
    GCM_REQUIRE(saved_host[i] && gmx_host[i]);
    const int c = cur_host[i];
    if (c >= rows_written || ht.row2step[c] != 0xff) return GCM_EUNSUPPORTED;   // every row below rows_written, written once
    ht.row2step[c] = (unsigned char)i;
    tab.saved[i] = saved_host[i];
    tab.gmx[i] = gmx_host[i];
  }
  const size_t Pg = 2 * (size_t)H1 * F + H1 + 2 * (size_t)H2 * H1 + H2;
  if (workspace_bytes < sizeof(float) * Pg * (size_t)B) return GCM_EWORKSPACE;
  const gcm_rows::CachedLayout lay = gcm_rows::make_cached_layout(B, N, H1, H2);
  if (lay.total >= ((size_t)1 << 31)) return GCM_EUNSUPPORTED;
  float* slabs = (float*)workspace;
  const float* w_rel2 = params + 2 * (size_t)H1 * F + H1;
  const float* w_root2 = w_rel2 + (size_t)H2 * H1;
  if (fold) {
    const size_t lds = sizeof(float) * (129 * 36 + 4 * Pg);   // D2 and its zero row, 4 + 4 partial slabs
    gcm_allow_dynamic_lds((const void*)gcm_rows::k_bptt_hops_graph_fold, lds);
    hipLaunchKernelGGL(gcm_rows::k_bptt_hops_graph_fold, dim3(B), dim3(512), lds, (hipStream_t)stream, tab, ht, n_steps,
                       rows_written, gmx_stride_b, gmx_stride_h, w_rel2, w_root2, act1, act2, (unsigned)lay.o_v, cache_h1,
                       cache_agg1, cache_nodes, slabs, N, H2);
  } else {
    const size_t stage = sizeof(float) * (128 * 33 + 128 * 65 + 128), out = sizeof(float) * 8 * Pg;
    const size_t lds = stage > out ? stage : out;
    gcm_allow_dynamic_lds((const void*)gcm_rows::k_bptt_hops_graph, lds);
    hipLaunchKernelGGL(gcm_rows::k_bptt_hops_graph, dim3(B), dim3(512), lds, (hipStream_t)stream, tab, ht, n_steps,
                       rows_written, gmx_stride_b, gmx_stride_h, w_rel2, w_root2, act1, act2, (unsigned)lay.o_v, cache_h1,
                       cache_agg1, cache_nodes, slabs, N, H2);
  }
  const int rc = gcm_launch_status();
  if (rc) return rc;
  return gcm_sum_slabs_acc(slabs, B, (int)Pg, g_params_prev, g_params, stream);
}

#define GCM_BPTT_HOPS_ARGS                                                                                              \
  saved_host, gmx_host, n_steps, gmx_stride_b, gmx_stride_h, params, has_bias, act1, act2, cache_nodes, cache_h1,       \
      cache_agg1, cur_host, selectors, n_selectors, rows_written, g_params_prev, g_params, workspace, workspace_bytes, \
      B, N, F, H1, H2, stream

extern "C" int gcm_dense_rows_bptt_cached_hops(const float* const* saved_host, const float* const* gmx_host, int n_steps,
                                               long gmx_stride_b, long gmx_stride_h, const float* params, int has_bias,
                                               int act1, int act2, const float* cache_nodes, const float* cache_h1,
                                               const float* cache_agg1, const uint8_t* cur_host,
                                               const gcm_selector_desc* selectors, int n_selectors, int rows_written,
                                               const float* g_params_prev, float* g_params, void* workspace,
                                               size_t workspace_bytes, int B, int N, int F, int H1, int H2,
                                               gcm_stream_t stream) {
  return launch_bptt_hops(true, GCM_BPTT_HOPS_ARGS);
}

extern "C" int gcm_dense_rows_bptt_cached_hops_unfolded(const float* const* saved_host, const float* const* gmx_host,
                                                        int n_steps, long gmx_stride_b, long gmx_stride_h,
                                                        const float* params, int has_bias, int act1, int act2,
                                                        const float* cache_nodes, const float* cache_h1,
                                                        const float* cache_agg1, const uint8_t* cur_host,
                                                        const gcm_selector_desc* selectors, int n_selectors,
                                                        int rows_written, const float* g_params_prev, float* g_params,
                                                        void* workspace, size_t workspace_bytes, int B, int N, int F,
                                                        int H1, int H2, gcm_stream_t stream) {
  return launch_bptt_hops(false, GCM_BPTT_HOPS_ARGS);
}
