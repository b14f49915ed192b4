// Back-to-back lean cached steps as ONE graph node: the multi-step form of k_step_rows_cached_img4_lean and
// the capture-time merging that puts steps into it.
//
// A replayed chain of dependent kernel nodes pays ~1.6 us per node that no kernel work buys back.  While a
// stream is being captured the library sees whether step t + 1 follows step t with nothing in between: the stream's only
// pending dependency is then the node step t became.  No captured work can observe the state between the two steps, so
// step t + 1 is appended to that node's argument table (n -> n + 1) instead of being launched; the node runs
// k_step_rows_cached_img4_lean_run, which makes the n steps inside one workgroup per graph.
//
// The kernel's step is the lean kernel's, operation for operation (the product chain of rows_lean.h, the same source
// order and association, gcm_tanh), so beliefs, records, caches, state and flags are the bits the per-step launches write.
// What changes is where its inputs come from and who makes which step:
//   * in a chain of cached steps a step's layer 1 reads observations alone (its own and those of the rows cur - hop) and
//     its layer 2 the h1 rows of those same rows (a layer-1 row is final once written), so inside one launch
//     the steps do not wait for one another: each of the workgroup's eight waves takes the step pairs p = w, w + 8, ...
//     (steps 2 p and 2 p + 1, one per half-wave: a lane makes both K halves of its output column, lean_half_chain
//     twice, added in the order in which the lean kernel's half-waves meet), in three phases with a workgroup barrier
//     between them - observations into LDS; layer 1 of every step; layer 2 of every step;
//   * the graph's x and h1 rows live in LDS by row (2 x N x 32 floats <= 32 KB): the rows from before the run's first
//     step - at most max(hop) of them - are loaded from nodes / cH up front, a step's own rows are written there by the
//     wave that makes it, and the source rows are read from there behind the barrier.  Nothing this launch stored to
//     global memory is read back (the vector L1 may still hold the old line);
//   * the weight image is loaded once per workgroup into LDS (16 KB, both K halves of a column side by side); a wave
//     takes a layer's 64 registers per lane from there before that layer's phase.  Every global load of the launch -
//     observations and record pointers (two steps per instruction: half-waves), earlier rows, weights - is issued
//     before the first wait, and every store is fire and forget: loads and stores share one in-order vmcnt on this ISA
//     (rollout_persist.hip), so a load behind stores would drain them;
//   * the source rows of row cur are resolved once: from row max(hop) on every slot is live and row cur - hop lies at a
//     fixed distance from row cur in both LDS images; only the rows before that resolve their slots step by step;
//   * what follows from cur and the hops alone (adjacency entries, the record's live list / coefficients / header) is
//     written at the end in closed form, eight lanes per step and eight steps per wave instruction, the count once
//     with the run's last value.
//
// The same reasoning removes the rollout's head launch (k_head_fused, head_fused.hip) when it sits directly in front of
// step 0: the node that replaces the lean node at the first append is added on the head's dependencies and runs the
// kernel's FRESH form, which does the head's work itself ("the head absorbed" below; gcm_hip_run_head.h).
#include <atomic>
#include <new>
#include <type_traits>

#include "fused_common.h"
#include "gcm_common.h"
#include "rows_common.h"
#include "rows_head.h"
#include "rows_lean.h"

namespace gcm_rows {

constexpr int RUN_CAP = GCM_ROWS_MAX_STEPS;   // two tables of 128 pointers: 2 KB of the 4 KB of kernel arguments
constexpr int RUN_WAVES = 8;
constexpr int RUN_PAIRS = RUN_CAP / 2 / RUN_WAVES;   // passes per wave (two steps each, one per half-wave)
constexpr int RUN_OCTS = RUN_CAP / 8 / RUN_WAVES;    // phase D passes per wave (eight steps each)
constexpr int RUN_WSTAGE = 2 * 16 * 64 / (64 * RUN_WAVES);   // weight pairs a thread carries into LDS

struct RunTable {
  const float* obs[RUN_CAP];
  float* rec[RUN_CAP];
};

// What the fresh-state form (FRESH) does in place of the rollout's head launch (k_head_fused, absorbed at capture time:
// "the head absorbed" below): the head's sources, the packed vector and the image it wrote, and the 64-float paddings of
// the state allocation nodes | adj | count it zeroed (floats from `nodes`: [pad0, pad0_end) and [pad1, pad1_end)).
struct FreshArgs {
  HeadSrcs hs;
  float* packed;
  float* image;
  unsigned pad0, pad0_end, pad1, pad1_end;
};
struct NoFresh {};
constexpr int RUN_ADJ_TAB = 256 + 128;   // FRESH: the adjacency pattern by column - row + 128, then a row of zeros

// Where the FRESH form's state / image / packed stores sit: 0 behind the first barrier (the pattern table is made in
// phase A), 1 at the end with phase D.  Measured on cfg2 (profiles/r12_bench_cfg2_cuts.jsonl): 0.0604 - 0.0614 ms per
// rollout against 0.0614 - 0.0634 - issued early they drain under phases B and C.
#ifndef GCM_RUN_FRESH_STORES_LATE
#define GCM_RUN_FRESH_STORES_LATE 0
#endif

// Timing-only builds of the VALU form (their outputs are wrong; run under a kernel trace alone): 1 leaves its layer-2 loop
// out, 2 both layer loops - what the layers cost in the eight-wave form (profiles/r14_bench_cfg2_cuts.jsonl).
#ifndef GCM_RUN_CUT
#define GCM_RUN_CUT 0
#endif
// ... and of the matrix-core form, a mask: 1 leaves the matrix instructions out, 2 the tanh, 4 the layers' global stores.
#ifndef GCM_RUN_MFMA_CUT
#define GCM_RUN_MFMA_CUT 0
#endif
// The matrix-core form's distance between LDS rows in floats (a multiple of 2, >= 32).  36 puts the 8-byte operand reads
// of a tile's sixteen rows on distinct banks; with 32 they meet on eight and the launch took 19.3 us against 14.7 (the same file).
#ifndef GCM_RUN_MFMA_RS
#define GCM_RUN_MFMA_RS 36
#endif

// hops4: the distinct hops 0 < h < 128 ASCENDING, one byte each, 0xff in the unused slots.  nhs: N | H2 << 8 | self << 16.
// Steps t < n <= RUN_CAP: row cur0 + t < N, observation tab.obs[t] [B, 32], record tab.rec[t] (o_*: CachedLayout;
// rec = 0: mx alone).
//
// FRESH: the run starts at row 0 of the empty graphs the rollout's head launch would have made, and that launch is not
// in the graph: this kernel does its work ("the head absorbed").  N % 4 == 0, cur0 == 0.
//   * the weights come from the parameter tensors themselves (fr.hs: W_rel1, W_root1, b1, W_rel2, W_root2, b2 lead it),
//     sixteen bytes of a row per load, and reach the LDS image through the index map k_head_fused writes layout 3 with
//     (rows_head.h); `image` and `params` are not read;
//   * the packed vector and the three image layouts are written to global memory for the backward and later launches:
//     workgroup g makes elements g, g + B, ... with k_head_fused's own expressions (the first round's loads are issued
//     with the other loads; further rounds, at B < 32, run at the end);
//   * the graph's state is written whole: node rows [n, N) zero, adjacency rows [0, n) in closed form - one 16-byte
//     store per four columns, 1.0 at the sources (and at cur with self) and 0.0 elsewhere, read from a pattern table in
//     LDS indexed by column - row - and rows [n, N) zero; workgroup 0 zeroes the paddings of the allocation.  Every
//     address is stored once, so no order between waves is needed; phase D's scalar adjacency stores are left out.
//
// MFMA: phases B and C on the fp32 matrix cores ("the layers on the matrix cores").  A wave owns the
// sixteen steps 16 w ... 16 w + 15 and both column tiles of their 32 outputs; each of lean_half_chain's eight chains
// (K half x parity x rel | root) is one accumulator of v_mfma_f32_16x16x4_f32, whose result is the k-ordered fmaf chain
// from the accumulator: two instructions per chain, then the chain's own tree of adds.  The LDS rows are 36 floats
// apart there, so that the 8-byte operand reads of sixteen rows fall on distinct banks.
template <bool FRESH, bool MFMA>
__global__ __launch_bounds__(64 * RUN_WAVES) void k_step_rows_cached_img4_lean_run(
    const float* __restrict__ image, float* __restrict__ nodes, float* __restrict__ cH, const float* __restrict__ params,
    int cur0_arg, int n, unsigned hops4, unsigned nhs, float* __restrict__ adj, int64_t* __restrict__ count,
    float* __restrict__ cA, float* __restrict__ cX, uint32_t* __restrict__ flags, unsigned o_v, unsigned o_hdr,
    unsigned o_coef, unsigned o_live, int rec, RunTable tab, std::conditional_t<FRESH, FreshArgs, NoFresh> fr) {
  constexpr int F = 32, H1 = 32, RS = MFMA ? GCM_RUN_MFMA_RS : 32, ROWS = 128 * RS;   // RS: floats from an LDS row to the next
  const int cur0 = FRESH ? 0 : cur0_arg;
  __shared__ __attribute__((aligned(16))) float sXH[2 * ROWS];            // x rows [128][32] | h1 rows [128][32]
  __shared__ __attribute__((aligned(16))) float svw[MFMA ? 4 : RUN_WAVES * 128];   // each wave's lane exchange: two steps' vectors
  __shared__ __attribute__((aligned(16))) f32x2 sW[2 * 16 * 32 * 2];      // image3 as [layer][k][h][K half]: 16 KB
  __shared__ float sadj[FRESH ? RUN_ADJ_TAB : 1];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned gb = blockIdx.x;
  const unsigned N = nhs & 0xffu;
  const int H2 = (int)((nhs >> 8) & 0xffu);
  const bool self = (nhs >> 16) & 1u;
  const unsigned g0 = gb * N;
  // a wave makes two steps per pass, one per half-wave: lane (fl, hs) is output column fl of step 2 p + hs of pair p
  const int fl = lane & 31, hs = lane >> 5;
  float* sv = svw + 128 * wv + 64 * hs;
  const int ol = fl < H2 ? fl : H2 - 1;
  // ---- phase A: every global load of the launch ------------------------------------------------------------------
  // the records of phase D's steps (eight lanes per step: oct o = steps 8 o ... 8 o + 7, this wave's are o = w, w + 8, ...)
  float* recd[RUN_OCTS];
#pragma unroll
  for (int j = 0; j < RUN_OCTS; ++j) {
    const int t = 8 * (wv + RUN_WAVES * j) + (lane >> 3);
    recd[j] = tab.rec[t < n ? t : n - 1];
  }
  // the observations and records of this wave's pairs p = w, w + 8, ...; a step past the run's end doubles the last one
  // (and stores nothing)
  float xo[RUN_PAIRS];
  float* recp[RUN_PAIRS];
#pragma unroll
  for (int j = 0; j < RUN_PAIRS; ++j) {
    const int t = 2 * (wv + RUN_WAVES * j) + hs;
    const int tc = t < n ? t : n - 1;
    xo[j] = tab.obs[tc][gb * F + fl];
    recp[j] = tab.rec[tc];
  }
  // the weight image goes through LDS, loaded once per workgroup: a lane needs both K halves of a layer (64 registers),
  // so layer 2's wait there until phase C
  f32x2 wst[RUN_WSTAGE];
  f32x4 wq[2];
  float bias1, bias2;
  // MFMA: operand layout - lane (ar, ak) holds row ar of the wave's sixteen and k group ak; result layout - column
  // ar + 16 ct, rows 4 ak + v.  The records of those rows and the biases of those columns
  const int ar = lane & 15, ak = lane >> 4;
  float* rec_a = nullptr;
  float* rec_c[4] = {nullptr, nullptr, nullptr, nullptr};
  float b1c[2] = {0.f, 0.f}, b2c[2] = {0.f, 0.f};
  if constexpr (MFMA) {
    const int ta = 16 * wv + ar;
    rec_a = tab.rec[ta < n ? ta : n - 1];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int tc = 16 * wv + 4 * ak + v;
      rec_c[v] = tab.rec[tc < n ? tc : n - 1];
    }
  }
  // FRESH: this workgroup's first elements of the image and of the packed vector (element gb + B * thread)
  float v_img = 0.f, v_pack = 0.f;
  const size_t e_first = (size_t)gb + (size_t)gridDim.x * threadIdx.x, e_wave = (size_t)gb + (size_t)gridDim.x * (64 * wv);
  if constexpr (!FRESH) {
    const f32x2* i3 = reinterpret_cast<const f32x2*>(image + 2 * 4 * 64 * 64);   // image3 (k_cached_weight_image)
#pragma unroll
    for (int r = 0; r < RUN_WSTAGE; ++r) wst[r] = i3[(int)threadIdx.x + 64 * RUN_WAVES * r];
    const float* b1 = params + 2 * H1 * F;
    bias1 = b1[fl];
    bias2 = b1[H1 + 2 * H2 * H1 + ol];
    if constexpr (MFMA) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int col = 16 * ct + ar;
        b1c[ct] = b1[col];
        b2c[ct] = b1[H1 + 2 * H2 * H1 + (col < H2 ? col : H2 - 1)];
      }
    }
  } else {
    // quad q = thread + 512 r of [m][h][k / 4]: columns 4 (q & 7) ... + 3 of row h of matrix m (zero past row H2)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int q = (int)threadIdx.x + 64 * RUN_WAVES * r;
      const int m = q >> 8, h = (q >> 3) & 31;
      const float* w = m == 0 ? fr.hs.p[0] : m == 1 ? fr.hs.p[1] : m == 2 ? fr.hs.p[3] : fr.hs.p[4];
      wq[r] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m < 2 || h < H2) wq[r] = *reinterpret_cast<const f32x4*>(w + h * 32 + 4 * (q & 7));
    }
    bias1 = fr.hs.p[2][fl];
    bias2 = fr.hs.p[5][ol];
    if constexpr (MFMA) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int col = 16 * ct + ar;
        b1c[ct] = fr.hs.p[2][col];
        b2c[ct] = fr.hs.p[5][col < H2 ? col : H2 - 1];
      }
    }
    if (e_wave < (size_t)IMG_LAYOUT_FLOATS && e_first < (size_t)IMG_LAYOUT_FLOATS) {
      const int e = (int)e_first;
      v_img = head_image_value(fr.hs, e >> 12, (e >> 6) & 63, e & 63, F, H1, H2);
    }
    if (e_wave < fr.hs.off[HEAD_MAX_SRCS] && e_first < fr.hs.off[HEAD_MAX_SRCS])
      v_pack = head_packed_value(fr.hs, (unsigned)e_first);
  }
  // the rows from before the run that a step of it can read: [cur0 - max(hop), cur0), x (lanes 0 - 31) and h1 (32 - 63)
  int hmax = 0, nh = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int h = (int)((hops4 >> (8 * i)) & 0xffu);
    if (h != 0xff) {
      ++nh;
      if (h > hmax) hmax = h;
    }
  }
  {
    const int lo = cur0 - hmax > 0 ? cur0 - hmax : 0;
    const float* src = hs ? cH : nodes;
    for (int r = lo + wv; r < cur0; r += RUN_WAVES) sXH[hs * ROWS + r * RS + fl] = src[(g0 + (unsigned)r) * 32 + fl];
  }
  if constexpr (!FRESH) {
#pragma unroll
    for (int r = 0; r < RUN_WSTAGE; ++r) {   // image3 element (layer, k, lane l): [layer][k][l & 31][l >> 5]
      const int e = (int)threadIdx.x + 64 * RUN_WAVES * r;
      sW[image3_lds_pair(e)] = wst[r];
    }
  } else {
    float* sWf = reinterpret_cast<float*>(sW);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int q = (int)threadIdx.x + 64 * RUN_WAVES * r;
#pragma unroll
      for (int u = 0; u < 4; ++u) sWf[image3_lds_index(q >> 8, 4 * (q & 7) + u, (q >> 3) & 31)] = wq[r][u];
    }
    // the adjacency pattern: entry x is column - row + 128, 1.0 where row - column is a hop (or 0 with self); from 256
    // on a row of zeros (the rows past the run's end)
    if (threadIdx.x < RUN_ADJ_TAB) {
      const int d = 128 - (int)threadIdx.x;
      bool hit = d == 0 && self;
#pragma unroll
      for (int i = 0; i < 4; ++i) hit = hit || (d > 0 && (int)((hops4 >> (8 * i)) & 0xffu) == d);
      sadj[threadIdx.x] = hit && threadIdx.x < 256 ? 1.f : 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < RUN_PAIRS; ++j) {   // the observations: x rows in LDS, rows of the node matrix and of its cache
    const int t = 2 * (wv + RUN_WAVES * j) + hs;   // (rows cur and cur + 1 are 64 consecutive floats)
    if (t < n) {
      sXH[(cur0 + t) * RS + fl] = xo[j];
      const unsigned at = (g0 + (unsigned)(cur0 + t)) * F + fl;
      nodes[at] = xo[j];
      cX[at] = xo[j];
    }
  }
  __syncthreads();
  // FRESH: what the head launch wrote, and the rest of this graph's state (no load follows: loads and stores share vmcnt)
  auto fresh_stores = [&]() {
    if constexpr (FRESH) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const int nq = (int)(N >> 2);   // 16-byte stores per adjacency row: a half-wave makes a row
      f32x4* arow = reinterpret_cast<f32x4*>(adj + (size_t)g0 * N);
      for (int r = 2 * wv + hs; r < (int)N; r += 2 * RUN_WAVES) {
        if (fl < nq) {
          const float* at = sadj + (r < n ? 128 + 4 * fl - r : 256);
          arow[r * nq + fl] = f32x4{at[0], at[1], at[2], at[3]};
        }
      }
      f32x4* nrow = reinterpret_cast<f32x4*>(nodes + (size_t)g0 * F);
      for (int i = n * (F / 4) + (int)threadIdx.x; i < (int)N * (F / 4); i += 64 * RUN_WAVES) nrow[i] = z;
      if (gb == 0 && threadIdx.x < 64) {
        if (fr.pad0 + threadIdx.x < fr.pad0_end) nodes[fr.pad0 + threadIdx.x] = 0.f;
        if (fr.pad1 + threadIdx.x < fr.pad1_end) nodes[fr.pad1 + threadIdx.x] = 0.f;
      }
      if (e_wave < (size_t)IMG_LAYOUT_FLOATS && e_first < (size_t)IMG_LAYOUT_FLOATS) head_image_store(fr.image, (int)e_first, v_img);
      if (e_wave < fr.hs.off[HEAD_MAX_SRCS] && e_first < fr.hs.off[HEAD_MAX_SRCS]) fr.packed[e_first] = v_pack;
    }
  };
  if (!GCM_RUN_FRESH_STORES_LATE) fresh_stores();
  // the source rows of row cur, ascending and compacted as the lean kernel's host resolves them: the k hops <= cur are
  // the first k of the ascending list, slot q holds row cur - hop[k - 1 - q]; an empty slot reads row 0 and adds nothing
  auto sources = [&](int cur, const float* rows, float (&va)[4]) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) k += (int)(((hops4 >> (8 * i)) & 0xffu) <= (unsigned)cur);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = k - 1 - q;
      const bool any = idx >= 0;
      const int s = any ? cur - (int)((hops4 >> (8 * (idx & 3))) & 0xffu) : 0;
      const float v = rows[s * 32 + fl];
      va[q] = any ? v : 0.f;
    }
  };
  // From row max(hop) on every hop reaches a stored row (k = nh for good): slot q is row cur - hop[nh - 1 - q], at a
  // distance from row cur that is the same for every step and for both layers - resolved here, once.  Rows before
  // that (and every row of a run whose largest hop is >= N: cur < N <= max(hop)) go through sources().
  int back[4];
  bool has[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = nh - 1 - q;
    has[q] = idx >= 0;
    back[q] = has[q] ? 32 * (int)((hops4 >> (8 * (idx & 3))) & 0xffu) : 0;
  }
  auto sources_all = [&](int cur, const float* rows, float (&va)[4]) {
    const float* at = rows + cur * 32 + fl;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float v = *(at - back[q]);
      va[q] = has[q] ? v : 0.f;
    }
  };
  // a layer's weights from LDS: wa = K half 0, wb = K half 1 of column fl
  f32x2 wa[16], wb[16];
  auto weights = [&](int layer) {
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(sW + ((layer * 16 + k) * 32 + fl) * 2);
      wa[k] = f32x2{q[0], q[1]};
      wb[k] = f32x2{q[2], q[3]};
    }
  };
  // the layer's two products of one step in ONE lane: the two half-wave chains of lean_half_matvec, met in its order
  auto matvec = [&]() { return lean_half_chain(wa, sv, 0) + lean_half_chain(wb, sv, 1); };
  // ---- the matrix-core form of a layer (MFMA) -------------------------------------------------------------------------
  // This wave's steps are 16 w ... 16 w + 15.  In the operand layout lane (ar, ak) holds, of row ar, the columns
  // f = 2 ak + 8 qf + p (qf < 4, p < 2) of the aggregate and of the row itself: the A operand of instruction i of the
  // chain (K half kh, parity p) is column 16 kh + 2 (4 i + ak) + p, so qf = 2 kh + i, and the instruction's k index ak
  // runs through the chain's j = 4 i ... 4 i + 3 in order.  The B operand is W[h = ar + 16 ct][that column], from the
  // LDS image (one 16-byte read holds both K halves and both matrices).  A step past the run's end doubles the last.
  const bool act = 16 * wv < n;   // (by wave)
  const bool live_a = 16 * wv + ar < n;
  const int cur_a = cur0 + (live_a ? 16 * wv + ar : n - 1);
  int so[4];
  bool sa[4];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) k += (int)(((hops4 >> (8 * i)) & 0xffu) <= (unsigned)cur_a);
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // (sources() by row: slot q is row cur - hop[k - 1 - q], an empty slot adds 0.f)
      const int idx = k - 1 - q;
      sa[q] = idx >= 0;
      so[q] = sa[q] ? RS * (cur_a - (int)((hops4 >> (8 * (idx & 3))) & 0xffu)) : 0;
    }
  }
  auto operands = [&](const float* rows, f32x2 (&ag)[4], f32x2 (&own)[4]) {
    const float* at = rows + 2 * ak;
#pragma unroll
    for (int qf = 0; qf < 4; ++qf) {
      own[qf] = *reinterpret_cast<const f32x2*>(at + cur_a * RS + 8 * qf);
      f32x2 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x2 u = *reinterpret_cast<const f32x2*>(at + so[q] + 8 * qf);
        v[q] = sa[q] ? u : f32x2{0.f, 0.f};
      }
      ag[qf] = (v[0] + v[1]) + (v[2] + v[3]);
      ag[qf] = ag[qf] + (self ? own[qf] : f32x2{0.f, 0.f});
    }
  };
  // the sixteen chains of the wave's tile, acc[ct][kh][p][rel | root], each from +0: instruction i = 0 of every chain,
  // then i = 1 (no instruction waits for its own predecessor)
  f32x4 acc[2][2][2][2];
  auto products = [&](int layer, const f32x2 (&ag)[4], const f32x2 (&own)[4]) {
    const float* sWf = reinterpret_cast<const float*>(sW);
    f32x4 bw[2][2][2];   // [i][p][ct]: {K half 0 rel, root, K half 1 rel, root}
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
          bw[i][p][ct] = *reinterpret_cast<const f32x4*>(sWf + ((layer * 16 + 8 * i + 2 * ak + p) * 32 + 16 * ct + ar) * 4);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int m = 0; m < 2; ++m) acc[ct][kh][p][m] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (GCM_RUN_MFMA_CUT & 1) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[ct][0][0][0] = f32x4{ag[0][0] + bw[0][0][ct][0], own[1][1] + bw[1][1][ct][1], ag[2][0], own[3][1]};
      return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            const int qf = 2 * kh + i;
            acc[ct][kh][p][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag[qf][p], bw[i][p][ct][2 * kh], acc[ct][kh][p][0], 0, 0, 0);
            acc[ct][kh][p][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(own[qf][p], bw[i][p][ct][2 * kh + 1], acc[ct][kh][p][1], 0, 0, 0);
          }
  };
  // lean_half_chain's tree on the chains of result (ct, v): per K half (rel 0 + rel 1) + (root 0 + root 1), half 0 + half 1
  auto tree = [&](int ct, int v) {
    const float s0 = (acc[ct][0][0][0][v] + acc[ct][0][1][0][v]) + (acc[ct][0][0][1][v] + acc[ct][0][1][1][v]);
    const float s1 = (acc[ct][1][0][0][v] + acc[ct][1][1][0][v]) + (acc[ct][1][0][1][v] + acc[ct][1][1][1][v]);
    return s0 + s1;
  };
  auto run_tanh = [](float v) { return (GCM_RUN_MFMA_CUT & 2) ? v : gcm_tanh(v); };
  constexpr bool STORES = !(GCM_RUN_MFMA_CUT & 4);
  bool bad = false;
  // ---- phase B: layer 1 of this wave's steps (reads x rows, writes h1 rows) ------------------------------------------
  if constexpr (MFMA) {
    if (act) {
      f32x2 ag[4], own[4];
      operands(sXH, ag, own);
      if (STORES && live_a) {
        float* to = cA + (size_t)(g0 + (unsigned)cur_a) * F + 2 * ak;
#pragma unroll
        for (int qf = 0; qf < 4; ++qf) *reinterpret_cast<f32x2*>(to + 8 * qf) = ag[qf];
      }
      products(0, ag, own);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int t = 16 * wv + 4 * ak + v;
          const float h1c = run_tanh(b1c[ct] + tree(ct, v));
          if (t < n) {
            sXH[ROWS + (cur0 + t) * RS + 16 * ct + ar] = h1c;
            if (STORES) cH[(size_t)(g0 + (unsigned)(cur0 + t)) * H1 + 16 * ct + ar] = h1c;
          }
        }
    }
  }
  if constexpr (!MFMA) weights(0);
  auto layer1 = [&](int cur, bool live, const float (&xa)[4]) {
    const unsigned rc = g0 + (unsigned)cur;
    const float xc = sXH[cur * 32 + fl];
    asm volatile("" ::: "memory");
    // (the sums img4b's mask walk makes: sources ascending, (v0 + v1) + (v2 + v3))
    float agg1 = (xa[0] + xa[1]) + (xa[2] + xa[3]);
    agg1 = agg1 + (self ? xc : 0.f);
    *reinterpret_cast<f32x2*>(sv + 2 * fl) = f32x2{agg1, xc};
    asm volatile("" ::: "memory");   // (lanes exchange through LDS; one wave: its LDS operations execute in order)
    const float p1 = bias1 + matvec();
    const float h1c = gcm_tanh(p1);
    asm volatile("" ::: "memory");
    if (live) {
      sXH[ROWS + cur * 32 + fl] = h1c;
      cA[rc * F + fl] = agg1;
      cH[rc * H1 + fl] = h1c;
    }
  };
  if constexpr (!MFMA && GCM_RUN_CUT < 2) {   // (the VALU form)
#pragma unroll
    for (int j = 0; j < RUN_PAIRS; ++j) {
      const int t0 = 2 * (wv + RUN_WAVES * j);
      if (t0 >= n) break;
      const bool live = t0 + hs < n;
      const int cur = cur0 + (live ? t0 + hs : n - 1);
      float xa[4];
      if (cur0 + t0 < hmax) sources(cur, sXH, xa);
      else sources_all(cur, sXH, xa);
      layer1(cur, live, xa);
    }
  }
  __syncthreads();
  // ---- phase C: layer 2 of this wave's steps (reads h1 rows) --------------------------------------------------------
  if constexpr (MFMA) {
    if (act) {
      f32x2 ag[4], own[4];
      operands(sXH + ROWS, ag, own);
      if (STORES && rec && live_a) {   // the record's v section: (agg2 | h1) of the row
        float* to = rec_a + o_v + gb * 2 * H1 + 2 * ak;
#pragma unroll
        for (int qf = 0; qf < 4; ++qf) {
          *reinterpret_cast<f32x2*>(to + 8 * qf) = ag[qf];
          *reinterpret_cast<f32x2*>(to + H1 + 8 * qf) = own[qf];
        }
      }
      products(1, ag, own);
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const bool out = 16 * wv + 4 * ak + v < n && 16 * ct + ar < H2;
          const float mx = run_tanh(b2c[ct] + tree(ct, v));
          if (STORES && out) rec_c[v][gb * H2 + 16 * ct + ar] = mx;
          bad = bad || (out && !isfinite(mx));
        }
    }
  }
  if constexpr (!MFMA) weights(1);
  auto layer2 = [&](int cur, bool live, float* saved, const float (&ha)[4]) {
    const float h1c = sXH[ROWS + cur * 32 + fl];
    asm volatile("" ::: "memory");
    float agg2 = (ha[0] + ha[1]) + (ha[2] + ha[3]);
    agg2 = agg2 + (self ? h1c : 0.f);
    *reinterpret_cast<f32x2*>(sv + 2 * fl) = f32x2{agg2, h1c};
    asm volatile("" ::: "memory");
    const float p2 = bias2 + matvec();
    const float v = gcm_tanh(p2);
    asm volatile("" ::: "memory");
    if (live && fl < H2) saved[gb * H2 + fl] = v;
    if (rec && live) {
      saved[o_v + gb * 2 * H1 + fl] = agg2;
      saved[o_v + gb * 2 * H1 + H1 + fl] = h1c;
    }
    bad = bad || (live && fl < H2 && !isfinite(v));
  };
  if constexpr (!MFMA && GCM_RUN_CUT < 1) {   // (the VALU form)
#pragma unroll
    for (int j = 0; j < RUN_PAIRS; ++j) {
      const int t0 = 2 * (wv + RUN_WAVES * j);
      if (t0 >= n) break;
      const bool live = t0 + hs < n;
      const int cur = cur0 + (live ? t0 + hs : n - 1);
      float ha[4];
      if (cur0 + t0 < hmax) sources(cur, sXH + ROWS, ha);
      else sources_all(cur, sXH + ROWS, ha);
      layer2(cur, live, recp[j], ha);
    }
  }
  // ---- phase D: what follows from cur and the hops alone, eight lanes per step (slot q = lane & 7) ------------------
  // With k = #{hop <= cur} of the ascending hops, the live list of row cur is cur - hop[k - 1 - q] for q < k and cur
  // itself at q = k (ascending rows, as the mask walk of the lean kernel numbers them), every coefficient 1 but the
  // self entry's, the header {k + 1, k, cur, 0}; adjacency row cur gets 1 at the k sources and, with self, at cur.
  // (It needs kernel arguments alone; ahead of the first barrier it measured 0.4 us slower than here.)
#pragma unroll
  for (int o = 0; o < RUN_OCTS; ++o) {
    const int t = 8 * (wv + RUN_WAVES * o) + (lane >> 3);
    if (t < n) {
      const int q = lane & 7;
      const int cur = cur0 + t;
      int k = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) k += (int)(((hops4 >> (8 * i)) & 0xffu) <= (unsigned)cur);
      const int j = q < k ? cur - (int)((hops4 >> (8 * ((k - 1 - q) & 3))) & 0xffu) : cur;
      const bool is_cur = q == k;
      if (!FRESH && (q < k || (is_cur && self))) adj[(size_t)(g0 + (unsigned)cur) * N + j] = 1.f;
      if (rec) {
        float* saved = recd[o];
        if (q <= k) {
          (reinterpret_cast<int*>(saved + o_live) + gb * N)[q] = j;
          (saved + o_coef + gb * N)[q] = (is_cur && !self) ? 0.f : 1.f;
        }
        if (q == 7) {
          int* hdr = reinterpret_cast<int*>(saved + o_hdr) + 4 * gb;
          hdr[0] = k + 1; hdr[1] = k; hdr[2] = cur; hdr[3] = 0;
        }
      }
    }
  }
  if (threadIdx.x == 0) count[gb] = cur0 + n;   // (nothing can observe the values in between)
  const bool nonfinite = __any(bad);
  if (nonfinite && lane == 0) atomicOr(flags, GCM_FLAG_NONFINITE);
  if constexpr (FRESH) {
    if (GCM_RUN_FRESH_STORES_LATE) fresh_stores();
    // the further rounds of the image and the packed vector (a batch of fewer than 32 graphs)
    const size_t step = (size_t)gridDim.x * (64 * RUN_WAVES);
    for (size_t e = e_first + step; e < (size_t)IMG_LAYOUT_FLOATS; e += step)
      head_image_store(fr.image, (int)e, head_image_value(fr.hs, (int)e >> 12, ((int)e >> 6) & 63, (int)e & 63, F, H1, H2));
    for (size_t e = e_first + step; e < fr.hs.off[HEAD_MAX_SRCS]; e += step) fr.packed[e] = head_packed_value(fr.hs, (unsigned)e);
  }
}

// ---- the host side: one run object per chain --------------------------------------------------------------------
struct Run {
  // the remembered node: valid only while the stream's capture is `cid`
  hipGraphNode_t node = nullptr;
  unsigned long long cid = 0;
  hipStream_t stream = nullptr;
  int n = 0, cur0 = 0;
  // what a step must share with the node to continue it
  float *nodes = nullptr, *adj = nullptr, *cH = nullptr, *cA = nullptr, *cX = nullptr;
  int64_t* count = nullptr;
  const float *params = nullptr, *image = nullptr;
  uint32_t* flags = nullptr;
  int B = 0, N = 0, H2 = 0, self = 0, rec = 0;
  unsigned hops4 = 0xffffffffu;
  RunTable tab;
  int cap = RUN_CAP;
  // counters of the capture seen last
  unsigned long long stat_cid = 0;
  int stat_nodes = 0, stat_merged = 0, stat_absorbed = 0;
  // the head launch seen last under a capture (gcm_dense_rows_head_fused_run): looked at only while the stream's capture
  // is head.cid.  fresh: the remembered node has absorbed it and runs the fresh-state form with `fr`
  struct Head {
    hipGraphNode_t node = nullptr;
    unsigned long long cid = 0;
    hipStream_t stream = nullptr;
    HeadSrcs hs{};
    float *packed = nullptr, *image = nullptr;
    void* zero = nullptr;
    size_t zero_bytes = 0;
    int H2 = 0;
  } head;
  bool absorb = true, fresh = false;
  FreshArgs fr{};
  bool mfma = true;   // the node's layers run on the matrix cores (gcm_hip_run_mfma.h); false: the VALU form
};

// a graph call failed once: every later step of the process is a launch of its own
static std::atomic<bool> g_merge_ok{true};
static std::atomic<int> g_route{0}, g_last_error{0};   // 1: node edited in place, 2: node replaced; the last graph error

static void merge_off(hipError_t e) {
  g_last_error = (int)e;
  g_merge_ok = false;
  (void)hipGetLastError();
}
// a graph call of the head's absorption was refused once: heads stay launches of their own (merging itself goes on)
static std::atomic<bool> g_absorb_ok{true};
static void absorb_off(hipError_t e) {
  g_last_error = (int)e;
  g_absorb_ok = false;
  (void)hipGetLastError();
}

// n steps of R (tab filled up to n) as the parameters of a kernel node
struct RunArgs {
  int cur0, n, rec;
  unsigned hops4, nhs, o_v, o_hdr, o_coef, o_live;
  NoFresh none;
  void* ptr[20];
  hipKernelNodeParams p;
};
static void fill_args(Run& R, int n, RunArgs& a) {
  const CachedLayout lay = make_cached_layout(R.B, R.N, 32, R.H2);
  a.cur0 = R.cur0;
  a.n = n;
  a.rec = R.rec;
  a.hops4 = R.hops4;
  a.nhs = (unsigned)R.N | (unsigned)R.H2 << 8 | (R.self ? 1u << 16 : 0u);
  a.o_v = (unsigned)lay.o_v; a.o_hdr = (unsigned)lay.o_hdr; a.o_coef = (unsigned)lay.o_coef; a.o_live = (unsigned)lay.o_live;
  void* ptr[20] = {&R.image, &R.nodes, &R.cH, &R.params, &a.cur0, &a.n, &a.hops4, &a.nhs, &R.adj, &R.count,
                   &R.cA,    &R.cX,    &R.flags, &a.o_v, &a.o_hdr, &a.o_coef, &a.o_live, &a.rec, &R.tab,
                   R.fresh ? (void*)&R.fr : (void*)&a.none};
  for (int i = 0; i < 20; ++i) a.ptr[i] = ptr[i];
  a.p = hipKernelNodeParams{};
  a.p.func = R.fresh ? (R.mfma ? (void*)k_step_rows_cached_img4_lean_run<true, true> : (void*)k_step_rows_cached_img4_lean_run<true, false>)
                     : (R.mfma ? (void*)k_step_rows_cached_img4_lean_run<false, true> : (void*)k_step_rows_cached_img4_lean_run<false, false>);
  a.p.gridDim = dim3(R.B);
  a.p.blockDim = dim3(64 * RUN_WAVES);
  a.p.sharedMemBytes = 0;
  a.p.kernelParams = a.ptr;
  a.p.extra = nullptr;
}

// The remembered node now runs n steps.  First by editing it in place (hipGraphKernelNodeSetParams); if the runtime
// refuses that, by a new node on the old one's dependencies that takes its place as the stream's pending dependency.
// ROCm 7.2 accepts the edit of a node under capture while function and block size stay as they are, and refuses it with
// hipErrorLaunchFailure (719) when the node goes from the lean kernel's 128 threads to this kernel's 512: the second
// route is the one that runs there, and once it has, it is taken straight away.  The old node is replaced only while
// nothing depends on it (a fork recorded behind step t on another stream would): else the step starts a new run.
// false: nothing changed; the step is then a launch of its own (and after a failed graph call merging is off)
inline int64_t pad64(int64_t v) { return (v + 63) & ~int64_t(63); }

// The head absorbed.  The first append of a run replaces the lean node by the multi-step node anyway; if
// that lean node is step 0 of a rollout whose head launch (k_head_fused, remembered by gcm_dense_rows_head_fused_run)
// sits directly in front of it - the lean node's only dependency is the head's node and the head's only dependent is
// the lean node - no captured work can observe the head's outputs before the steps have run, and the new node does the
// head's work itself (the kernel's FRESH form): it is added on the HEAD's dependencies, and both old nodes go.
// -> 1: absorbed, R.node is the new node of n steps; 0: not absorbed and nothing changed (a refused graph call also
// turns absorption off for the process); *broken set: the head's node could neither be destroyed nor ordered in front
// of the new node - the graph must not be used, the entry returns the error.
static int absorb_head(Run& R, int n, hipGraph_t graph, hipError_t* broken) {
  const Run::Head& H = R.head;
  if (!R.absorb || !g_absorb_ok.load() || R.fresh || R.cur0 != 0 || !H.node || H.cid != R.cid || H.stream != R.stream)
    return 0;
  const int64_t n_nodes = pad64((int64_t)R.B * R.N * 32), n_adj = pad64((int64_t)R.B * R.N * R.N);
  const auto aligned16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (H.packed != R.params || H.image != R.image || H.H2 != R.H2 || R.N % 4 != 0 || H.zero != (void*)R.nodes ||
      H.zero_bytes != sizeof(float) * (size_t)(n_nodes + n_adj + 2 * (int64_t)R.B) || R.adj != R.nodes + n_nodes ||
      reinterpret_cast<float*>(R.count) != R.nodes + n_nodes + n_adj || !aligned16(H.hs.p[0]) || !aligned16(H.hs.p[1]) ||
      !aligned16(H.hs.p[3]) || !aligned16(H.hs.p[4]))
    return 0;
  size_t nd = 0, n_dep = 0, nh = 0;
  hipGraphNode_t one = nullptr, hdeps[8];
  hipError_t e = hipGraphNodeGetDependentNodes(R.node, nullptr, &n_dep);
  if (e == hipSuccess && n_dep) return 0;
  if (e == hipSuccess) e = hipGraphNodeGetDependencies(R.node, nullptr, &nd);
  if (e == hipSuccess && nd != 1) return 0;
  if (e == hipSuccess) e = hipGraphNodeGetDependencies(R.node, &one, &nd);
  if (e == hipSuccess && (nd != 1 || one != H.node)) return 0;
  if (e == hipSuccess) e = hipGraphNodeGetDependentNodes(H.node, nullptr, &n_dep);
  if (e == hipSuccess && n_dep != 1) return 0;
  if (e == hipSuccess) e = hipGraphNodeGetDependentNodes(H.node, &one, &n_dep);
  if (e == hipSuccess && (n_dep != 1 || one != R.node)) return 0;
  if (e == hipSuccess) e = hipGraphNodeGetDependencies(H.node, nullptr, &nh);
  if (e == hipSuccess && nh > 8) return 0;
  if (e == hipSuccess && nh) e = hipGraphNodeGetDependencies(H.node, hdeps, &nh);
  if (e != hipSuccess) {
    absorb_off(e);
    return 0;
  }
  R.fr = FreshArgs{};
  R.fr.hs = H.hs;
  R.fr.packed = H.packed;
  R.fr.image = H.image;
  R.fr.pad0 = (unsigned)((int64_t)R.B * R.N * 32);
  R.fr.pad0_end = (unsigned)n_nodes;
  R.fr.pad1 = (unsigned)(n_nodes + (int64_t)R.B * R.N * R.N);
  R.fr.pad1_end = (unsigned)(n_nodes + n_adj);
  R.fresh = true;
  RunArgs a;
  fill_args(R, n, a);
  hipGraphNode_t fresh = nullptr;
  e = hipGraphAddKernelNode(&fresh, graph, nh ? hdeps : nullptr, nh, &a.p);
  if (e != hipSuccess) {
    R.fresh = false;
    absorb_off(e);
    return 0;
  }
  e = hipStreamUpdateCaptureDependencies(R.stream, &fresh, 1, hipStreamSetCaptureDependencies);
  if (e == hipSuccess) {
    e = hipGraphDestroyNode(R.node);
    if (e != hipSuccess) {   // put the stream back on the lean node
      hipGraphNode_t old = R.node;
      (void)hipStreamUpdateCaptureDependencies(R.stream, &old, 1, hipStreamSetCaptureDependencies);
    }
  }
  if (e != hipSuccess) {   // nothing is gone yet: the ordinary replacement follows
    (void)hipGraphDestroyNode(fresh);
    R.fresh = false;
    absorb_off(e);
    return 0;
  }
  R.node = fresh;
  g_route = 2;
  e = hipGraphDestroyNode(H.node);
  if (e != hipSuccess) {
    // The lean node is gone and the head is not.  Ordered in front of the new node the head is harmless - the fresh
    // form rewrites every byte it wrote with the same values - but side by side they would race: order it, or give up.
    absorb_off(e);
    hipGraphNode_t from = H.node;
    const hipError_t e2 = hipGraphAddDependencies(graph, &from, &fresh, 1);
    if (e2 != hipSuccess) {
      (void)hipGetLastError();
      *broken = e;
      R.node = nullptr;
      R.head.node = nullptr;
      return 0;
    }
  } else {
    ++R.stat_absorbed;
  }
  R.head.node = nullptr;
  return 1;
}

static bool grow_node(Run& R, int n, hipGraph_t graph, hipError_t* broken) {
  if (R.n == 1 && n == 2) {
    const int ab = absorb_head(R, n, graph, broken);
    if (ab || *broken != hipSuccess) return ab == 1;
  }
  RunArgs a;
  fill_args(R, n, a);
  if (g_route.load() != 2) {
    const hipError_t e = hipGraphKernelNodeSetParams(R.node, &a.p);
    if (e == hipSuccess) {
      g_route = 1;
      return true;
    }
    g_last_error = (int)e;
    (void)hipGetLastError();
    if (g_route.load() == 1) {   // (it worked before: not a question of the route)
      merge_off(e);
      return false;
    }
  }
  size_t nd = 0, n_dependent = 0;
  hipError_t e = hipGraphNodeGetDependentNodes(R.node, nullptr, &n_dependent);
  if (e == hipSuccess && n_dependent) return false;
  if (e == hipSuccess) e = hipGraphNodeGetDependencies(R.node, nullptr, &nd);
  hipGraphNode_t deps[8];
  if (e == hipSuccess && nd > 8) e = hipErrorInvalidValue;
  if (e == hipSuccess && nd) e = hipGraphNodeGetDependencies(R.node, deps, &nd);
  hipGraphNode_t fresh = nullptr;
  if (e == hipSuccess) e = hipGraphAddKernelNode(&fresh, graph, nd ? deps : nullptr, nd, &a.p);
  if (e != hipSuccess) {
    merge_off(e);
    return false;
  }
  e = hipStreamUpdateCaptureDependencies(R.stream, &fresh, 1, hipStreamSetCaptureDependencies);
  if (e != hipSuccess) {
    (void)hipGraphDestroyNode(fresh);
    merge_off(e);
    return false;
  }
  e = hipGraphDestroyNode(R.node);
  if (e != hipSuccess) {   // put the stream back on the old node
    hipGraphNode_t old = R.node;
    (void)hipStreamUpdateCaptureDependencies(R.stream, &old, 1, hipStreamSetCaptureDependencies);
    (void)hipGraphDestroyNode(fresh);
    merge_off(e);
    return false;
  }
  R.node = fresh;
  g_route = 2;
  return true;
}

// [p, p + floats) and [q, q + floats2) share an address
static bool overlap(const float* p, size_t floats, const float* q, size_t floats2) {
  return p < q + floats2 && q < p + floats;
}

// Inside one launch the steps are not ordered against one another (each wave makes every eighth pair of steps, the
// observations are all read up front), so a step may join a run only if it shares no memory with the run's earlier
// steps in a way the order of the per-step launches would have resolved: its record must not lie on an earlier step's
// record (the later write must win) or observation (read before it is overwritten), and its observation must not lie
// on an earlier step's record (a belief fed back as the next observation).  The caching allocator hands a block freed
// during a capture out again without a node of its own, so this does happen: records of a no_grad loop that keeps
// only its last belief alternate between two addresses.
static bool shares_memory(const Run& R, const float* obs, const float* saved, size_t obs_floats, size_t rec_floats) {
  for (int t = 0; t < R.n; ++t)
    if (overlap(saved, rec_floats, R.tab.rec[t], rec_floats) || overlap(saved, rec_floats, R.tab.obs[t], obs_floats) ||
        overlap(obs, obs_floats, R.tab.rec[t], rec_floats))
      return true;
  return false;
}

}  // namespace gcm_rows

extern "C" int gcm_rows_run_steps_cap(void) { return gcm_rows::RUN_CAP; }
extern "C" void* gcm_rows_run_create(void) { return new (std::nothrow) gcm_rows::Run(); }
extern "C" int gcm_rows_run_destroy(void* run) {
  delete static_cast<gcm_rows::Run*>(run);
  return GCM_OK;
}
extern "C" int gcm_rows_run_reset(void* run) {
  GCM_REQUIRE(run);
  static_cast<gcm_rows::Run*>(run)->node = nullptr;
  static_cast<gcm_rows::Run*>(run)->fresh = false;
  return GCM_OK;
}
extern "C" int gcm_rows_run_set_cap(void* run, int cap) {
  GCM_REQUIRE(run && cap >= 1 && cap <= gcm_rows::RUN_CAP);
  static_cast<gcm_rows::Run*>(run)->cap = cap;
  return GCM_OK;
}
extern "C" int gcm_rows_run_stats(const void* run, int* out2) {
  GCM_REQUIRE(run && out2);
  const gcm_rows::Run* R = static_cast<const gcm_rows::Run*>(run);
  out2[0] = R->stat_nodes;
  out2[1] = R->stat_merged;
  return GCM_OK;
}
extern "C" int gcm_rows_run_enabled(void) { return gcm_rows::g_merge_ok.load() ? 1 : 0; }
extern "C" int gcm_rows_run_route(int* out2) {
  GCM_REQUIRE(out2);
  out2[0] = gcm_rows::g_route.load();
  out2[1] = gcm_rows::g_last_error.load();
  return GCM_OK;
}

extern "C" int gcm_dense_rows_step_cached_run(void* run, const float* obs, float* nodes, float* adj, int64_t* count,
                                              const gcm_selector_desc* selectors, int n_selectors, const float* params,
                                              const float* weight_image, int has_bias, int act1, int act2,
                                              float* cache_h1, float* cache_agg1, float* cache_nodes, float* saved,
                                              int record, int cur_host, uint32_t* flags, void* workspace,
                                              size_t workspace_bytes, int B, int N, int F, int H1, int H2,
                                              gcm_stream_t stream) {
  using namespace gcm_rows;
  auto plain = [&]() {
    return gcm_dense_rows_step_cached_ws(obs, nodes, adj, count, selectors, n_selectors, params, weight_image, has_bias,
                                         act1, act2, cache_h1, cache_agg1, cache_nodes, saved, record, cur_host, flags,
                                         workspace, workspace_bytes, B, N, F, H1, H2, stream);
  };
  Run* R = static_cast<Run*>(run);
  if (!R || !g_merge_ok.load()) return plain();
  hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long cid = 0;
  hipGraph_t graph = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  hipError_t e = hipStreamGetCaptureInfo_v2(st, &cs, &cid, &graph, &deps, &nd);
  if (e != hipSuccess) {
    merge_off(e);
    return plain();
  }
  if (cs != hipStreamCaptureStatusActive) {   // eager: exactly today's path
    R->node = nullptr;
    R->head.node = nullptr;
    R->fresh = false;
    R->stat_cid = 0;
    R->stat_nodes = R->stat_merged = R->stat_absorbed = 0;
    return plain();
  }
  // the lean case, as gcm_dense_rows_step_cached_ws decides it
  GCM_REQUIRE(obs && nodes && adj && count && params && cache_h1 && cache_agg1 && cache_nodes && saved && flags);
  GCM_REQUIRE(B > 0 && (selectors || n_selectors == 0));
  LeanCase lc;
  CachedLayout lay = make_cached_layout(B, N, H1, H2);
  const bool lean = gcm_dense_rows_cached_supported_ws(selectors, n_selectors, has_bias, N, F, H1, H2) &&
                    (size_t)B * N * (size_t)(F > N ? F : N) < ((size_t)1 << 31) && lay.total < ((size_t)1 << 31) &&
                    lean_step_case(selectors, n_selectors, weight_image, has_bias, act1, act2, N, F, H1, H2, cur_host, lc);
  if (!lean) {
    R->node = nullptr;
    R->fresh = false;
    return plain();
  }
  const int self = lc.self;
  unsigned hops4 = 0xffffffffu;
  for (int a = 0; a < lc.nh; ++a) hops4 = (hops4 & ~(0xffu << (8 * a))) | (unsigned)lc.hops[a] << (8 * a);
  const size_t obs_floats = (size_t)B * F, rec_floats = record ? lay.total : (size_t)B * H2;
  // (an observation that is a view of the state or the caches this chain writes: a row an earlier step made)
  const size_t rows_floats = (size_t)B * N * 32;
  const bool obs_in_state = overlap(obs, obs_floats, nodes, rows_floats) || overlap(obs, obs_floats, cache_nodes, rows_floats) ||
                            overlap(obs, obs_floats, cache_h1, rows_floats) || overlap(obs, obs_floats, cache_agg1, rows_floats) ||
                            overlap(obs, obs_floats, adj, (size_t)B * N * N);
  if (R->stat_cid != cid) {
    R->stat_cid = cid;
    R->stat_nodes = R->stat_merged = R->stat_absorbed = 0;
  }
  // (a handle is looked at only while the stream's capture is the one it was made in)
  const bool follows = R->node && R->cid == cid && R->stream == st && nd == 1 && deps[0] == R->node &&
                       cur_host == R->cur0 + R->n && R->n < R->cap && R->n < RUN_CAP && R->nodes == nodes &&
                       R->adj == adj && R->count == count && R->cH == cache_h1 && R->cA == cache_agg1 &&
                       R->cX == cache_nodes && R->params == params && R->image == weight_image && R->flags == flags &&
                       R->B == B && R->N == N && R->H2 == H2 && R->self == self && R->hops4 == hops4 &&
                       R->rec == (record ? 1 : 0) && !obs_in_state &&
                       !shares_memory(*R, obs, saved, obs_floats, rec_floats);
  if (follows) {
    R->tab.obs[R->n] = obs;
    R->tab.rec[R->n] = saved;
    hipError_t broken = hipSuccess;
    if (grow_node(*R, R->n + 1, graph, &broken)) {
      ++R->n;
      ++R->stat_merged;
      return GCM_OK;
    }
    if (broken != hipSuccess) return (int)broken;   // (the graph is half-edited: the capture must fail)
  }
  // a new run: the lean kernel, captured as gcm_dense_rows_step_cached_ws captures it, and its node remembered
  R->node = nullptr;
  R->fresh = false;
  if (!record) lay.total = 0;
  const int rc = launch_step_cached_lean(obs, nodes, adj, count, lc.m0, lc.m1, self, params, weight_image, cache_h1,
                                         cache_agg1, cache_nodes, saved, lay, flags, B, N, H2, cur_host, st);
  if (rc == GCM_EUNSUPPORTED) return plain();
  if (rc) return rc;
  ++R->stat_nodes;
  if (!g_merge_ok.load()) return GCM_OK;
  unsigned long long cid2 = 0;
  e = hipStreamGetCaptureInfo_v2(st, &cs, &cid2, &graph, &deps, &nd);
  if (e != hipSuccess) {
    merge_off(e);
    return GCM_OK;
  }
  if (cs != hipStreamCaptureStatusActive || cid2 != cid || nd != 1) return GCM_OK;
  hipGraphNode_t node = deps[0];
  hipGraphNodeType type;
  hipKernelNodeParams got;
  if ((e = hipGraphNodeGetType(node, &type)) != hipSuccess ||
      (type == hipGraphNodeTypeKernel && (e = hipGraphKernelNodeGetParams(node, &got)) != hipSuccess)) {
    merge_off(e);
    return GCM_OK;
  }
  if (type != hipGraphNodeTypeKernel || got.func != lean_step_kernel()) return GCM_OK;
  R->node = node;
  R->cid = cid;
  R->stream = st;
  R->n = 1;
  R->cur0 = cur_host;
  R->nodes = nodes; R->adj = adj; R->count = count; R->cH = cache_h1; R->cA = cache_agg1; R->cX = cache_nodes;
  R->params = params; R->image = weight_image; R->flags = flags;
  R->B = B; R->N = N; R->H2 = H2; R->self = self; R->rec = record ? 1 : 0;
  R->hops4 = hops4;
  R->tab.obs[0] = obs;
  R->tab.rec[0] = saved;
  return GCM_OK;
}

extern "C" int gcm_rows_run_set_absorb(void* run, int on) {
  GCM_REQUIRE(run);
  static_cast<gcm_rows::Run*>(run)->absorb = on != 0;
  return GCM_OK;
}
extern "C" int gcm_rows_run_absorbed(const void* run) {
  return run ? static_cast<const gcm_rows::Run*>(run)->stat_absorbed : 0;
}
// (the form is read whenever the node's parameters are made: set it before the capture, not inside a run)
extern "C" int gcm_rows_run_set_mfma(void* run, int on) {
  GCM_REQUIRE(run);
  static_cast<gcm_rows::Run*>(run)->mfma = on != 0;
  return GCM_OK;
}
extern "C" int gcm_rows_run_mfma(const void* run) { return run && static_cast<const gcm_rows::Run*>(run)->mfma ? 1 : 0; }
extern "C" int gcm_rows_run_absorb_enabled(void) { return gcm_rows::g_absorb_ok.load() ? 1 : 0; }

extern "C" int gcm_dense_rows_head_fused_run(void* run, const float* const* srcs_host, const size_t* lens_host, int n,
                                             float* packed, float* image, int F, int H1, int H2, void* zero,
                                             size_t zero_bytes, gcm_stream_t stream) {
  using namespace gcm_rows;
  const int rc = gcm_dense_rows_head_fused(srcs_host, lens_host, n, packed, image, F, H1, H2, zero, zero_bytes, stream);
  Run* R = static_cast<Run*>(run);
  if (!R) return rc;
  R->head.node = nullptr;
  if (rc != GCM_OK || !R->absorb || !g_absorb_ok.load() || !g_merge_ok.load() || !image || !zero || F != 32 || H1 != 32)
    return rc;
  hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long cid = 0;
  hipGraph_t graph = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0;
  hipError_t e = hipStreamGetCaptureInfo_v2(st, &cs, &cid, &graph, &deps, &nd);
  if (e != hipSuccess) {
    absorb_off(e);
    return rc;
  }
  if (cs != hipStreamCaptureStatusActive || nd != 1) return rc;
  hipGraphNode_t node = deps[0];
  hipGraphNodeType type;
  hipKernelNodeParams got;
  if ((e = hipGraphNodeGetType(node, &type)) != hipSuccess ||
      (type == hipGraphNodeTypeKernel && (e = hipGraphKernelNodeGetParams(node, &got)) != hipSuccess)) {
    absorb_off(e);
    return rc;
  }
  if (type != hipGraphNodeTypeKernel || got.func != head_fused_kernel()) return rc;
  size_t total = 0;
  if (!head_make_srcs(srcs_host, lens_host, n, R->head.hs, total)) return rc;
  R->head.node = node;
  R->head.cid = cid;
  R->head.stream = st;
  R->head.packed = packed;
  R->head.image = image;
  R->head.zero = zero;
  R->head.zero_bytes = zero_bytes;
  R->head.H2 = H2;
  return rc;
}

extern "C" int gcm_rows_capture_node_count(gcm_stream_t stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long cid = 0;
  hipGraph_t graph = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t nd = 0, nodes = 0;
  if (hipStreamGetCaptureInfo_v2((hipStream_t)stream, &cs, &cid, &graph, &deps, &nd) != hipSuccess ||
      cs != hipStreamCaptureStatusActive || hipGraphGetNodes(graph, nullptr, &nodes) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return (int)nodes;
}
