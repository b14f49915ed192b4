// Episode resets inside one SparseGCM call (SparseGCM.rollout(x, reset=mask)) - include/gcm_hip_segments.h.
// A graph with m valid resets becomes m + 1 virtual graphs ("segments") of one ordinary call; these kernels plan the
// segments, move x / the node matrices / the edge list into the segment layout and the call's results back out.
// Pure data movement.  Where an edge lands comes from counts and scans only (per 1024-entry chunk, then over the
// chunks), never from an atomic, so the output is bitwise reproducible; a graph's entries may span any number of
// chunks.  The mask, taus, the table and the batch row of a list are clamped on the device: every access stays in
// bounds whatever they hold.
#include "gcm_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = GCM_SPARSE_SEG_CHUNK;
static_assert(kChunk == 1024, "one entry per thread of a 1024-thread workgroup");

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int64_t shfl_up_i64(int64_t v, int d, int lane) {
  const int lo = __shfl_up((int)(v & 0xffffffffll), d), hi = __shfl_up((int)(v >> 32), d);
  const int64_t r = ((int64_t)hi << 32) | (uint32_t)lo;
  return lane >= d ? r : 0;
}

// exclusive prefix of c over the workgroup's 64 * WAVES threads (thread order), and the workgroup's total
template <int WAVES>
__device__ __forceinline__ int64_t block_exclusive(int64_t c, int64_t* s_wave, int64_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t incl = c;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) incl += shfl_up_i64(incl, d, lane);
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int64_t base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int64_t v = s_wave[w];
    if (w < wave) base += v;
    total += v;
  }
  return base + incl - c;
}

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
  return v;
}

// One 64-column tile of graph b's mask row: this lane's column s, whether it holds a valid reset, the wave's ballot of
// those, and the column of the nearest valid reset before s (`last` when the tile has none before it).
struct Tile {
  int s;
  bool flag;
  uint64_t bal;
  int prev, rank;
};
__device__ __forceinline__ Tile read_tile(const uint8_t* __restrict__ row, int c0, int tau, int last, int lane) {
  Tile r;
  r.s = c0 + lane;
  r.flag = r.s < tau && row[r.s] != 0;
  r.bal = __ballot(r.flag);
  const uint64_t lower = r.bal & ((1ull << lane) - 1ull);
  r.rank = __popcll(lower);
  r.prev = lower ? c0 + 63 - __clzll(lower) : last;
  return r;
}
__device__ __forceinline__ int last_of(uint64_t bal, int c0, int last) { return bal ? c0 + 63 - __clzll(bal) : last; }

// plan pass 1, one wave per graph: vbase[b] = m_b + 1 (scanned by pass 3), longest[b] = its longest segment,
// relabel[b] = -1 when column 0 holds a valid reset (the stored state goes), else 0
__global__ __launch_bounds__(64) void k_seg_count(const uint8_t* __restrict__ mask, const int64_t* __restrict__ taus,
                                                  int64_t* __restrict__ vbase, int64_t* __restrict__ longest,
                                                  int64_t* __restrict__ relabel, int t) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int tau = (int)clamp64(taus[b], 0, t);
  const uint8_t* __restrict__ row = mask + (size_t)b * t;
  int m = 0, last = 0, longest_here = 0;
  for (int c0 = 0; c0 < tau; c0 += 64) {      // (wave-uniform bounds)
    const Tile q = read_tile(row, c0, tau, last, lane);
    if (q.flag) longest_here = max(longest_here, q.s - q.prev);
    m += __popcll(q.bal);
    last = last_of(q.bal, c0, last);
  }
  longest_here = max(wave_max_i32(longest_here), tau - last);
  if (lane == 0) {
    vbase[b] = m + 1;
    longest[b] = longest_here;
    relabel[b] = (tau > 0 && row[0] != 0) ? -1 : 0;
  }
}

// survivors per chunk of a list under `relabel` (sign only)
__device__ __forceinline__ bool kept(const int64_t* __restrict__ idx, const int64_t* __restrict__ relabel, int64_t e,
                                     int64_t E, int B_old, int64_t& nb) {
  const int64_t bat = e < E ? clamp64(idx[e], 0, B_old - 1) : 0;
  nb = relabel[bat];
  return e < E && nb >= 0;
}

__global__ __launch_bounds__(kChunk) void k_edges_count(const int64_t* __restrict__ idx,
                                                        const int64_t* __restrict__ relabel,
                                                        int64_t* __restrict__ chunk, int64_t E, int B_old) {
  __shared__ int64_t s_wave[kChunk / 64];
  const int64_t e = (int64_t)blockIdx.x * kChunk + threadIdx.x;
  int64_t nb;
  const bool keep = kept(idx, relabel, e, E, B_old, nb);
  int64_t total;
  block_exclusive<kChunk / 64>(keep ? 1 : 0, s_wave, total);
  if (threadIdx.x == 0) chunk[blockIdx.x] = total;
}

// counts a[0..n) -> their exclusive prefix in place, a[n] = total (one workgroup; a thread rewrites only the range it
// read); -> the total
__device__ __forceinline__ int64_t scan_in_place(int64_t* __restrict__ a, int64_t n, int64_t* s_wave) {
  const int64_t per = (n + kThreads - 1) / kThreads;
  const int64_t first = (int64_t)threadIdx.x * per;
  const int64_t lo = first < n ? first : n, hi = lo + per < n ? lo + per : n;
  int64_t sum = 0;
  for (int64_t c = lo; c < hi; ++c) sum += a[c];
  int64_t total;
  int64_t run = block_exclusive<kThreads / 64>(sum, s_wave, total);
  for (int64_t c = lo; c < hi; ++c) {
    const int64_t v = a[c];
    a[c] = run;
    run += v;
  }
  if (threadIdx.x == 0) a[n] = total;
  return total;
}

// plan pass 3 (one workgroup): vbase and the chunk counts become exclusive prefixes, relabel[b] = vbase[b] where the
// stored state stays, and the totals
__global__ __launch_bounds__(kThreads) void k_seg_scan(int64_t* __restrict__ vbase, const int64_t* __restrict__ longest,
                                                       int64_t* __restrict__ relabel, int64_t* __restrict__ chunk,
                                                       int64_t nb, int64_t* __restrict__ totals, int B) {
  __shared__ int64_t s_a[kThreads / 64], s_b[kThreads / 64];
  __shared__ int s_max[kThreads / 64];
  const int64_t Bp = scan_in_place(vbase, B, s_a);
  const int64_t kept_edges = scan_in_place(chunk, nb, s_b);
  int longest_here = 1;
  for (int b = threadIdx.x; b < B; b += kThreads) longest_here = max(longest_here, (int)longest[b]);
  longest_here = wave_max_i32(longest_here);
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = longest_here;
  __syncthreads();      // (also: every vbase[b] of pass 3 is written)
  for (int b = threadIdx.x; b < B; b += kThreads)
    if (relabel[b] >= 0) relabel[b] = vbase[b];
  if (threadIdx.x == 0) {
    int tp = 1;
    for (int w = 0; w < kThreads / 64; ++w) tp = max(tp, s_max[w]);
    totals[0] = Bp;
    totals[1] = tp;
    totals[2] = Bp - B;
    totals[3] = kept_edges;
  }
}

// standalone scan of the chunk counts (gcm_sparse_seg_edges_plan)
__global__ __launch_bounds__(kThreads) void k_edges_scan(int64_t* __restrict__ chunk, int64_t nb) {
  __shared__ int64_t s_a[kThreads / 64];
  scan_in_place(chunk, nb, s_a);
}

// plan pass 4, one wave per graph: the table rows of its segments
__global__ __launch_bounds__(64) void k_seg_table(const uint8_t* __restrict__ mask, const int64_t* __restrict__ taus,
                                                  const int64_t* __restrict__ T, const int64_t* __restrict__ vbase,
                                                  int64_t* __restrict__ table, int64_t cap, int t) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int tau = (int)clamp64(taus[b], 0, t);
  const uint8_t* __restrict__ row = mask + (size_t)b * t;
  const int64_t base = vbase[b];
  int64_t* __restrict__ owner = table + GCM_SPARSE_SEG_OWNER * cap;
  int64_t* __restrict__ start = table + GCM_SPARSE_SEG_START * cap;
  int64_t* __restrict__ len = table + GCM_SPARSE_SEG_LEN * cap;
  int64_t* __restrict__ empty = table + GCM_SPARSE_SEG_EMPTY * cap;
  int64_t* __restrict__ Tin = table + GCM_SPARSE_SEG_T * cap;
  int64_t* __restrict__ fin = table + GCM_SPARSE_SEG_FINAL * cap;
  int done = 0, last = 0;        // segments closed so far; first column of the open one
  for (int c0 = 0; c0 < tau; c0 += 64) {
    const Tile q = read_tile(row, c0, tau, last, lane);
    // a valid reset at s closes segment done + rank (which began at q.prev) and opens the next one
    const int64_t v = base + done + q.rank;
    if (q.flag && v >= 0 && v + 1 < cap) {
      len[v] = q.s - q.prev;
      fin[v] = -1;
      owner[v + 1] = b;
      start[v + 1] = q.s;
      empty[v + 1] = 1;
      Tin[v + 1] = 0;
    }
    done += __popcll(q.bal);
    last = last_of(q.bal, c0, last);
  }
  if (lane == 0 && base >= 0 && base + done < cap) {
    const bool drop = tau > 0 && row[0] != 0;
    owner[base] = b;
    start[base] = 0;
    empty[base] = drop ? 1 : 0;
    Tin[base] = drop ? 0 : T[b];
    len[base + done] = tau - last;
    fin[base + done] = b;
  }
}

__device__ __forceinline__ float vt_zero(float) { return 0.f; }
__device__ __forceinline__ float4 vt_zero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }

// rows between [B,t,F] and [Bp,tp,F]; one VT per thread; F counts VTs
template <bool BWD, typename VT>
__global__ __launch_bounds__(kThreads) void k_seg_rows(const VT* __restrict__ in, const int64_t* __restrict__ table,
                                                       int64_t cap, VT* __restrict__ out, int64_t total, int tp, int B,
                                                       int t, int F) {
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int64_t r = e / F;
  const int c = (int)(e - r * F);
  const int64_t v = r / tp;
  const int i = (int)(r - v * tp);
  const int64_t owner = clamp64(table[GCM_SPARSE_SEG_OWNER * cap + v], 0, B - 1);
  const int64_t start = clamp64(table[GCM_SPARSE_SEG_START * cap + v], 0, t);
  const int64_t len = clamp64(table[GCM_SPARSE_SEG_LEN * cap + v], 0, t - start);
  const bool live = i < len;
  const int64_t at = ((owner * t + start + i) * F) + c;
  if (BWD) {
    if (live) out[at] = in[e];
  } else {
    out[e] = live ? in[at] : vt_zero(VT());
  }
}

// node matrices between [B,N,F] and [Bp,N,F]: blockIdx.x = the graph written, blockIdx.y = its share of N * F
template <typename VT>
__global__ __launch_bounds__(kThreads) void k_seg_nodes(const VT* __restrict__ in, const int64_t* __restrict__ vbase,
                                                        const int64_t* __restrict__ table, int64_t cap,
                                                        VT* __restrict__ out, int Bp, int B, int NF, int final,
                                                        int to_segments) {
  const int64_t w = blockIdx.x;
  int64_t from;
  bool paired;
  if (to_segments) {
    const int64_t b = clamp64(table[GCM_SPARSE_SEG_OWNER * cap + w], 0, B - 1);
    paired = final ? w == vbase[b + 1] - 1 : (w == vbase[b] && table[GCM_SPARSE_SEG_EMPTY * cap + w] == 0);
    from = b;
  } else {
    from = clamp64(final ? vbase[w + 1] - 1 : vbase[w], 0, Bp - 1);
    paired = final ? true : table[GCM_SPARSE_SEG_EMPTY * cap + from] == 0;
  }
  const VT* __restrict__ s = in + (size_t)from * NF;
  VT* __restrict__ d = out + (size_t)w * NF;
  constexpr int U = 4;
  const int e0 = blockIdx.y * (U * kThreads) + threadIdx.x;
  VT v[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = e0 + u * kThreads;
    v[u] = (paired && i < NF) ? s[i] : vt_zero(VT());
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = e0 + u * kThreads;
    if (i < NF) d[i] = v[u];
  }
}

__global__ __launch_bounds__(kChunk) void k_edges_compact(const int64_t* __restrict__ idx,
                                                          const float* __restrict__ vals,
                                                          const int64_t* __restrict__ relabel,
                                                          const int64_t* __restrict__ chunk_off,
                                                          int64_t* __restrict__ out_idx, float* __restrict__ out_vals,
                                                          int64_t* __restrict__ src_pos, int64_t E, int64_t E_new,
                                                          int B_old, int B_new) {
  __shared__ int64_t s_wave[kChunk / 64];
  const int64_t e = (int64_t)blockIdx.x * kChunk + threadIdx.x;
  const int64_t base = chunk_off[blockIdx.x];
  int64_t nb;
  const bool keep = kept(idx, relabel, e, E, B_old, nb);
  const int64_t snk = e < E ? idx[E + e] : 0, src = e < E ? idx[2 * E + e] : 0;
  const float val = keep && vals ? vals[e] : 0.f;
  int64_t total;
  const int64_t pos = base + block_exclusive<kChunk / 64>(keep ? 1 : 0, s_wave, total);
  if (keep && pos >= 0 && pos < E_new) {
    out_idx[pos] = clamp64(nb, 0, B_new - 1);
    out_idx[E_new + pos] = snk;
    out_idx[2 * E_new + pos] = src;
    if (out_vals) out_vals[pos] = val;
    src_pos[pos] = e;
  }
}

__global__ __launch_bounds__(kThreads) void k_seg_final_T(const int64_t* __restrict__ T_seg,
                                                          const int64_t* __restrict__ vbase,
                                                          int64_t* __restrict__ T_out, int Bp, int B) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b < B) T_out[b] = T_seg[clamp64(vbase[b + 1] - 1, 0, Bp - 1)];
}

inline bool aligned16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }
inline int64_t chunks_of(int64_t E) { return (E + kChunk - 1) / kChunk; }

}  // namespace

extern "C" int gcm_sparse_seg_plan(const uint8_t* mask, const int64_t* taus, const int64_t* T, const int64_t* idx,
                                   int64_t* vbase, int64_t* table, int64_t cap, int64_t* relabel, int64_t* chunk_off,
                                   int64_t* totals, int64_t E, int B, int t, gcm_stream_t stream) {
  GCM_REQUIRE(mask && taus && T && vbase && table && relabel && chunk_off && totals && (idx || E == 0));
  GCM_REQUIRE(E >= 0 && B > 0 && t > 0 && cap >= (int64_t)B * ((int64_t)t + 1));
  const int64_t nb = chunks_of(E);
  if (nb > 0x7fffffffll || cap > 0x7fffffffll) return GCM_EUNSUPPORTED;
  const hipStream_t st = (hipStream_t)stream;
  // (the longest segment of every graph rests in the table's LEN row, which has at least B entries, between pass 1
  //  and pass 3; pass 4 then writes the row)
  int64_t* longest = table + GCM_SPARSE_SEG_LEN * cap;
  hipLaunchKernelGGL(k_seg_count, dim3(B), dim3(64), 0, st, mask, taus, vbase, longest, relabel, t);
  if (nb > 0) hipLaunchKernelGGL(k_edges_count, dim3((unsigned)nb), dim3(kChunk), 0, st, idx, relabel, chunk_off, E, B);
  hipLaunchKernelGGL(k_seg_scan, dim3(1), dim3(kThreads), 0, st, vbase, longest, relabel, chunk_off, nb, totals, B);
  hipLaunchKernelGGL(k_seg_table, dim3(B), dim3(64), 0, st, mask, taus, T, vbase, table, cap, t);
  return gcm_launch_status();
}

extern "C" int gcm_sparse_seg_rows(const float* in, const int64_t* table, int64_t cap, float* out, int Bp, int tp,
                                   int B, int t, int F, int backward, gcm_stream_t stream) {
  GCM_REQUIRE(in && table && out && in != out);
  GCM_REQUIRE(Bp > 0 && tp > 0 && B > 0 && t > 0 && F > 0 && cap >= Bp);
  const hipStream_t st = (hipStream_t)stream;
  if (backward && hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * t * F, st) != hipSuccess) return GCM_EINVAL;
  const bool vec = F % 4 == 0 && aligned16(in, out);
  const int FV = vec ? F / 4 : F;
  const int64_t total = (int64_t)Bp * tp * FV;
  const int64_t blocks = (total + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffll) return GCM_EUNSUPPORTED;
  const dim3 grid((unsigned)blocks), block(kThreads);
  if (vec) {
    const float4* s = (const float4*)in;
    float4* d = (float4*)out;
    if (backward) hipLaunchKernelGGL((k_seg_rows<true, float4>), grid, block, 0, st, s, table, cap, d, total, tp, B, t, FV);
    else hipLaunchKernelGGL((k_seg_rows<false, float4>), grid, block, 0, st, s, table, cap, d, total, tp, B, t, FV);
  } else {
    if (backward) hipLaunchKernelGGL((k_seg_rows<true, float>), grid, block, 0, st, in, table, cap, out, total, tp, B, t, FV);
    else hipLaunchKernelGGL((k_seg_rows<false, float>), grid, block, 0, st, in, table, cap, out, total, tp, B, t, FV);
  }
  return gcm_launch_status();
}

extern "C" int gcm_sparse_seg_nodes(const float* in, const int64_t* vbase, const int64_t* table, int64_t cap,
                                    float* out, int Bp, int B, int N, int F, int final, int to_segments,
                                    gcm_stream_t stream) {
  GCM_REQUIRE(in && vbase && table && out && in != out);
  GCM_REQUIRE(Bp > 0 && B > 0 && N > 0 && F > 0 && cap >= Bp);
  if ((int64_t)N * F > 0x7fffffffll) return GCM_EUNSUPPORTED;
  const bool vec = F % 4 == 0 && aligned16(in, out);
  const int NF = vec ? N * (F / 4) : N * F;
  const int per = 4 * kThreads;
  const int shares = (NF + per - 1) / per;
  if (shares > 65535) return GCM_EUNSUPPORTED;
  const dim3 grid(to_segments ? Bp : B, shares), block(kThreads);
  const hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL((k_seg_nodes<float4>), grid, block, 0, st, (const float4*)in, vbase, table, cap, (float4*)out, Bp,
                       B, NF, final, to_segments);
  else
    hipLaunchKernelGGL((k_seg_nodes<float>), grid, block, 0, st, in, vbase, table, cap, out, Bp, B, NF, final,
                       to_segments);
  return gcm_launch_status();
}

extern "C" int gcm_sparse_seg_edges_plan(const int64_t* idx, const int64_t* relabel, int64_t* chunk_off, int64_t E,
                                         int B_old, gcm_stream_t stream) {
  GCM_REQUIRE(relabel && chunk_off && (idx || E == 0));
  GCM_REQUIRE(E >= 0 && B_old > 0);
  const int64_t nb = chunks_of(E);
  if (nb > 0x7fffffffll) return GCM_EUNSUPPORTED;
  const hipStream_t st = (hipStream_t)stream;
  if (nb > 0)
    hipLaunchKernelGGL(k_edges_count, dim3((unsigned)nb), dim3(kChunk), 0, st, idx, relabel, chunk_off, E, B_old);
  hipLaunchKernelGGL(k_edges_scan, dim3(1), dim3(kThreads), 0, st, chunk_off, nb);
  return gcm_launch_status();
}

extern "C" int gcm_sparse_seg_edges(const int64_t* idx, const float* vals, const int64_t* relabel,
                                    const int64_t* chunk_off, int64_t* out_idx, float* out_vals, int64_t* src_pos,
                                    int64_t E, int64_t E_new, int B_old, int B_new, gcm_stream_t stream) {
  GCM_REQUIRE(relabel && chunk_off && (idx || E == 0) && ((out_idx && src_pos) || E_new == 0));
  GCM_REQUIRE((vals != nullptr) == (out_vals != nullptr) || E_new == 0);
  GCM_REQUIRE(E >= 0 && E_new >= 0 && E_new <= E && B_old > 0 && B_new > 0);
  const int64_t nb = chunks_of(E);
  if (nb > 0x7fffffffll) return GCM_EUNSUPPORTED;
  if (E == 0 || E_new == 0) return GCM_OK;
  hipLaunchKernelGGL(k_edges_compact, dim3((unsigned)nb), dim3(kChunk), 0, (hipStream_t)stream, idx, vals, relabel,
                     chunk_off, out_idx, out_vals, src_pos, E, E_new, B_old, B_new);
  return gcm_launch_status();
}

extern "C" int gcm_sparse_seg_final_T(const int64_t* T_seg, const int64_t* vbase, int64_t* T_out, int Bp, int B,
                                      gcm_stream_t stream) {
  GCM_REQUIRE(T_seg && vbase && T_out && Bp > 0 && B > 0);
  hipLaunchKernelGGL(k_seg_final_T, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, T_seg,
                     vbase, T_out, Bp, B);
  return gcm_launch_status();
}
