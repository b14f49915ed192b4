// SparseGCM's sliding window: drop the oldest k_b nodes of every graph of a sparse hidden state
// (nodes [B,N,F], COO (batch, sink, source) sorted, T [B]) - include/gcm_hip_window.h.
// k_b = max(0, T_b + tau_b - N) is the wrap-around of a full graph, k_b = T_b an episode reset.
// Pure data movement: a row shift of the node matrix and an order-preserving compaction of the edge list.  Where a
// survivor lands comes from counts and scans only (per 1024-entry chunk, then over the chunks), never from an atomic,
// so the output is bitwise reproducible; a graph's entries may span any number of chunks.
// k and T are clamped on the device: every access stays in bounds whatever they hold.
#include "gcm_common.h"

namespace {

constexpr int kThreads = 256;
// the list kernels: a workgroup owns one chunk, one entry per thread - the rows are read fully coalesced, and sixteen
// waves per workgroup keep enough loads in flight to hide the chain batch -> k, T of that graph -> compare
constexpr int kChunk = GCM_SPARSE_DROP_CHUNK;
static_assert(kChunk == 1024, "one entry per thread of a 1024-thread workgroup");

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// nodes stored in graph b (t) and how many of them go (kc), both inside [0, N]
__device__ __forceinline__ void window_of(const int64_t* __restrict__ k, const int64_t* __restrict__ T, int64_t b, int N,
                                          int64_t& t, int64_t& kc) {
  t = clamp64(T[b], 0, N);
  kc = clamp64(k[b], 0, t);
}

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

// does entry e survive (source >= k of its graph); its batch (clamped into [0, B)) and that k
__device__ __forceinline__ bool survives(const int64_t* __restrict__ idx, const int64_t* __restrict__ k,
                                         const int64_t* __restrict__ T, int64_t e, int64_t E, int B, int N,
                                         int64_t& bat, int64_t& src, int64_t& kc) {
  bat = e < E ? idx[e] : 0;
  src = e < E ? idx[2 * E + e] : 0;
  int64_t t;
  window_of(k, T, clamp64(bat, 0, B - 1), N, t, kc);
  return e < E && src >= kc;
}

// pass 1: survivors per chunk
__global__ __launch_bounds__(kChunk) void k_drop_count(const int64_t* __restrict__ idx, const int64_t* __restrict__ k,
                                                       const int64_t* __restrict__ T, int64_t* __restrict__ chunk,
                                                       int64_t E, int B, int N) {
  __shared__ int64_t s_wave[kChunk / 64];
  const int64_t e = (int64_t)blockIdx.x * kChunk + threadIdx.x;
  int64_t bat, src, kc;
  const bool keep = survives(idx, k, T, e, E, B, N, bat, src, kc);
  int64_t total;
  block_exclusive<kChunk / 64>(keep ? 1 : 0, s_wave, total);
  if (threadIdx.x == 0) chunk[blockIdx.x] = total;
}

// pass 2 (one workgroup): the chunk counts become their exclusive prefix in place, chunk[nb] = E'; T' = T - k
__global__ __launch_bounds__(kThreads) void k_drop_scan(int64_t* __restrict__ chunk, int64_t nb,
                                                        const int64_t* __restrict__ k, const int64_t* __restrict__ T,
                                                        int64_t* __restrict__ T_out, int B, int N) {
  __shared__ int64_t s_wave[kThreads / 64];
  for (int b = threadIdx.x; b < B; b += kThreads) {
    int64_t t, kc;
    window_of(k, T, b, N, t, kc);
    T_out[b] = T[b] - kc;
  }
  const int64_t per = (nb + kThreads - 1) / kThreads;
  const int64_t first = (int64_t)threadIdx.x * per;
  const int64_t lo = first < nb ? first : nb, hi = lo + per < nb ? lo + per : nb;
  int64_t sum = 0;
  for (int64_t c = lo; c < hi; ++c) sum += chunk[c];
  int64_t total;
  int64_t run = block_exclusive<kThreads / 64>(sum, s_wave, total);
  for (int64_t c = lo; c < hi; ++c) {       // (a thread rewrites only the range it read)
    const int64_t n = chunk[c];
    chunk[c] = run;
    run += n;
  }
  if (threadIdx.x == 0) chunk[nb] = total;
}

// pass 3: survivors to their places, indices moved by their graph's k; and the new per-graph pointer - the survivors
// ahead of the first entry of every graph (an entry whose batch differs from its predecessor's writes the pointer of
// its graph and of the empty graphs before it; the last entry writes the tail)
__global__ __launch_bounds__(kChunk) void k_drop_compact(
    const int64_t* __restrict__ idx, const float* __restrict__ vals, const int64_t* __restrict__ k,
    const int64_t* __restrict__ T, const int64_t* __restrict__ chunk_off, int64_t* __restrict__ out_idx,
    float* __restrict__ out_vals, int64_t* __restrict__ src_pos, int64_t* __restrict__ bptr, int64_t E, int64_t E_new,
    int B, int N) {
  __shared__ int64_t s_wave[kChunk / 64];
  const int64_t e = (int64_t)blockIdx.x * kChunk + threadIdx.x;
  const int64_t base = chunk_off[blockIdx.x];
  int64_t bat, src, kc;
  const bool keep = survives(idx, k, T, e, E, B, N, bat, src, kc);
  const int64_t snk = e < E ? idx[E + e] : 0;
  const int64_t prev = e > 0 && e < E ? clamp64(idx[e - 1], 0, B - 1) : -1;
  const float val = keep && vals ? vals[e] : 0.f;
  int64_t total;
  const int64_t pos = base + block_exclusive<kChunk / 64>(keep ? 1 : 0, s_wave, total);
  if (keep && pos >= 0 && pos < E_new) {
    out_idx[pos] = bat;
    out_idx[E_new + pos] = snk - kc;
    out_idx[2 * E_new + pos] = src - kc;
    if (out_vals) out_vals[pos] = val;
    src_pos[pos] = e;
  }
  if (e < E) {
    const int64_t b1 = clamp64(bat, 0, B - 1);
    for (int64_t b = prev + 1; b <= b1; ++b) bptr[b] = pos;
    if (e == E - 1)
      for (int64_t b = b1 + 1; b <= B; ++b) bptr[b] = pos + (keep ? 1 : 0);
  }
}

// the node matrix moved up by k rows (forward), or the gradient moved back down (BWD); rows outside are zero.
// VT = float4: rows of F / 4 vectors, 16 bytes per lane; F counts VTs.
__device__ __forceinline__ float vt_zero(float) { return 0.f; }
__device__ __forceinline__ float4 vt_zero(float4) { return make_float4(0.f, 0.f, 0.f, 0.f); }

template <bool BWD, typename VT>
__global__ __launch_bounds__(kThreads) void k_drop_nodes(const VT* __restrict__ src, const int64_t* __restrict__ k,
                                                         const int64_t* __restrict__ T, VT* __restrict__ dst, int N,
                                                         int F, int rows_per_block) {
  // a graph's rows are contiguous, so the shift is one contiguous move by kc * F elements: element i of the graph
  // comes from i + kc * F (forward, live while that stays below t * F) or i - kc * F (backward, live for
  // kc * F <= i < t * F).  Four elements per thread, their loads issued before the first store.
  const int b = blockIdx.y;
  int64_t t, kc;
  window_of(k, T, b, N, t, kc);
  const int shift = (int)kc * F;
  const int lo = BWD ? shift : 0, hi = BWD ? (int)t * F : (int)(t - kc) * F;
  const int off = BWD ? -shift : shift;
  const int e0 = blockIdx.x * rows_per_block * F, e1 = min(N * F, e0 + rows_per_block * F);
  const VT* __restrict__ s = src + (size_t)b * N * F;
  VT* __restrict__ d = dst + (size_t)b * N * F;
  constexpr int U = 4;
  for (int e = e0 + threadIdx.x; e < e1; e += U * kThreads) {
    VT v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = e + u * kThreads;
      v[u] = (i < e1 && i >= lo && i < hi) ? s[i + off] : vt_zero(VT());
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = e + u * kThreads;
      if (i < e1) d[i] = v[u];
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_drop_values_bwd(const float* __restrict__ g_out,
                                                              const int64_t* __restrict__ src_pos,
                                                              float* __restrict__ g_in, int64_t E, int64_t E_new) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= E_new) return;
  const int64_t p = src_pos[i];
  if (p >= 0 && p < E) g_in[p] = g_out[i];
}

inline bool aligned16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }
inline int64_t chunks_of(int64_t E) { return (E + kChunk - 1) / kChunk; }

}  // namespace

extern "C" int gcm_sparse_drop_plan(const int64_t* idx, const int64_t* k, const int64_t* T, int64_t* T_out,
                                    int64_t* chunk_off, int64_t E, int B, int N, gcm_stream_t stream) {
  GCM_REQUIRE(k && T && T_out && chunk_off && (idx || E == 0));
  GCM_REQUIRE(E >= 0 && B > 0 && N > 0);
  const int64_t nb = chunks_of(E);
  if (nb > 0x7fffffffll) return GCM_EUNSUPPORTED;
  if (nb > 0)
    hipLaunchKernelGGL(k_drop_count, dim3((unsigned)nb), dim3(kChunk), 0, (hipStream_t)stream, idx, k, T, chunk_off,
                       E, B, N);
  hipLaunchKernelGGL(k_drop_scan, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, chunk_off, nb, k, T, T_out, B, N);
  return gcm_launch_status();
}

extern "C" int gcm_sparse_drop_nodes(const float* in, const int64_t* k, const int64_t* T, float* out, int B, int N,
                                     int F, int backward, gcm_stream_t stream) {
  GCM_REQUIRE(in && k && T && out && in != out);
  GCM_REQUIRE(B > 0 && N > 0 && F > 0);
  if (B > 65535 || (int64_t)N * F > 0x7fffffffll) return GCM_EUNSUPPORTED;
  const int rpb = 128;   // (F = 32: 1024 float4 per workgroup, four per thread)
  const dim3 grid((N + rpb - 1) / rpb, B), block(kThreads);
  const hipStream_t st = (hipStream_t)stream;
  if (F % 4 == 0 && aligned16(in, out)) {
    const float4* s = (const float4*)in;
    float4* d = (float4*)out;
    if (backward) hipLaunchKernelGGL((k_drop_nodes<true, float4>), grid, block, 0, st, s, k, T, d, N, F / 4, rpb);
    else hipLaunchKernelGGL((k_drop_nodes<false, float4>), grid, block, 0, st, s, k, T, d, N, F / 4, rpb);
  } else {
    if (backward) hipLaunchKernelGGL((k_drop_nodes<true, float>), grid, block, 0, st, in, k, T, out, N, F, rpb);
    else hipLaunchKernelGGL((k_drop_nodes<false, float>), grid, block, 0, st, in, k, T, out, N, F, rpb);
  }
  return gcm_launch_status();
}

extern "C" int gcm_sparse_drop_edges(const int64_t* idx, const float* vals, const int64_t* k, const int64_t* T,
                                     const int64_t* chunk_off, int64_t* out_idx, float* out_vals, int64_t* src_pos,
                                     int64_t* bptr, int64_t E, int64_t E_new, int B, int N, gcm_stream_t stream) {
  GCM_REQUIRE(k && T && chunk_off && bptr && (idx || E == 0) && ((out_idx && src_pos) || E_new == 0));
  GCM_REQUIRE((vals != nullptr) == (out_vals != nullptr) || E_new == 0);
  GCM_REQUIRE(E >= 0 && E_new >= 0 && E_new <= E && B > 0 && N > 0);
  const int64_t nb = chunks_of(E);
  if (nb > 0x7fffffffll) return GCM_EUNSUPPORTED;
  if (E == 0)   // no entry to write the pointer from
    return hipMemsetAsync(bptr, 0, sizeof(int64_t) * ((size_t)B + 1), (hipStream_t)stream) == hipSuccess ? GCM_OK
                                                                                                          : GCM_EINVAL;
  // (E_new == 0: nothing survives and nothing is stored, but the pointer is still written - all zeros)
  hipLaunchKernelGGL(k_drop_compact, dim3((unsigned)nb), dim3(kChunk), 0, (hipStream_t)stream, idx, vals, k, T,
                     chunk_off, out_idx, out_vals, src_pos, bptr, E, E_new, B, N);
  return gcm_launch_status();
}

extern "C" int gcm_sparse_drop_values_bwd(const float* g_out, const int64_t* src_pos, float* g_in, int64_t E,
                                          int64_t E_new, gcm_stream_t stream) {
  GCM_REQUIRE(E >= 0 && E_new >= 0 && (g_in || E == 0) && ((g_out && src_pos) || E_new == 0));
  if (E == 0) return GCM_OK;
  if (hipMemsetAsync(g_in, 0, sizeof(float) * (size_t)E, (hipStream_t)stream) != hipSuccess) return GCM_EINVAL;
  if (E_new > 0)
    hipLaunchKernelGGL(k_drop_values_bwd, dim3((unsigned)((E_new + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, g_out, src_pos, g_in, E, E_new);
  return gcm_launch_status();
}
