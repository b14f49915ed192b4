// The primitives under gcm.nn.MessagePassing (PyG's MessagePassing contract on GraphIndex) and gcm.graph_utils'
// softmax / scatter, on gfx950: rows gathered by an index, segments of rows reduced (sum, mean, max, min), the
// gradient of max / min routed to the winning row, and a softmax over the rows of a segment with its gradient.
//
//   gather      out[e,:]   = (scale ? scale[idx[e]] : 1) x[idx[e],:]
//   reduce      out[i,:]   = op over p in [ptr[i], ptr[i+1]) of src[row(p),:],   row(p) = perm ? perm[p] : p
//   select_bwd  g_src[e,c] = arg[dst[e],c] == e ? g_out[dst[e],c] : 0
//   softmax     out[row(p),c] = exp(src[row(p),c] - max_seg) / sum_seg over the segment that holds p
//
// Unlike the fused layers these materialise [E,C] rows, as PyG does; all of it is row traffic.  One layout serves every
// kernel: a wave holds 64 >> shift rows, 1 << shift lanes across the channels of each, and a lane strides over the
// row when it is wider than that - so a wave is full at C = 32 (8 lanes of 16 bytes a row, 8 rows) as at C = 1 (64
// rows) or C = 260 (one row, two strides).  VEC = 4: 16-byte accesses, taken when C % 4 == 0 and every row pointer is
// 16-byte aligned; VEC = 1 serves every other shape.  No width cap.  A segment is walked serially by the lanes of its
// row, four independent loads in flight, the terms combined in the segment's order: every sum has one order (no float
// atomics), two calls are bitwise equal, and the first entry of a segment wins a tie of max / min.  PERM = false
// (a list already in CSR order) pays no index load.  Indices are read with bounds: an entry outside [0, M) gathers 0,
// pointers and permutation entries are clamped into the list - a bad index cannot read outside the tensors, and
// every store goes to the thread's own row.  int64 element offsets throughout.
#include <climits>

#include "gcm_common.h"

namespace {

constexpr int TPB = 256;
constexpr int WPB = TPB / 64;
constexpr int UNROLL = 4;   // rows in flight per lane

// VEC consecutive channels of one row
template <int VEC>
struct Pack {
  float a[VEC];
  __device__ __forceinline__ static Pack load(const float* __restrict__ p) {
    Pack r;
    if constexpr (VEC == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p);
      r.a[0] = v.x, r.a[1] = v.y, r.a[2] = v.z, r.a[3] = v.w;
    } else {
      r.a[0] = *p;
    }
    return r;
  }
  __device__ __forceinline__ static Pack fill(float v) {
    Pack r;
#pragma unroll
    for (int k = 0; k < VEC; ++k) r.a[k] = v;
    return r;
  }
  __device__ __forceinline__ void store(float* __restrict__ p) const {
    if constexpr (VEC == 4) {
      *reinterpret_cast<f32x4*>(p) = f32x4{a[0], a[1], a[2], a[3]};
    } else {
      *p = a[0];
    }
  }
};

// the lanes of a wave over rows and channels: row `sub` of the wave's 64 >> shift, channel packs c0, c0 + lpr, ...
struct Lanes {
  int sub, c0, lpr, rpw;
  int64_t wave;
  __device__ __forceinline__ explicit Lanes(int shift) {
    const int lane = threadIdx.x & 63;
    lpr = 1 << shift;
    rpw = 64 >> shift;
    sub = lane >> shift;
    c0 = lane & (lpr - 1);
    wave = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6);
  }
};

__device__ __forceinline__ int64_t clamp_to(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// row of src behind position p of a segment
template <bool PERM>
__device__ __forceinline__ int64_t row_at(const int64_t* __restrict__ perm, int64_t p, int64_t E) {
  if constexpr (PERM) return clamp_to(perm[p], E - 1);
  return p;
}

// ---------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------
template <int VEC, bool SCALE>
__global__ __launch_bounds__(TPB) void k_mp_gather(const float* __restrict__ x, const int64_t* __restrict__ idx,
                                                   const float* __restrict__ scale, float* __restrict__ out,
                                                   int64_t M, int64_t E, int CV, int shift) {
  const Lanes L(shift);
  const int64_t e0 = L.wave * (L.rpw * UNROLL) + L.sub;
  int64_t e[UNROLL], j[UNROLL];
  float s[UNROLL];
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    e[u] = e0 + (int64_t)u * L.rpw;
    j[u] = e[u] < E ? idx[e[u]] : -1;
    if ((uint64_t)j[u] >= (uint64_t)M) j[u] = -1;
    s[u] = 1.f;
    if constexpr (SCALE) s[u] = j[u] >= 0 ? scale[j[u]] : 0.f;
  }
  for (int c = L.c0; c < CV; c += L.lpr) {
    Pack<VEC> v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      v[u] = j[u] >= 0 ? Pack<VEC>::load(x + (j[u] * CV + c) * VEC) : Pack<VEC>::fill(0.f);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if constexpr (SCALE) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[u].a[k] *= s[u];
      }
      if (e[u] < E) v[u].store(out + (e[u] * CV + c) * VEC);
    }
  }
}

// ---------------------------------------------------------------------------
// reduce
// ---------------------------------------------------------------------------
template <int OP>
__device__ __forceinline__ void combine(float& acc, int64_t& best, float v, int64_t r) {
  if constexpr (OP == GCM_MP_MAX) {
    if (best < 0 || v > acc) acc = v, best = r;      // strict: the first entry of the segment keeps a tie
  } else if constexpr (OP == GCM_MP_MIN) {
    if (best < 0 || v < acc) acc = v, best = r;
  } else {
    acc += v;
  }
}

template <int VEC, int OP, bool PERM, bool ARG>
__global__ __launch_bounds__(TPB) void k_mp_reduce(const float* __restrict__ src, const int64_t* __restrict__ ptr,
                                                   const int64_t* __restrict__ perm, float* __restrict__ out,
                                                   int64_t* __restrict__ arg, int64_t M, int64_t E, int CV,
                                                   int shift) {
  const Lanes L(shift);
  const int64_t i = L.wave * L.rpw + L.sub;
  if (i >= M) return;
  const int64_t p0 = E > 0 ? clamp_to(ptr[i], E) : 0;
  const int64_t p1 = E > 0 ? clamp_to(ptr[i + 1], E) : 0;
  const float count = (float)(p1 - p0 > 1 ? p1 - p0 : 1);
  for (int c = L.c0; c < CV; c += L.lpr) {
    float acc[VEC];
    int64_t best[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f, best[k] = -1;
    int64_t p = p0;
    for (; p + UNROLL <= p1; p += UNROLL) {
      int64_t r[UNROLL];
      Pack<VEC> v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) r[u] = row_at<PERM>(perm, p + u, E);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) v[u] = Pack<VEC>::load(src + (r[u] * CV + c) * VEC);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) combine<OP>(acc[k], best[k], v[u].a[k], r[u]);
      }
    }
    for (; p < p1; ++p) {
      const int64_t r = row_at<PERM>(perm, p, E);
      const Pack<VEC> v = Pack<VEC>::load(src + (r * CV + c) * VEC);
#pragma unroll
      for (int k = 0; k < VEC; ++k) combine<OP>(acc[k], best[k], v.a[k], r);
    }
    Pack<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.a[k] = OP == GCM_MP_MEAN ? acc[k] / count : acc[k];
    const int64_t at = (i * CV + c) * VEC;
    o.store(out + at);
    if constexpr (ARG) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) arg[at + k] = best[k];
    }
  }
}

// ---------------------------------------------------------------------------
// the gradient of max / min: to the winning row alone
// ---------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(TPB) void k_mp_select_bwd(const float* __restrict__ g_out,
                                                       const int64_t* __restrict__ arg,
                                                       const int64_t* __restrict__ dst, float* __restrict__ g_src,
                                                       int64_t M, int64_t E, int CV, int shift) {
  const Lanes L(shift);
  const int64_t e0 = L.wave * (L.rpw * UNROLL) + L.sub;
  int64_t e[UNROLL], j[UNROLL];
#pragma unroll
  for (int u = 0; u < UNROLL; ++u) {
    e[u] = e0 + (int64_t)u * L.rpw;
    j[u] = e[u] < E ? dst[e[u]] : -1;
    if ((uint64_t)j[u] >= (uint64_t)M) j[u] = -1;
  }
  for (int c = L.c0; c < CV; c += L.lpr) {
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (e[u] >= E) continue;
      Pack<VEC> v = Pack<VEC>::fill(0.f);
      if (j[u] >= 0) {
        const int64_t at = (j[u] * CV + c) * VEC;
        const Pack<VEC> g = Pack<VEC>::load(g_out + at);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v.a[k] = arg[at + k] == e[u] ? g.a[k] : 0.f;
      }
      v.store(g_src + (e[u] * CV + c) * VEC);
    }
  }
}

// ---------------------------------------------------------------------------
// softmax over the rows of a segment, per channel
// ---------------------------------------------------------------------------
// running maximum and shifted sum of one (segment, channel)
struct OnlineSum {
  float M = -INFINITY, S = 0.f;
  // One exp an entry, no branch (a segment's lanes would take both sides): e = exp(-|l - M|) is the factor that moves
  // the sum to a new maximum (whose own term is then exp(0) = 1), or the entry's term under the old one.  exp(-inf) = 0
  // at the first entry.
  __device__ __forceinline__ void add(float l) {
    const float d = l - M;
    const float e = expf(-fabsf(d));
    const bool up = d > 0.f;
    S = up ? fmaf(S, e, 1.f) : S + e;
    M = up ? l : M;
  }
};

template <int VEC, bool PERM>
__global__ __launch_bounds__(TPB) void k_mp_softmax_fwd(const float* __restrict__ src,
                                                        const int64_t* __restrict__ ptr,
                                                        const int64_t* __restrict__ perm, float* __restrict__ out,
                                                        int64_t M, int64_t E, int CV, int shift) {
  const Lanes L(shift);
  const int64_t i = L.wave * L.rpw + L.sub;
  if (i >= M) return;
  const int64_t p0 = clamp_to(ptr[i], E), p1 = clamp_to(ptr[i + 1], E);
  for (int c = L.c0; c < CV; c += L.lpr) {
    OnlineSum st[VEC];
    int64_t p = p0;
    for (; p + UNROLL <= p1; p += UNROLL) {
      int64_t r[UNROLL];
      Pack<VEC> v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) r[u] = row_at<PERM>(perm, p + u, E);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) v[u] = Pack<VEC>::load(src + (r[u] * CV + c) * VEC);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) st[k].add(v[u].a[k]);
      }
    }
    for (; p < p1; ++p) {
      const Pack<VEC> v = Pack<VEC>::load(src + (row_at<PERM>(perm, p, E) * CV + c) * VEC);
#pragma unroll
      for (int k = 0; k < VEC; ++k) st[k].add(v.a[k]);
    }
    float inv[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) inv[k] = 1.f / st[k].S;
    // the rows again (they are in the cache): the weights, four rows' loads in flight as above
    for (p = p0; p + UNROLL <= p1; p += UNROLL) {
      int64_t at[UNROLL];
      Pack<VEC> v[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) at[u] = (row_at<PERM>(perm, p + u, E) * CV + c) * VEC;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) v[u] = Pack<VEC>::load(src + at[u]);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[u].a[k] = expf(v[u].a[k] - st[k].M) * inv[k];
        v[u].store(out + at[u]);
      }
    }
    for (; p < p1; ++p) {
      const int64_t at = (row_at<PERM>(perm, p, E) * CV + c) * VEC;
      Pack<VEC> v = Pack<VEC>::load(src + at);
#pragma unroll
      for (int k = 0; k < VEC; ++k) v.a[k] = expf(v.a[k] - st[k].M) * inv[k];
      v.store(out + at);
    }
  }
}

// g_src = out (g - sum over the segment of out g), both factors of the sum from the saved out
template <int VEC, bool PERM>
__global__ __launch_bounds__(TPB) void k_mp_softmax_bwd(const float* __restrict__ g_out,
                                                        const float* __restrict__ out,
                                                        const int64_t* __restrict__ ptr,
                                                        const int64_t* __restrict__ perm, float* __restrict__ g_src,
                                                        int64_t M, int64_t E, int CV, int shift) {
  const Lanes L(shift);
  const int64_t i = L.wave * L.rpw + L.sub;
  if (i >= M) return;
  const int64_t p0 = clamp_to(ptr[i], E), p1 = clamp_to(ptr[i + 1], E);
  for (int c = L.c0; c < CV; c += L.lpr) {
    float dot[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) dot[k] = 0.f;
    int64_t p = p0;
    for (; p + UNROLL <= p1; p += UNROLL) {
      int64_t at[UNROLL];
      Pack<VEC> a[UNROLL], g[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) at[u] = (row_at<PERM>(perm, p + u, E) * CV + c) * VEC;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) a[u] = Pack<VEC>::load(out + at[u]), g[u] = Pack<VEC>::load(g_out + at[u]);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) dot[k] = fmaf(a[u].a[k], g[u].a[k], dot[k]);
      }
    }
    for (; p < p1; ++p) {
      const int64_t at = (row_at<PERM>(perm, p, E) * CV + c) * VEC;
      const Pack<VEC> a = Pack<VEC>::load(out + at), g = Pack<VEC>::load(g_out + at);
#pragma unroll
      for (int k = 0; k < VEC; ++k) dot[k] = fmaf(a.a[k], g.a[k], dot[k]);
    }
    for (p = p0; p + UNROLL <= p1; p += UNROLL) {
      int64_t at[UNROLL];
      Pack<VEC> a[UNROLL], g[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) at[u] = (row_at<PERM>(perm, p + u, E) * CV + c) * VEC;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) a[u] = Pack<VEC>::load(out + at[u]), g[u] = Pack<VEC>::load(g_out + at[u]);
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) g[u].a[k] = a[u].a[k] * (g[u].a[k] - dot[k]);
        g[u].store(g_src + at[u]);
      }
    }
    for (; p < p1; ++p) {
      const int64_t at = (row_at<PERM>(perm, p, E) * CV + c) * VEC;
      const Pack<VEC> a = Pack<VEC>::load(out + at);
      Pack<VEC> g = Pack<VEC>::load(g_out + at);
#pragma unroll
      for (int k = 0; k < VEC; ++k) g.a[k] = a.a[k] * (g.a[k] - dot[k]);
      g.store(g_src + at);
    }
  }
}

// ---------------------------------------------------------------------------
// launch shapes
// ---------------------------------------------------------------------------
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// 16-byte accesses when every row of every tensor starts on a 16-byte boundary
template <typename... P>
int vec_of(int C, const P*... ptrs) {
  return (C % 4 == 0 && (aligned16(ptrs) && ...)) ? 4 : 1;
}

// lanes per row: the power of two that covers the row's packs, at most a wave
int shift_of(int CV) {
  int s = 0;
  while (s < 6 && (1 << s) < CV) ++s;
  return s;
}

// workgroups for `rows` rows at `per_wave` rows a wave; 0: more than a grid holds
unsigned grid_of(int64_t rows, int64_t per_wave) {
  const int64_t waves = (rows + per_wave - 1) / per_wave;
  const int64_t blocks = (waves + WPB - 1) / WPB;
  return blocks > INT_MAX ? 0u : (unsigned)blocks;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int gcm_mp_gather(const float* x, const int64_t* idx, const float* scale, float* out, int64_t M, int64_t E,
                             int C, gcm_stream_t stream) {
  GCM_REQUIRE(M >= 0 && E >= 0 && C > 0);
  GCM_REQUIRE(E == 0 || (x && idx && out && M > 0));
  if (E == 0) return GCM_OK;
  const int vec = vec_of(C, x, out), CV = C / vec, shift = shift_of(CV);
  const unsigned grid = grid_of(E, (int64_t)(64 >> shift) * UNROLL);
  if (!grid) return GCM_EUNSUPPORTED;
  return gcm_pick(
      [&](auto v, auto sc) {
        hipLaunchKernelGGL((k_mp_gather<v(), bool(sc())>), dim3(grid), dim3(TPB), 0, (hipStream_t)stream, x, idx,
                           scale, out, M, E, CV, shift);
        return gcm_launch_status();
      },
      OneOf<1, 4>{vec}, Flag{scale != nullptr});
}

extern "C" int gcm_mp_reduce(const float* src, const int64_t* ptr, const int64_t* perm, int op, float* out,
                             int64_t* arg, int64_t M, int64_t E, int C, gcm_stream_t stream) {
  GCM_REQUIRE(M >= 0 && E >= 0 && C > 0);
  GCM_REQUIRE(op == GCM_MP_SUM || op == GCM_MP_MEAN || op == GCM_MP_MAX || op == GCM_MP_MIN);
  GCM_REQUIRE(!arg || op == GCM_MP_MAX || op == GCM_MP_MIN);
  GCM_REQUIRE(M == 0 || out);
  GCM_REQUIRE(E == 0 || (src && ptr && M > 0));
  if (M == 0) return GCM_OK;
  const int vec = vec_of(C, src, out), CV = C / vec, shift = shift_of(CV);
  const unsigned grid = grid_of(M, 64 >> shift);
  if (!grid) return GCM_EUNSUPPORTED;
  return gcm_pick(
      [&](auto v, auto o, auto pm, auto ag) {
        if constexpr (ag() && o() != GCM_MP_MAX && o() != GCM_MP_MIN) {
          return GCM_EINVAL;
        } else {
          hipLaunchKernelGGL((k_mp_reduce<v(), o(), bool(pm()), bool(ag())>), dim3(grid), dim3(TPB), 0,
                             (hipStream_t)stream, src, ptr, perm, out, arg, M, E, CV, shift);
          return gcm_launch_status();
        }
      },
      OneOf<1, 4>{vec}, OneOf<GCM_MP_SUM, GCM_MP_MEAN, GCM_MP_MAX, GCM_MP_MIN>{op}, Flag{perm != nullptr},
      Flag{arg != nullptr});
}

extern "C" int gcm_mp_select_bwd(const float* g_out, const int64_t* arg, const int64_t* dst, float* g_src, int64_t M,
                                 int64_t E, int C, gcm_stream_t stream) {
  GCM_REQUIRE(M >= 0 && E >= 0 && C > 0);
  GCM_REQUIRE(E == 0 || (g_out && arg && dst && g_src && M > 0));
  if (E == 0) return GCM_OK;
  const int vec = vec_of(C, g_out, g_src), CV = C / vec, shift = shift_of(CV);
  const unsigned grid = grid_of(E, (int64_t)(64 >> shift) * UNROLL);
  if (!grid) return GCM_EUNSUPPORTED;
  return gcm_pick(
      [&](auto v) {
        hipLaunchKernelGGL((k_mp_select_bwd<v()>), dim3(grid), dim3(TPB), 0, (hipStream_t)stream, g_out, arg, dst,
                           g_src, M, E, CV, shift);
        return gcm_launch_status();
      },
      OneOf<1, 4>{vec});
}

extern "C" int gcm_mp_softmax_fwd(const float* src, const int64_t* ptr, const int64_t* perm, float* out, int64_t M,
                                  int64_t E, int C, gcm_stream_t stream) {
  GCM_REQUIRE(M >= 0 && E >= 0 && C > 0);
  GCM_REQUIRE(E == 0 || (src && ptr && out && M > 0));
  if (E == 0) return GCM_OK;
  const int vec = vec_of(C, src, out), CV = C / vec, shift = shift_of(CV);
  const unsigned grid = grid_of(M, 64 >> shift);
  if (!grid) return GCM_EUNSUPPORTED;
  return gcm_pick(
      [&](auto v, auto pm) {
        hipLaunchKernelGGL((k_mp_softmax_fwd<v(), bool(pm())>), dim3(grid), dim3(TPB), 0, (hipStream_t)stream, src,
                           ptr, perm, out, M, E, CV, shift);
        return gcm_launch_status();
      },
      OneOf<1, 4>{vec}, Flag{perm != nullptr});
}

extern "C" int gcm_mp_softmax_bwd(const float* g_out, const float* out, const int64_t* ptr, const int64_t* perm,
                                  float* g_src, int64_t M, int64_t E, int C, gcm_stream_t stream) {
  GCM_REQUIRE(M >= 0 && E >= 0 && C > 0);
  GCM_REQUIRE(E == 0 || (g_out && out && ptr && g_src && M > 0));
  if (E == 0) return GCM_OK;
  const int vec = vec_of(C, g_out, out, g_src), CV = C / vec, shift = shift_of(CV);
  const unsigned grid = grid_of(M, 64 >> shift);
  if (!grid) return GCM_EUNSUPPORTED;
  return gcm_pick(
      [&](auto v, auto pm) {
        hipLaunchKernelGGL((k_mp_softmax_bwd<v(), bool(pm())>), dim3(grid), dim3(TPB), 0, (hipStream_t)stream, g_out,
                           out, ptr, perm, g_src, M, E, CV, shift);
        return gcm_launch_status();
      },
      OneOf<1, 4>{vec}, Flag{perm != nullptr});
}
