// Sums of fp64 values in one fixed order, for the scalar gradients (GINConv's and GINEConv's g_eps, GENConv's g_t): a workgroup of
// 256 threads sums its values as a tree over LDS, and one workgroup sums the workgroups' partials.  No atomics.
#pragma once
#include <algorithm>

#include "gcm_common.h"

namespace {

// sum of the 256 per-thread values in a fixed order (every thread of the workgroup calls it; sp: 256 doubles of LDS)
__device__ __forceinline__ double block_sum(double s, double* sp) {
  sp[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sp[threadIdx.x] += sp[threadIdx.x + w];
    __syncthreads();
  }
  return sp[0];
}

// pass 2 (one workgroup): out[0] = sum of the n partials in a fixed order
__global__ __launch_bounds__(256) void k_sum_parts(const double* __restrict__ part, int n, float* __restrict__ out) {
  __shared__ double sp[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += part[i];
  const double total = block_sum(s, sp);
  if (threadIdx.x == 0) out[0] = (float)total;
}

int sum_parts(const double* part, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(256), 0, s, part, n, out);
  return gcm_launch_status();
}

// The dot product sum_e a[e] b[e] -> out[0] in a fixed order (g_eps of GINConv and GINEConv).  Pass 1: part[blk] = the
// sum of a[e] b[e] over the block's element range [blk * chunk, (blk + 1) * chunk), in fp64 (every product exact),
// lanes and waves combined in a fixed order; pass 2 is sum_parts
constexpr int DOT_BLOCKS = 1024;  // at most; chunk a multiple of 256

__global__ __launch_bounds__(256) void k_dot_parts(const float* __restrict__ a, const float* __restrict__ b,
                                                   int64_t L, int64_t chunk, double* __restrict__ part) {
  __shared__ double sp[256];
  const int64_t e0 = (int64_t)blockIdx.x * chunk;
  const int64_t e1 = min(L, e0 + chunk);
  double s = 0.0;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) s += (double)a[e] * (double)b[e];
  const double total = block_sum(s, sp);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

void dot_plan(int64_t L, int* nblocks, int64_t* chunk) {
  int64_t c = (L + DOT_BLOCKS - 1) / DOT_BLOCKS;
  c = std::max<int64_t>((c + 255) / 256 * 256, 4096);
  *chunk = c;
  *nblocks = (int)((L + c - 1) / c);
}

size_t dot_ws_bytes(int64_t L) {
  int n;
  int64_t c;
  dot_plan(L, &n, &c);
  return ((size_t)n * sizeof(double) + 255) & ~(size_t)255;
}

int dot_sum(const float* a, const float* b, int64_t L, float* out, void* workspace, hipStream_t s) {
  int n;
  int64_t c;
  dot_plan(L, &n, &c);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(k_dot_parts, dim3(n), dim3(256), 0, s, a, b, L, c, part);
  const int rc = gcm_launch_status();
  return rc ? rc : sum_parts(part, n, out, s);
}

}  // namespace
