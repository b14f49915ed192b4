// Sums of fp64 values in one fixed order, for the scalar gradients (GINConv's g_eps, GENConv's g_t): a workgroup of
// 256 threads sums its values as a tree over LDS, and one workgroup sums the workgroups' partials.  No atomics.
#pragma once
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

}  // namespace
