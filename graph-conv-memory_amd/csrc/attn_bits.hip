// The pattern-image kernels of attn_bits.h, compiled once for the whole library.
#include "attn_bits.h"

namespace gcm_mm {
namespace {

// bits[r, w] bit t: adj[r, 32 w + t] != 0 (the diagonal set when add_loop).  One wave per row.
__global__ __launch_bounds__(256) void k_gat_mask_bits(const float* __restrict__ adj, unsigned* __restrict__ bits,
                                                       int64_t rows, int N, int W, int add_loop) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int i = (int)(row % N);
  const float* a = adj + (size_t)row * N;
  for (int j0 = 0; j0 < N; j0 += 64) {
    const int j = j0 + lane;
    const bool v = j < N && ((add_loop && j == i) || a[j] != 0.f);
    const unsigned long long m = __ballot(v);
    const int w = j0 / 32 + lane;
    if (lane < 2 && w < W) bits[(size_t)row * W + w] = lane ? (unsigned)(m >> 32) : (unsigned)m;
  }
}

// bitsT[b, j, w] bit t = bits[b, 32 w + t, j / 32] bit j % 32.  One thread per word.
__global__ __launch_bounds__(256) void k_mask_bits_t(const unsigned* __restrict__ bits, unsigned* __restrict__ bitsT,
                                                     int64_t R, int N, int W) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= R * W) return;
  const int64_t row = t / W;
  const int w = (int)(t - row * W);
  const int j = (int)(row % N);
  const size_t rb = (size_t)(row - j);
  unsigned word = 0;
  for (int k = 0; k < 32; ++k) {
    const int i = w * 32 + k;
    if (i < N) word |= ((bits[(rb + i) * W + (j >> 5)] >> (j & 31)) & 1u) << k;
  }
  bitsT[t] = word;
}

}  // namespace

int mask_bits(const float* adj, unsigned* bits, int64_t R, int N, int W, int add_loop, hipStream_t s) {
  hipLaunchKernelGGL(k_gat_mask_bits, dim3(blocks(R, 4)), dim3(256), 0, s, adj, bits, R, N, W, add_loop);
  return gcm_launch_status();
}

int mask_bits_t(const unsigned* bits, unsigned* bitsT, int64_t R, int N, int W, hipStream_t s) {
  hipLaunchKernelGGL(k_mask_bits_t, dim3(blocks(R * W, 256)), dim3(256), 0, s, bits, bitsT, R, N, W);
  return gcm_launch_status();
}

}  // namespace gcm_mm
