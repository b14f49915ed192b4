// The bit image of a dense neighbourhood pattern, shared by the attention and gated layers (csrc/gatconv.hip,
// csrc/transformerconv.hip, csrc/resgatedconv.hip, csrc/gatedgraphconv.hip): the adjacency is read once, the kernels
// read the image.  Also their lane-group reduction.
#pragma once
#include "gcn_mm.h"

namespace {

constexpr int GT = 32;  // neighbour / row tile of the dense attention kernels

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

// the sum over a group of G adjacent lanes
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;  // the same bits in every lane of the group
}

}  // namespace
