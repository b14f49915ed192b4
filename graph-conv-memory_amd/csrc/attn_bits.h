// The bit image of a dense attention pattern, shared by the attention layers (csrc/gatconv.hip,
// csrc/transformerconv.hip): the adjacency is read once, the kernels read the image.
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

}  // namespace
