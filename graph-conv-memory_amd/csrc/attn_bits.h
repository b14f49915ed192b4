// The bit image of a dense neighbourhood pattern, shared by the attention and gated layers (csrc/gatconv.hip,
// csrc/transformerconv.hip, csrc/resgatedconv.hip, csrc/gatedgraphconv.hip): the adjacency is read once
// (csrc/attn_bits.hip), the kernels read the image.  Also their lane-group reduction.
#pragma once
#include "gcn_mm.h"

namespace gcm_mm {

constexpr int GT = 32;  // neighbour / row tile of the dense attention kernels

// bits[r, w] bit t: adj[r, 32 w + t] != 0 (the diagonal set when add_loop); R = B N rows of W = ceil(N / 32) words
int mask_bits(const float* adj, unsigned* bits, int64_t R, int N, int W, int add_loop, hipStream_t s);

// bitsT[b, j, w] bit t = bits[b, 32 w + t, j / 32] bit j % 32
int mask_bits_t(const unsigned* bits, unsigned* bitsT, int64_t R, int N, int W, hipStream_t s);

// the sum over a group of G adjacent lanes
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;  // the same bits in every lane of the group
}

}  // namespace gcm_mm
