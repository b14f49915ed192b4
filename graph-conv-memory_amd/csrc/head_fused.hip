// The head of a rollout from hidden = None as ONE launch: the zero fill of the fresh state, the packed parameter vector
// (torch.cat of the flattened parameter tensors) and the cached step's weight image (k_cached_weight_image).
//
// As three launches these ran one behind the other in front of step 0 although none reads what another writes: the
// pack and the image read the same parameter tensors, and the fill reads nothing.  Here the image is laid out FROM THE
// SOURCES (not from `packed`), so the three parts are independent workgroups of one grid and nothing inside the kernel
// waits for anything else:
//   blocks [0, n_img)              the image, one element of [4][64][64] per thread, the three layouts of
//                                  k_cached_weight_image (rows_cached.hip) index for index - copies and zeros, so the
//                                  result is the same bits
//   blocks [n_img, n_img + n_pack) the packed vector, one float per thread
//   the rest                       the fill: 16-byte stores, four per thread and round, a byte tail by the first of them
// The small parts come first in the grid so that they are dispatched with the first wave of fill workgroups.
#include "gcm_common.h"

namespace gcm_rows {

constexpr int HEAD_MAX_SRCS = 16;

struct HeadSrcs {
  const float* p[HEAD_MAX_SRCS];
  unsigned off[HEAD_MAX_SRCS + 1];   // off[i]: the first float of source i in `packed`; off[n] = the total (repeated to the end)
};

__global__ __launch_bounds__(256) void k_head_fused(HeadSrcs hs, float* __restrict__ packed, float* __restrict__ image,
                                                    int F, int H1, int H2, f32x4* __restrict__ zero, size_t n16,
                                                    unsigned tail_bytes, int n_img, int n_pack, int n_fill) {
  const int blk = blockIdx.x, tid = threadIdx.x;
  if (blk < n_img) {
    // (k_cached_weight_image with params + offset replaced by the source tensors: W_rel1, W_root1, b1, W_rel2, W_root2, b2)
    const int e = blk * 256 + tid;   // over [4][64][64]: n_img * 256 == 4 * 64 * 64
    const int m = e >> 12, k = (e >> 6) & 63, lane = e & 63;
    float v = 0.f;
    if (m < 2) { if (lane < H1 && k < F) v = (m == 0 ? hs.p[0] : hs.p[1])[(size_t)lane * F + k]; }
    else { if (lane < H2 && k < H1) v = (m == 2 ? hs.p[3] : hs.p[4])[(size_t)lane * H1 + k]; }
    image[e] = v;
    image[4 * 64 * 64 + ((((m >> 1) * 64 + k) * 64 + lane) << 1) + (m & 1)] = v;
    if (lane < 32 && k < 32)
      image[2 * 4 * 64 * 64 + ((((m >> 1) * 16 + (k & 15)) * 64 + (k >> 4) * 32 + lane) << 1) + (m & 1)] = v;
    return;
  }
  if (blk < n_img + n_pack) {
    const unsigned e = (unsigned)(blk - n_img) * 256u + (unsigned)tid;
    if (e >= hs.off[HEAD_MAX_SRCS]) return;
    // the source that holds float e: the last one that starts at or before it (empty sources share their successor's start)
    const float* src = hs.p[0];
    unsigned base = 0;
#pragma unroll
    for (int i = 1; i < HEAD_MAX_SRCS; ++i) {
      const bool in = e >= hs.off[i] && hs.off[i] < hs.off[HEAD_MAX_SRCS];
      src = in ? hs.p[i] : src;
      base = in ? hs.off[i] : base;
    }
    packed[e] = src[e - base];
    return;
  }
  const int fb = blk - n_img - n_pack;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  const size_t stride = (size_t)n_fill * 256;
  for (size_t i = (size_t)fb * 256 + tid; i < n16; i += 4 * stride) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u * stride < n16) zero[i + u * stride] = z;
  }
  if (fb == 0 && (unsigned)tid < tail_bytes) reinterpret_cast<unsigned char*>(zero + n16)[tid] = 0;
}

}  // namespace gcm_rows

extern "C" int gcm_dense_rows_head_fused(const float* const* srcs_host, const size_t* lens_host, int n, float* packed,
                                         float* image, int F, int H1, int H2, void* zero, size_t zero_bytes,
                                         gcm_stream_t stream) {
  GCM_REQUIRE(srcs_host && lens_host && packed && n > 0 && n <= gcm_rows::HEAD_MAX_SRCS);
  gcm_rows::HeadSrcs hs{};
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    GCM_REQUIRE(srcs_host[i] || lens_host[i] == 0);
    hs.p[i] = srcs_host[i];
    hs.off[i] = (unsigned)total;
    total += lens_host[i];
    GCM_REQUIRE(total < ((size_t)1 << 31));
  }
  GCM_REQUIRE(total > 0);
  for (int i = n; i <= gcm_rows::HEAD_MAX_SRCS; ++i) hs.off[i] = (unsigned)total;
  if (image) {   // the six GNN tensors lead the vector ("packed parameter vector" of gcm_hip.h), every one present
    GCM_REQUIRE(F > 0 && F <= 64 && H1 > 0 && H1 <= 64 && H2 > 0 && H2 <= 64 && n >= 6);
    GCM_REQUIRE(lens_host[0] == (size_t)H1 * F && lens_host[1] == (size_t)H1 * F && lens_host[2] == (size_t)H1 &&
                lens_host[3] == (size_t)H2 * H1 && lens_host[4] == (size_t)H2 * H1 && lens_host[5] == (size_t)H2);
  }
  if (!zero) zero_bytes = 0;
  GCM_REQUIRE((reinterpret_cast<uintptr_t>(zero) & 15) == 0);
  const size_t n16 = zero_bytes / 16;
  const unsigned tail = (unsigned)(zero_bytes % 16);
  const int n_img = image ? 4 * 64 * 64 / 256 : 0;
  const int n_pack = (int)((total + 255) / 256);
  // (four 16-byte stores per thread and round; 2048 workgroups of four waves fill every CU of the device twice over)
  const size_t want = (n16 + 4 * 256 - 1) / (4 * 256);
  const int n_fill = zero_bytes == 0 ? 0 : (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
  hipLaunchKernelGGL(gcm_rows::k_head_fused, dim3(n_img + n_pack + n_fill), dim3(256), 0, (hipStream_t)stream, hs, packed,
                     image, F, H1, H2, reinterpret_cast<f32x4*>(zero), n16, tail, n_img, n_pack, n_fill);
  return gcm_launch_status();
}
