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
// (What each element is and where it goes: rows_head.h, shared with the merged step kernel's fresh-state form, which
// does the same work beside its steps when the head's node has been absorbed - DESIGN 3.2.1.)
#include "gcm_common.h"
#include "rows_head.h"

namespace gcm_rows {

__global__ __launch_bounds__(256) void k_head_fused(HeadSrcs hs, float* __restrict__ packed, float* __restrict__ image,
                                                    int F, int H1, int H2, f32x4* __restrict__ zero, size_t n16,
                                                    unsigned tail_bytes, int n_img, int n_pack, int n_fill) {
  const int blk = blockIdx.x, tid = threadIdx.x;
  if (blk < n_img) {
    // (k_cached_weight_image with params + offset replaced by the source tensors: W_rel1, W_root1, b1, W_rel2, W_root2, b2)
    const int e = blk * 256 + tid;   // over [4][64][64]: n_img * 256 == 4 * 64 * 64
    head_image_store(image, e, head_image_value(hs, e >> 12, (e >> 6) & 63, e & 63, F, H1, H2));
    return;
  }
  if (blk < n_img + n_pack) {
    const unsigned e = (unsigned)(blk - n_img) * 256u + (unsigned)tid;
    if (e >= hs.off[HEAD_MAX_SRCS]) return;
    packed[e] = head_packed_value(hs, e);
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

const void* head_fused_kernel() { return (const void*)k_head_fused; }

}  // namespace gcm_rows

extern "C" int gcm_dense_rows_head_fused(const float* const* srcs_host, const size_t* lens_host, int n, float* packed,
                                         float* image, int F, int H1, int H2, void* zero, size_t zero_bytes,
                                         gcm_stream_t stream) {
  GCM_REQUIRE(srcs_host && lens_host && packed && n > 0 && n <= gcm_rows::HEAD_MAX_SRCS);
  gcm_rows::HeadSrcs hs;
  size_t total = 0;
  GCM_REQUIRE(gcm_rows::head_make_srcs(srcs_host, lens_host, n, hs, total));
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
