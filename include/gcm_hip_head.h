/* gcm_hip_head.h - the one-launch head of a rollout of the C ABI (csrc/head_fused.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the entries around it: device pointers unless named *_host, int
 * return (GCM_EINVAL on null / invalid arguments), one launch on `stream`, no allocation, no host synchronisation.
 * Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as gcm_hip.h
 * (gcm/_abi.py, gcm/_hip.py). */
#ifndef GCM_HIP_HEAD_H
#define GCM_HIP_HEAD_H

/* The packed parameter vector, the cached step's weight image and the zero fill of a fresh state, which as three
 * launches ran one behind the other in front of a rollout's first step although none reads what another writes.
 * srcs_host / lens_host: HOST arrays of n <= 16 device pointers and their float counts (a NULL pointer with a count of
 * 0 is allowed) - packed receives them back to back, what torch.cat of the flattened tensors gives.  image (may be
 * NULL): gcm_dense_rows_cached_weight_image_floats() floats, written from the SOURCES with the bits
 * gcm_dense_rows_cached_weight_image(packed, ...) writes, all three layouts; the first six sources must then be
 * W_rel1 [H1,F] | W_root1 [H1,F] | b1 [H1] | W_rel2 [H2,H1] | W_root2 [H2,H1] | b2 [H2] (F, H1, H2 <= 64, read only
 * with an image).  zero (may be NULL: no fill): zero_bytes bytes at a 16-byte aligned address are set to zero, any
 * byte count. */
int gcm_dense_rows_head_fused(const float* const* srcs_host, const size_t* lens_host, int n, float* packed,
                              float* image, int F, int H1, int H2, void* zero, size_t zero_bytes,
                              gcm_stream_t stream);

#endif /* GCM_HIP_HEAD_H */
