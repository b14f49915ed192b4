/* gcm_hip_mp.h - the message-passing section of the C ABI (csrc/message_passing.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the GEN section: device pointers only, int return (GCM_EINVAL on
 * null / invalid arguments, before anything is launched), launches on `stream`, no allocation, no host
 * synchronisation and no float atomics: every sum runs in one fixed order and results are bitwise reproducible.
 * Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as gcm_hip.h
 * (gcm/_abi.py, gcm/_hip.py).
 *
 * These are the primitives under gcm.nn.MessagePassing and gcm.graph_utils (softmax, scatter): rows gathered by an
 * index, segments of rows reduced, the gradient of max / min, and a softmax over the rows of a segment.  Rows are
 * [*, C] float32, row-major and dense; any C >= 1 (16-byte accesses when C % 4 == 0 and the pointers are 16-byte
 * aligned, 4-byte ones otherwise).  Element offsets are int64: E * C is not bounded by 2^31.  A segment list is
 * (ptr [M+1], perm [E] | NULL): segment i holds the positions p in [ptr[i], ptr[i+1]), position p stands for row
 * perm[p] of the [E, C] tensor, or for row p when perm is NULL (a list already in segment order, which then pays no
 * index load).  GraphIndex's (row_ptr, csr_perm) is such a list by sink; its CSC composed with csr_perm is one by
 * source.  Index entries are read with bounds (an entry outside its range gathers 0 / is clamped into the list); every
 * store goes to the row the thread owns.  A size of 0 is allowed (nothing is launched where nothing is written) and
 * the pointers of an empty tensor may be NULL. */
#ifndef GCM_HIP_MP_H
#define GCM_HIP_MP_H

/* the reductions of gcm_mp_reduce */
#define GCM_MP_SUM 0
#define GCM_MP_MEAN 1 /* the sum divided by max(entries, 1) */
#define GCM_MP_MAX 2
#define GCM_MP_MIN 3

/* out[e,:] = (scale ? scale[idx[e]] : 1) * x[idx[e],:].  x [M,C], idx [E] in [0, M), scale [M] or NULL, out [E,C].
 * The x_i / x_j gathers of propagate; with idx = the sink of each row it is also the gradient of the sum (scale NULL)
 * and of the mean (scale = 1 / max(entries, 1)) reductions. */
int gcm_mp_gather(const float* x, const int64_t* idx, const float* scale, float* out, int64_t M, int64_t E, int C,
                  gcm_stream_t stream);

/* out[i,:] = op over the positions p of segment i of src[perm ? perm[p] : p, :], the terms taken in the order of the
 * segment.  src [E,C], out [M,C]; a segment without entries gives 0 for every op.  arg [M,C] int64 or NULL, with
 * GCM_MP_MAX / GCM_MP_MIN only: the row of src that won each (segment, channel) - the FIRST of the segment on a tie -
 * or -1 for a segment without entries.  With GCM_MP_SUM it is also the gradient of gcm_mp_gather (scale NULL): the
 * list by sink for idx = sinks, the list by source for idx = sources. */
int gcm_mp_reduce(const float* src, const int64_t* ptr, const int64_t* perm, int op, float* out, int64_t* arg,
                  int64_t M, int64_t E, int C, gcm_stream_t stream);

/* The gradient of a max / min reduction: g_src[e,c] = arg[dst[e],c] == e ? g_out[dst[e],c] : 0.  g_out [M,C], arg
 * [M,C] as gcm_mp_reduce wrote it, dst [E] the segment of each row of src, g_src [E,C] (every entry written). */
int gcm_mp_select_bwd(const float* g_out, const int64_t* arg, const int64_t* dst, float* g_src, int64_t M, int64_t E,
                      int C, gcm_stream_t stream);

/* out[r,c] = exp(src[r,c] - m) / s over the rows r of each segment, per channel: m the segment's maximum and s the
 * sum of exp(src - m), both from one pass with a running maximum (exact for logits of any size, no shift shared
 * between segments).  A segment of one row gives 1.  src, out [E,C]; every row belongs to one segment. */
int gcm_mp_softmax_fwd(const float* src, const int64_t* ptr, const int64_t* perm, float* out, int64_t M, int64_t E,
                       int C, gcm_stream_t stream);

/* g_src[r,c] = out[r,c] * (g_out[r,c] - sum over the rows q of r's segment of out[q,c] * g_out[q,c]); out as the
 * forward wrote it (both factors of the sum come from it).  g_out, out, g_src [E,C]. */
int gcm_mp_softmax_bwd(const float* g_out, const float* out, const int64_t* ptr, const int64_t* perm, float* g_src,
                       int64_t M, int64_t E, int C, gcm_stream_t stream);

#endif /* GCM_HIP_MP_H */
