/* gcm_hip_bptt_hops.h - the GEMM-form cached backward of the C ABI (csrc/rows_bptt_hops.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs, status codes and
 * gcm_selector_desc: include gcm_hip.h, not this file.  Same conventions as the entries around it: device pointers
 * unless named *_host, int return (GCM_EINVAL on null / invalid arguments, GCM_EUNSUPPORTED for a case without a
 * kernel), launches on `stream`, no allocation, no host synchronisation, no float atomics: results are bitwise
 * reproducible.  Additive: GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as
 * gcm_hip.h (gcm/_abi.py, gcm/_hip.py). */
#ifndef GCM_HIP_BPTT_HOPS_H
#define GCM_HIP_BPTT_HOPS_H

/* gcm_dense_rows_bptt_cached for records whose live rows follow from FORWARD TEMPORAL HOPS and a row the host knows:
 * a chain of cached steps from empty graphs (gcm_dense_rows_step_cached with cur_host >= 0) or the records of
 * gcm_dense_rollout_tp_fwd.  The records' live lists, coefficients and headers are not read: step i wrote row
 * cur_host[i] (one byte per step, HOST array) and aggregated the rows cur_host[i] - h >= 0 for the distinct hops
 * 0 < h < 128 of `selectors` (a hop of 0: the row itself), so per graph the gradient is four small matrix products
 * and one gather (csrc/rows_bptt_hops.hip).  rows_written: the rows 0 .. rows_written - 1 of the caches
 * [B, N, .] have been written by the chain (steps of the chain that are not part of this call included: their rows
 * still receive the gradient of later steps that aggregate them); rows at or beyond it may hold anything.
 * Returns GCM_EUNSUPPORTED - the caller then uses gcm_dense_rows_bptt_cached - unless F = H1 = 32, H2 <= 32,
 * N <= 128, n_steps <= 128, has_bias carries nothing but the two bias bits, every selector is GCM_SEL_TEMPORAL with
 * GCM_DIR_FORWARD and hops >= 0, at most four distinct hops 0 < h < 128, and the cur_host[i] are distinct and
 * < rows_written <= N.  workspace: B * gcm_dense_gnn2_param_count(F, H1, H2) floats (one slab per graph);
 * g_params = g_params_prev (NULL = 0) + the gradient, summed by gcm_sum_slabs_acc. */
int gcm_dense_rows_bptt_cached_hops(const float* const* saved_host, const float* const* gmx_host, int n_steps,
                                    long gmx_stride_b, long gmx_stride_h, const float* params, int has_bias,
                                    int act1, int act2, const float* cache_nodes, const float* cache_h1,
                                    const float* cache_agg1, const uint8_t* cur_host,
                                    const gcm_selector_desc* selectors, int n_selectors, int rows_written,
                                    const float* g_params_prev, float* g_params, void* workspace,
                                    size_t workspace_bytes, int B, int N, int F, int H1, int H2, gcm_stream_t stream);

#endif /* GCM_HIP_BPTT_HOPS_H */
