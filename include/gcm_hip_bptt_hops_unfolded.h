/* gcm_hip_bptt_hops_unfolded.h - the A/B twin of the GEMM-form cached backward (csrc/rows_bptt_hops.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block behind gcm_hip_bptt_hops.h: include gcm_hip.h, not
 * this file.  Same conventions as gcm_hip_bptt_hops.h.  Additive: GCM_ABI_VERSION is unchanged.  The Python binding
 * reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py). */
#ifndef GCM_HIP_BPTT_HOPS_UNFOLDED_H
#define GCM_HIP_BPTT_HOPS_UNFOLDED_H

/* The same call with the kernel gcm_dense_rows_bptt_cached_hops (gcm_hip_bptt_hops.h) launched before the hop sum was folded into its products
 * (k_bptt_hops_graph: U = D2 . [W_rel2 | W_root2] through LDS, then a gather; that entry sums the D2 rows first and
 * multiplies once, k_bptt_hops_graph_fold).  Same arguments, eligibility, workspace and return codes; the gradients of
 * the two differ by re-ordered float32 sums.  Kept for the A/B (DenseGCM.rows_hops_fold, env GCM_BPTT_HOPS_FOLD=0). */
int gcm_dense_rows_bptt_cached_hops_unfolded(const float* const* saved_host, const float* const* gmx_host, int n_steps,
                                             long gmx_stride_b, long gmx_stride_h, const float* params, int has_bias,
                                             int act1, int act2, const float* cache_nodes, const float* cache_h1,
                                             const float* cache_agg1, const uint8_t* cur_host,
                                             const gcm_selector_desc* selectors, int n_selectors, int rows_written,
                                             const float* g_params_prev, float* g_params, void* workspace,
                                             size_t workspace_bytes, int B, int N, int F, int H1, int H2,
                                             gcm_stream_t stream);

#endif /* GCM_HIP_BPTT_HOPS_UNFOLDED_H */
