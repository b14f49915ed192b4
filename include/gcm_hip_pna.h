/* gcm_hip_pna.h - the PNAConv / DensePNAConv section of the C ABI (csrc/pnaconv.hip, in libgcm_hip.so).
 * Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status codes: include
 * gcm_hip.h, not this file.  Same conventions as the other sections: device pointers only, one *_bwd_workspace_bytes
 * query per backward, int return (GCM_EINVAL on null / invalid arguments, GCM_EUNSUPPORTED beyond the limits below),
 * launches on `stream`, no allocation and no host synchronisation.  Additive: GCM_ABI_VERSION is unchanged.  The Python
 * binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py, gcm/_hip.py).
 *
 * Principal Neighbourhood Aggregation (Corso et al. 2020), per tower t of `towers` (Fi = in_channels / towers with
 * divide_input, else in_channels; Fo = out_channels / towers; x_t: the tower's Fi columns of x, or all of x):
 *   message     m_e  = a_i + b_src(e),   [a | b] = x_t w_pre[t]^T + b_pre[t]        (w_pre[t]: [2 Fi, Fi], rows = [dst; src])
 *   aggregators over the n_i messages of i, per channel: sum, mean, min, max, var = mean(m^2) - mean(m)^2 (computed
 *               about the first neighbour's value: an all-equal neighbourhood gives exactly 0), std = sqrt(max(var,
 *               1e-5)) set to 0 where that is <= sqrt(1e-5); every one 0 where n_i = 0; a tie in min / max goes to the
 *               lowest j (dense) or the first CSR entry
 *   scalers     identity 1, amplification log(n+1) / avg_log, attenuation avg_log / log(max(n,1)+1), linear n / avg_lin,
 *               inverse_linear avg_lin / max(n,1);   avg_deg = (avg_lin, avg_log) on the device
 *   cat[i,t]    = [x_t | scaler-major, then aggregator, blocks of Fi]               K1 = (1 + A S) Fi columns
 *   h_t = cat[i,t] w_post[t]^T + b_post[t]   (w_post[t]: [Fo, K1]);   out = h w_lin^T + b_lin, or out = h if w_lin is NULL
 * aggrs / scalers: the A (S) codes of the lists in order, 3 bits each from bit 0; 1 <= A, S <= 8.
 * in_channels, out_channels <= 128; dense N <= 32767, B <= 65535; E < 2^31. */
#ifndef GCM_HIP_PNA_H
#define GCM_HIP_PNA_H

#define GCM_PNA_SUM 0
#define GCM_PNA_MEAN 1
#define GCM_PNA_MIN 2
#define GCM_PNA_MAX 3
#define GCM_PNA_VAR 4
#define GCM_PNA_STD 5

#define GCM_PNA_IDENTITY 0
#define GCM_PNA_AMPLIFICATION 1
#define GCM_PNA_ATTENUATION 2
#define GCM_PNA_LINEAR 3
#define GCM_PNA_INVERSE_LINEAR 4

/* Dense: adj[b,i,j] != 0 means i aggregates from j (only the pattern is read; add_loop sets the diagonal).
 * x [B,N,in], adj [B,N,N], w_pre [T,2Fi,Fi], b_pre [T,2Fi], w_post [T,Fo,K1], b_post [T,Fo], w_lin [out,out] and b_lin
 * [out] or NULL, out [B,N,out].  Saved for the backward: ab [B,N,T,2Fi], cat [B,N,T,K1], h [B,N,out] (with w_lin), cnt
 * [B,N] = n_i, stat [B,N,2,T Fi] (the neighbourhood mean of b; std), winner [B,N,2,T Fi] (argmin, argmax: j or -1). */
int gcm_dense_pnaconv_fwd(const float* x, const float* adj, const float* w_pre, const float* b_pre,
                          const float* w_post, const float* b_post, const float* w_lin, const float* b_lin,
                          const float* avg_deg, float* out, float* ab, float* cat, float* h, int32_t* cnt,
                          float* stat, int16_t* winner, int B, int N, int in_channels, int out_channels, int towers,
                          int divide_input, int aggrs, int A, int scalers, int S, int add_loop,
                          gcm_stream_t stream);

/* Backward.  Outputs (NULL to skip, all overwritten): g_x [B,N,in], g_w_pre, g_b_pre, g_w_post, g_b_post, g_w_lin,
 * g_b_lin in the shapes of the operands.  adj has no gradient. */
size_t gcm_dense_pnaconv_bwd_workspace_bytes(int B, int N, int in_channels, int out_channels, int towers,
                                             int divide_input, int A, int S);
int gcm_dense_pnaconv_bwd(const float* g_out, const float* x, const float* adj, const float* w_pre,
                          const float* w_post, const float* w_lin, const float* avg_deg, const float* ab,
                          const float* cat, const float* h, const int32_t* cnt, const float* stat,
                          const int16_t* winner, float* g_x, float* g_w_pre, float* g_b_pre, float* g_w_post,
                          float* g_b_post, float* g_w_lin, float* g_b_lin, void* workspace, size_t workspace_bytes,
                          int B, int N, int in_channels, int out_channels, int towers, int divide_input, int aggrs,
                          int A, int scalers, int S, int add_loop, gcm_stream_t stream);

/* Sparse: the same layer over a destination CSR (row_ptr [M+1], col [E] = sources); every entry is one message,
 * duplicates and self loops included.  x [M,in], out [M,out]; saved as above with rows = M; winner: the CSR entry. */
int gcm_csr_pnaconv_fwd(const float* x, const int64_t* row_ptr, const int64_t* col, const float* w_pre,
                        const float* b_pre, const float* w_post, const float* b_post, const float* w_lin,
                        const float* b_lin, const float* avg_deg, float* out, float* ab, float* cat, float* h,
                        int32_t* cnt, float* stat, int32_t* winner, int64_t M, int64_t E, int in_channels,
                        int out_channels, int towers, int divide_input, int aggrs, int A, int scalers, int S,
                        gcm_stream_t stream);

/* Backward.  col_ptr / rows / perm: the CSC by source as for gcm_csr_graphconv_bwd (may be NULL when E == 0). */
size_t gcm_csr_pnaconv_bwd_workspace_bytes(int64_t M, int64_t E, int in_channels, int out_channels, int towers,
                                           int divide_input, int A, int S);
int gcm_csr_pnaconv_bwd(const float* g_out, const float* x, const int64_t* col_ptr, const int64_t* rows,
                        const int64_t* perm, const float* w_pre, const float* w_post, const float* w_lin,
                        const float* avg_deg, const float* ab, const float* cat, const float* h, const int32_t* cnt,
                        const float* stat, const int32_t* winner, float* g_x, float* g_w_pre, float* g_b_pre,
                        float* g_w_post, float* g_b_post, float* g_w_lin, float* g_b_lin, void* workspace,
                        size_t workspace_bytes, int64_t M, int64_t E, int in_channels, int out_channels, int towers,
                        int divide_input, int aggrs, int A, int scalers, int S, gcm_stream_t stream);

#endif /* GCM_HIP_PNA_H */
