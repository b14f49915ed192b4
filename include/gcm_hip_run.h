/* gcm_hip_run.h - capture-time merging of back-to-back lean cached steps of the C ABI (csrc/rows_cached_run.hip, in
 * libgcm_hip.so).  Part of gcm_hip.h, which includes it inside its extern "C" block after its typedefs and status
 * codes: include gcm_hip.h, not this file.  Same conventions as the entries around it: device pointers, int return
 * (GCM_EINVAL on null / invalid arguments), no allocation on the device, no host synchronisation.  Additive:
 * GCM_ABI_VERSION is unchanged.  The Python binding reads this file with the same reader as gcm_hip.h (gcm/_abi.py,
 * gcm/_hip.py). */
#ifndef GCM_HIP_RUN_H
#define GCM_HIP_RUN_H

/* A run object belongs to ONE chain of cached steps (the caller keeps it beside the chain's caches) and is used from one
 * host thread at a time.  It remembers the graph node the chain's last step was captured into, so that the next step,
 * when it follows directly, is appended to that node instead of becoming a node of its own.
 * gcm_rows_run_steps_cap: the most steps one node runs (its two pointer tables are kernel arguments). */
int gcm_rows_run_steps_cap(void);
void* gcm_rows_run_create(void);
int gcm_rows_run_destroy(void* run);
/* forget the remembered node: the next step starts a new run (the caller re-armed its chain).  Counters are kept. */
int gcm_rows_run_reset(void* run);
/* cap: steps per node from now on, 1 <= cap <= gcm_rows_run_steps_cap() (tests split a run with it) */
int gcm_rows_run_set_cap(void* run, int cap);
/* out2 = {nodes, merged_steps}: the graph nodes this object's steps became in the stream capture it saw last, and the
 * steps that were appended to an existing node instead of being launched.  Both 0 while nothing was captured. */
int gcm_rows_run_stats(const void* run, int* out2);
/* 1 unless a graph call failed in this process (merging is then off for good: every step is a launch of its own) */
int gcm_rows_run_enabled(void);
/* out2 = {route, last graph error}: how nodes are grown in this process - 0 not yet, 1 edited in place
 * (hipGraphKernelNodeSetParams), 2 replaced (hipGraphAddKernelNode on the old node's dependencies,
 * hipStreamUpdateCaptureDependencies, the old node destroyed - only while nothing depends on it) - and the hipError_t
 * of the graph call that was refused last (0: none) */
int gcm_rows_run_route(int* out2);

/* gcm_dense_rows_step_cached_ws (same arguments, same results to the bit) with a run object in front.
 *   - `stream` is not being captured, run == NULL, or the step is not the lean case (F = H1 = 32, H2 <= 32, tanh / tanh,
 *     at most four forward hops, 0 <= cur_host < N <= 128, GCM_STEP_IMG_V4 without GCM_STEP_ONE_WAVE /
 *     GCM_STEP_NOT_LEAN): exactly gcm_dense_rows_step_cached_ws.
 *   - `stream` is being captured and the step continues the run's remembered node - same stream and capture, the
 *     stream's only pending dependency is that node, cur_host = last cur_host + 1, the same state / cache / parameter /
 *     image / flag pointers, B, N, H2, hop set, record form, fewer than cap steps in the node, and its record and
 *     observation share no memory with the records and observations of the steps already in the node (inside one
 *     launch the steps are not ordered against one another; a record on an earlier record or observation, or an
 *     observation on an earlier record or inside the state / caches - recycled blocks, a belief fed back - starts a
 *     new run instead): the step is appended to the node's argument table (the node is edited or replaced, gcm_rows_run_route,
 *     and then runs k_step_rows_cached_img4_lean_run) and NOTHING is launched.
 *   - otherwise the lean kernel is launched (captured) as gcm_dense_rows_step_cached_ws does and its node remembered. */
int gcm_dense_rows_step_cached_run(void* run, const float* obs, float* nodes, float* adj, int64_t* count,
                                   const gcm_selector_desc* selectors, int n_selectors, const float* params,
                                   const float* weight_image, int has_bias, int act1, int act2, float* cache_h1,
                                   float* cache_agg1, float* cache_nodes, float* saved, int record, int cur_host,
                                   uint32_t* flags, void* workspace, size_t workspace_bytes, int B, int N, int F,
                                   int H1, int H2, gcm_stream_t stream);

#endif /* GCM_HIP_RUN_H */
