/* gcm_hip_run_head.h - the rollout's head launch absorbed into the merged step node, of the C ABI
 * (csrc/rows_cached_run.hip, in libgcm_hip.so; DESIGN 3.2.1 "the head absorbed").  An extension of the run object of
 * gcm_hip_run.h, kept in a section of its own.  Part of gcm_hip.h, which includes it inside its extern "C" block:
 * include gcm_hip.h, not this file.  Same conventions as the entries around it.  Additive: GCM_ABI_VERSION is unchanged. */
#ifndef GCM_HIP_RUN_HEAD_H
#define GCM_HIP_RUN_HEAD_H

/* gcm_dense_rows_head_fused (same arguments, same launch, same results) with the chain's run object in front.
 *   - run == NULL or `stream` is not being captured: exactly gcm_dense_rows_head_fused; nothing is remembered.
 *   - `stream` is being captured: the launch is captured as always, and the run remembers the node it became (checked to
 *     run k_head_fused), the capture and stream, the sources, `packed`, `image` and the zero region.
 * The first step gcm_dense_rows_step_cached_run appends to a run that starts at cur_host = 0 then absorbs that head when
 *   the head belongs to the same capture and stream; the lean node's only dependency is the head's node and the head's
 *   only dependent is the lean node; packed / image are the run's params / weight_image; the zero region is exactly the
 *   allocation nodes | adj | count (64-float paddings, the layout DenseGCM carves) the run's state pointers lie in;
 *   F = H1 = 32, N a multiple of 4, the four weight matrices 16-byte aligned:
 * the multi-step node is added on the HEAD's dependencies and runs the kernel's fresh-state form, which writes `packed`,
 * `image` and the whole state itself (the same bytes head + steps leave), and the lean node and the head's node are
 * destroyed.  Nothing between the head and step 0 can observe the difference.  If a condition fails nothing changes.
 * A graph call refused before a node is destroyed turns absorption off for the process (gcm_rows_run_absorb_enabled)
 * and the ordinary replacement follows; if the head's node can be neither destroyed nor ordered in front of the new
 * node, the step entry returns the error and the capture must be abandoned. */
int gcm_dense_rows_head_fused_run(void* run, const float* const* srcs_host, const size_t* lens_host, int n,
                                  float* packed, float* image, int F, int H1, int H2, void* zero, size_t zero_bytes,
                                  gcm_stream_t stream);
/* the switch of one run object (default on) */
int gcm_rows_run_set_absorb(void* run, int on);
/* heads absorbed by this object's nodes in the stream capture it saw last (0 or 1 per rollout captured) */
int gcm_rows_run_absorbed(const void* run);
/* 1 unless a graph call of an absorption was refused in this process */
int gcm_rows_run_absorb_enabled(void);
/* the nodes of the graph `stream` is being captured into so far (tests count what an absorption removed); -1 when the
 * stream is not being captured */
int gcm_rows_capture_node_count(gcm_stream_t stream);

#endif /* GCM_HIP_RUN_HEAD_H */
