/* gcm_hip_run_mfma.h - the form of the merged step node's two layers, of the C ABI (csrc/rows_cached_run.hip, in
 * libgcm_hip.so; DESIGN 3.2.1 "the layers on the matrix cores").  An extension of the run object of gcm_hip_run.h, kept
 * in a section of its own.  Part of gcm_hip.h, which includes it inside its extern "C" block: include gcm_hip.h, not
 * this file.  Same conventions as the entries around it.  Additive: GCM_ABI_VERSION is unchanged. */
#ifndef GCM_HIP_RUN_MFMA_H
#define GCM_HIP_RUN_MFMA_H

/* The switch of one run object.  on (the default): the nodes gcm_dense_rows_step_cached_run makes for this object run
 * the layers of their steps as v_mfma_f32_16x16x4_f32 chains, one accumulator per chain of the per-step kernel's
 * product; off: the VALU form of the same kernel.  Both write the bits of the per-step launches.  Read whenever a
 * node's parameters are made: set it before a capture, not between two steps of a run. */
int gcm_rows_run_set_mfma(void* run, int on);
/* 1: the object's nodes run the matrix-core form; 0: the VALU form (or run == NULL) */
int gcm_rows_run_mfma(const void* run);

#endif /* GCM_HIP_RUN_MFMA_H */
