"""The rollout's head launch absorbed into the merged step node (csrc/rows_cached_run.hip, include/gcm_hip_run_head.h),
what holds without a GPU: its section of the C ABI is exported and bound, the run object keeps the switch and its
counter, the head entry refuses what gcm_dense_rows_head_fused refuses, and the module's switch follows the
environment."""
import ctypes
import os
import re


def test_library_exports_every_symbol_of_the_run_head_header():
    from gcm import _abi, _hip
    assert '#include "gcm_hip_run_head.h"' in open(os.path.join(_abi.INCLUDE, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_run_head.h").split("#define GCM_HIP_RUN_HEAD_H")[1]))
    declared -= {"gcm_dense_rows_head_fused"}   # (named in the comment of the entry that wraps it)
    assert declared == {"gcm_dense_rows_head_fused_run", "gcm_rows_run_set_absorb", "gcm_rows_run_absorbed",
                        "gcm_rows_run_absorb_enabled", "gcm_rows_capture_node_count"} == set(_hip.RUN_HEAD_PROTOTYPES)
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == _hip.RUN_HEAD_PROTOTYPES[name]
    # the head entry is gcm_dense_rows_head_fused with the run object in front
    assert _hip.RUN_HEAD_PROTOTYPES["gcm_dense_rows_head_fused_run"][1][1:] == \
        _hip.HEAD_PROTOTYPES["gcm_dense_rows_head_fused"][1]


def test_run_object_switch_and_counter_host_side():
    from gcm import _hip
    lib = _hip.lib()
    run = lib.gcm_rows_run_create()
    assert run
    assert lib.gcm_rows_run_absorbed(run) == 0 and lib.gcm_rows_run_absorbed(None) == 0
    assert lib.gcm_rows_run_set_absorb(run, 0) == 0 and lib.gcm_rows_run_set_absorb(run, 1) == 0
    assert lib.gcm_rows_run_set_absorb(None, 1) == -1
    assert lib.gcm_rows_run_absorb_enabled() in (0, 1)   # (process-wide: 0 only after a graph call was refused)
    # invalid arguments are refused before anything is launched or remembered, as by the entry it wraps
    ptrs, lens = (ctypes.c_void_p * 1)(0), (ctypes.c_size_t * 1)(4)
    assert lib.gcm_dense_rows_head_fused_run(run, ptrs, lens, 1, None, None, 32, 32, 32, None, 0, None) == -1
    assert lib.gcm_dense_rows_head_fused_run(run, None, None, 0, None, None, 32, 32, 32, None, 0, None) == -1
    assert lib.gcm_rows_run_absorbed(run) == 0
    assert lib.gcm_rows_run_destroy(run) == 0


def test_module_switch_follows_the_environment(monkeypatch):
    import torch
    from gcm.gcm import DenseGCM
    for env, want in (({}, True), ({"GCM_ABSORB_HEAD": "0"}, False), ({"GCM_ABSORB_HEAD": "1"}, True)):
        monkeypatch.delenv("GCM_ABSORB_HEAD", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        mem = DenseGCM(torch.nn.Identity(), graph_size=4)
        assert mem.rows_absorb_head == want
        assert mem.merge_stats(head=True) == {"nodes": 0, "merged_steps": 0, "head_absorbed": 0}
        assert mem.merge_stats() == {"nodes": 0, "merged_steps": 0}
