"""Capture-time merging of lean cached steps (csrc/rows_cached_run.hip), what holds without a GPU: its section of the C
ABI is exported and bound, the run object's host side keeps its cap and counters, and the switch exists."""
import ctypes
import os
import re


_FUNCTIONS = {"gcm_rows_run_steps_cap", "gcm_rows_run_create", "gcm_rows_run_destroy", "gcm_rows_run_reset",
              "gcm_rows_run_set_cap", "gcm_rows_run_stats", "gcm_rows_run_enabled", "gcm_rows_run_route",
              "gcm_dense_rows_step_cached_run"}


def test_library_exports_every_symbol_of_the_run_header():
    """include/gcm_hip_run.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    from gcm import _abi, _hip
    assert '#include "gcm_hip_run.h"' in open(os.path.join(_abi.INCLUDE, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_run.h")))
    assert declared == _FUNCTIONS == set(_hip.RUN_PROTOTYPES)
    assert not declared & set(_hip.PROTOTYPES)
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == _hip.RUN_PROTOTYPES[name]
    # the step entry is gcm_dense_rows_step_cached_ws with the run object in front
    assert _hip.RUN_PROTOTYPES["gcm_dense_rows_step_cached_run"][1][1:] == \
        _hip.PROTOTYPES["gcm_dense_rows_step_cached_ws"][1]


def test_run_object_host_side():
    """create / cap / counters / destroy touch no device; the cap keeps both pointer tables inside 4 KB of arguments"""
    from gcm import _hip
    lib = _hip.lib()
    cap = lib.gcm_rows_run_steps_cap()
    assert 1 <= cap and 2 * 8 * cap + 128 <= 4096
    run = lib.gcm_rows_run_create()
    assert run
    out = (ctypes.c_int * 2)(7, 7)
    assert lib.gcm_rows_run_stats(run, out) == 0 and list(out) == [0, 0]
    assert lib.gcm_rows_run_set_cap(run, 5) == 0 and lib.gcm_rows_run_set_cap(run, cap) == 0
    assert lib.gcm_rows_run_set_cap(run, 0) == -1 and lib.gcm_rows_run_set_cap(run, cap + 1) == -1
    assert lib.gcm_rows_run_set_cap(None, 5) == -1 and lib.gcm_rows_run_stats(run, None) == -1
    assert lib.gcm_rows_run_reset(run) == 0 and lib.gcm_rows_run_reset(None) == -1
    assert lib.gcm_rows_run_enabled() in (0, 1)   # (process-wide: 0 only after a graph call has failed)
    assert lib.gcm_rows_run_destroy(run) == 0 and lib.gcm_rows_run_destroy(None) == 0


def test_module_switch_follows_the_environment(monkeypatch):
    import torch
    from gcm.gcm import DenseGCM
    for env, want in (({}, True), ({"GCM_MERGE_CAPTURED": "0"}, False), ({"GCM_MERGE_CAPTURED": "1"}, True)):
        monkeypatch.delenv("GCM_MERGE_CAPTURED", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        mem = DenseGCM(torch.nn.Identity(), graph_size=4)
        assert mem.rows_merge_captured == want and mem.rows_merge_cap is None
        assert mem.merge_stats() == {"nodes": 0, "merged_steps": 0}
