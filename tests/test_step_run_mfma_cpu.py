"""The merged step node's layers on the fp32 matrix cores (csrc/rows_cached_run.hip, include/gcm_hip_run_mfma.h), what
holds without a GPU: its section of the C ABI is exported and bound, the run object keeps the switch, and the module's
switch follows the environment and shows in merge_stats(form=True) only."""
import os
import re


def test_library_exports_every_symbol_of_the_run_mfma_header():
    from gcm import _abi, _hip
    assert '#include "gcm_hip_run_mfma.h"' in open(os.path.join(_abi.INCLUDE, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_run_mfma.h").split("#define GCM_HIP_RUN_MFMA_H")[1]))
    assert declared == {"gcm_rows_run_set_mfma", "gcm_rows_run_mfma"} == set(_hip.RUN_MFMA_PROTOTYPES)
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == _hip.RUN_MFMA_PROTOTYPES[name]


def test_run_object_keeps_the_switch():
    from gcm import _hip
    lib = _hip.lib()
    run = lib.gcm_rows_run_create()
    assert run
    assert lib.gcm_rows_run_mfma(run) == 1 and lib.gcm_rows_run_mfma(None) == 0   # (on by default)
    assert lib.gcm_rows_run_set_mfma(run, 0) == 0 and lib.gcm_rows_run_mfma(run) == 0
    assert lib.gcm_rows_run_set_mfma(run, 1) == 0 and lib.gcm_rows_run_mfma(run) == 1
    assert lib.gcm_rows_run_set_mfma(None, 1) == -1
    assert lib.gcm_rows_run_destroy(run) == 0


def test_module_switch_follows_the_environment(monkeypatch):
    import torch
    from gcm.gcm import DenseGCM
    for env, want in (({}, True), ({"GCM_RUN_MFMA": "0"}, False), ({"GCM_RUN_MFMA": "1"}, True)):
        monkeypatch.delenv("GCM_RUN_MFMA", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        mem = DenseGCM(torch.nn.Identity(), graph_size=4)
        assert mem.rows_run_mfma == want
        assert mem.merge_stats(form=True) == {"nodes": 0, "merged_steps": 0, "run_mfma": want}
        assert mem.merge_stats(head=True) == {"nodes": 0, "merged_steps": 0, "head_absorbed": 0}
        assert mem.merge_stats() == {"nodes": 0, "merged_steps": 0}
