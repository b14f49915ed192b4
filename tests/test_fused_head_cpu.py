"""The one-launch head of a rollout (csrc/head_fused.hip), what holds without a GPU: its section of the C ABI is
exported and bound, invalid arguments are refused before anything is launched, and the switch exists."""
import ctypes
import os
import re


def test_library_exports_every_symbol_of_the_head_header():
    """include/gcm_hip_head.h is a section gcm_hip.h includes: every function it declares is exported and bound; the
    image entries it stands beside stay exported from both libraries (bench.py calls them through the debug one)."""
    import sys
    from gcm import _abi, _hip
    assert '#include "gcm_hip_head.h"' in open(os.path.join(_abi.INCLUDE, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_head.h")))
    assert declared == {"gcm_dense_rows_head_fused"} == set(_hip.HEAD_PROTOTYPES)
    assert not declared & set(_hip.PROTOTYPES)
    lib = _hip.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == _hip.HEAD_PROTOTYPES[name][1]
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import gcm_debuglib
        dbg = gcm_debuglib.lib()
    finally:
        sys.path.remove(tools)
    for handle in (lib, dbg):
        for name in ("gcm_dense_rows_cached_weight_image", "gcm_dense_rows_cached_weight_image_floats"):
            assert getattr(handle, name) is not None


def test_head_fused_refuses_invalid_arguments_without_a_launch():
    """GCM_EINVAL (-1) from the host-side checks: no device is touched, so this runs anywhere."""
    from gcm import _hip
    lib = _hip.lib()
    ptrs = (ctypes.c_void_p * 6)(*[16] * 6)       # (never dereferenced: every call below is refused on the host)
    lens = (ctypes.c_size_t * 6)(1024, 1024, 32, 1024, 1024, 32)
    fake = ctypes.c_void_p(64)
    call = lib.gcm_dense_rows_head_fused
    assert call(None, lens, 6, fake, None, 32, 32, 32, None, 0, None) == -1
    assert call(ptrs, None, 6, fake, None, 32, 32, 32, None, 0, None) == -1
    assert call(ptrs, lens, 6, None, None, 32, 32, 32, None, 0, None) == -1
    assert call(ptrs, lens, 0, fake, None, 32, 32, 32, None, 0, None) == -1
    assert call(ptrs, lens, 17, fake, None, 32, 32, 32, None, 0, None) == -1
    assert call(ptrs, lens, 6, fake, fake, 32, 32, 24, None, 0, None) == -1      # widths against the sources' lengths
    assert call(ptrs, lens, 5, fake, fake, 32, 32, 32, None, 0, None) == -1      # an image needs the six GNN tensors
    assert call(ptrs, lens, 6, fake, fake, 65, 32, 32, None, 0, None) == -1
    assert call(ptrs, lens, 6, fake, None, 32, 32, 32, ctypes.c_void_p(68), 16, None) == -1   # unaligned zero region
    holes = (ctypes.c_void_p * 6)(16, None, 16, 16, 16, 16)
    assert call(holes, lens, 6, fake, None, 32, 32, 32, None, 0, None) == -1     # a NULL source with a length


def test_module_switch_follows_the_environment(monkeypatch):
    import torch
    from gcm.gcm import DenseGCM
    for env, want in (({}, True), ({"GCM_FUSED_HEAD": "0"}, False), ({"GCM_FUSED_HEAD": "1"}, True)):
        monkeypatch.delenv("GCM_FUSED_HEAD", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        assert DenseGCM(torch.nn.Identity(), graph_size=4).rows_fused_head == want
