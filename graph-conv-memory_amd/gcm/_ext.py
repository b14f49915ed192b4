"""Loader / builder of the C++ host path (csrc/torch_ext/step_ext.cpp): the autograd nodes and host loops of
the per-step DenseGCM / SparseGCM calls, around the C-ABI calls into libgcm_hip.so.  It exists because the
per-step loop of the reference's callers is host-bound.  Built in-tree by `python __graft_entry__.py`
(`build()` below) and required: there is no Python twin of its nodes."""
import importlib.util
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_DIR = os.path.join(_HERE, "_lib")
_EXT_DIR = os.path.join(_LIB_DIR, "ext")
_NAME = "gcm_torch_ext"
_SO = os.path.join(_EXT_DIR, _NAME + ".so")
_SRC = os.path.join(os.path.dirname(_HERE), "csrc", "torch_ext", "step_ext.cpp")

_mod = None


def build(verbose=False):
    """Compile the extension into gcm/_lib/ext/ (host C++ only; links libgcm_hip.so)."""
    import torch
    from torch.utils import cpp_extension
    from . import _abi, _hip
    _hip.lib()   # libgcm_hip.so must exist (and is then already mapped when the module loads)
    os.makedirs(_EXT_DIR, exist_ok=True)
    global _mod
    _mod = cpp_extension.load(
        name=_NAME, sources=[_SRC],
        # host C++ only; the ROCm include path is for c10/hip (current stream / device of the
        # process), whose library torch has loaded already
        extra_include_paths=[_abi.INCLUDE, os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")],
        extra_cflags=["-O2", "-std=c++17", "-Wno-deprecated-declarations"]
        + (["-DGCM_HOST_PROF"] if os.environ.get("GCM_HOST_PROF") == "1" else []),   # (tools/hosttime.py: segments of RowsFast.step)
        extra_ldflags=[f"-L{_LIB_DIR}", "-lgcm_hip", "-Wl,-rpath,'$$ORIGIN/..'",
                       f"-L{os.path.join(os.path.dirname(torch.__file__), 'lib')}", "-lc10_hip",
                       "-ltorch_python"],
        build_directory=_EXT_DIR, verbose=verbose)
    return _mod


def module():
    """The built extension module; raises _hip.HipLibraryError when it has not been built."""
    global _mod
    if _mod is None:
        import torch  # noqa: F401  (libtorch must be loaded first)
        from . import _hip
        if not os.path.exists(_SO):
            raise _hip.HipLibraryError(f"{_SO} not found: build it with `python __graft_entry__.py`")
        _hip.lib()
        spec = importlib.util.spec_from_file_location(_NAME, _SO)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _mod = mod
    return _mod
