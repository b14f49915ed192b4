"""ctypes binding of libgcm_hip_debug.so (include/gcm_hip_debug.h): the measurement aids of bench.py and tools/.
NOT part of the product: nothing under graph-conv-memory_amd/gcm loads this library, and the product library
(libgcm_hip.so) exports none of these entry points."""
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "graph-conv-memory_amd"))
from gcm import _abi, _hip  # noqa: E402

LIB_PATH = os.path.join(os.path.dirname(_HERE), "graph-conv-memory_amd", "gcm", "_lib", "libgcm_hip_debug.so")
# the aids of include/gcm_hip_debug.h + the product entry point they are used with (the same kernels, built from
# the same sources); float* results are c_void_p: pass ctypes.byref(c_float())
PROTOTYPES = dict(_abi.prototypes(_abi.header("gcm_hip_debug.h")),
                  gcm_dense_rows_cached_weight_image=_hip.PROTOTYPES["gcm_dense_rows_cached_weight_image"])
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not found: `make -C graph-conv-memory_amd/csrc debug`")
        _lib = _hip.bind(ctypes.CDLL(LIB_PATH), PROTOTYPES)
    return _lib


def launch_floor(grid=256, block=64, nodes=128, replays=50):
    """(us per node of a replayed HIP graph of `nodes` empty kernels, mean begin->end duration of one empty dispatch,
    begin-to-begin cadence of back-to-back empty launches without a graph) on this box."""
    a, d, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
    rc = lib().gcm_debug_empty_graph_cadence(nodes, grid, block, replays, ctypes.byref(a))
    assert rc == 0, rc
    rc = lib().gcm_debug_empty_launch_duration(nodes, grid, block, ctypes.byref(d), ctypes.byref(c))
    assert rc == 0, rc
    return a.value, d.value, c.value
