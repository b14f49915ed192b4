"""ctypes binding of libgcm_hip.so (C ABI: include/gcm_hip.h).

There is NO CPU fallback: importing is always allowed (so host-side logic can
be inspected anywhere) but the first kernel call raises if the library is
missing or a tensor is not on a HIP device.
"""
import ctypes
import os

import torch

from . import _abi

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libgcm_hip.so")
_lib = None

# The binding is derived from include/gcm_hip.h (gcm/_abi.py reads it once, here): a declaration the reader cannot
# map raises at import.  PROTOTYPES: name -> (restype, argtypes) of every entry point.
_HEADER = _abi.header("gcm_hip.h")
PROTOTYPES = _abi.prototypes(_HEADER)
_CONSTANTS = _abi.constants(_HEADER)
# the section gcm_hip.h includes from gcm_hip_aggr.h (mean / max aggregation), read the same way
_AGGR_HEADER = _abi.header("gcm_hip_aggr.h")
AGGR_PROTOTYPES = _abi.prototypes(_AGGR_HEADER)
_CONSTANTS.update(_abi.constants(_AGGR_HEADER))
# and the section from gcm_hip_learned_det.h (LearnedEdge(deterministic=True): hard sparsemax selection)
_LEARNED_DET_HEADER = _abi.header("gcm_hip_learned_det.h")
LEARNED_DET_PROTOTYPES = _abi.prototypes(_LEARNED_DET_HEADER)
# and the section from gcm_hip_transformer.h (TransformerConv / DenseTransformerConv)
_TRANSFORMER_HEADER = _abi.header("gcm_hip_transformer.h")
TRANSFORMER_PROTOTYPES = _abi.prototypes(_TRANSFORMER_HEADER)
# and the section from gcm_hip_reset.h (per-graph episode resets: DenseGCM.rollout(reset=...), DenseGCM.reset_hidden)
_RESET_HEADER = _abi.header("gcm_hip_reset.h")
RESET_PROTOTYPES = _abi.prototypes(_RESET_HEADER)
# and the section from gcm_hip_gin.h (the aggregation of GINConv / DenseGINConv and its gradients)
GIN_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_gin.h"))
# and the section from gcm_hip_gine.h (the aggregation of GINEConv / DenseGINEConv, and RelativeEdgeAttr)
_GINE_HEADER = _abi.header("gcm_hip_gine.h")
GINE_PROTOTYPES = _abi.prototypes(_GINE_HEADER)
_CONSTANTS.update(_abi.constants(_GINE_HEADER))
# and the section from gcm_hip_gatv2.h (GATv2Conv / DenseGATv2Conv with edge_dim)
_GATV2_HEADER = _abi.header("gcm_hip_gatv2.h")
GATV2_PROTOTYPES = _abi.prototypes(_GATV2_HEADER)
_CONSTANTS.update(_abi.constants(_GATV2_HEADER))
# and the section from gcm_hip_transformer_edge.h (TransformerConv / DenseTransformerConv with edge_dim)
_TRE_HEADER = _abi.header("gcm_hip_transformer_edge.h")
TRE_PROTOTYPES = _abi.prototypes(_TRE_HEADER)
_CONSTANTS.update(_abi.constants(_TRE_HEADER))
# and the section from gcm_hip_bptt_hops.h (the GEMM-form backward of forward-hop cached chains)
BPTT_HOPS_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_bptt_hops.h"))
# and the section from gcm_hip_bptt_hops_unfolded.h (that backward before the hop sum was folded into its products: the A/B)
BPTT_HOPS_UNFOLDED_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_bptt_hops_unfolded.h"))
# and the section from gcm_hip_resgated.h (ResGatedGraphConv / DenseResGatedGraphConv)
RESGATED_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_resgated.h"))
# and the section from gcm_hip_gated.h (GatedGraphConv / DenseGatedGraphConv)
GATED_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_gated.h"))
# and the section from gcm_hip_tag.h (TAGConv / DenseTAGConv)
TAG_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_tag.h"))
# and the section from gcm_hip_pna.h (PNAConv / DensePNAConv)
_PNA_HEADER = _abi.header("gcm_hip_pna.h")
PNA_PROTOTYPES = _abi.prototypes(_PNA_HEADER)
_CONSTANTS.update(_abi.constants(_PNA_HEADER))
# and the section from gcm_hip_rgcn.h (RGCNConv / DenseRGCNConv, and the merge of the TypedEdge selector)
RGCN_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_rgcn.h"))
# and the section from gcm_hip_gen.h (the softmax aggregation of GENConv / DenseGENConv and its gradients)
GEN_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_gen.h"))
# and the section from gcm_hip_edgeconv.h (the per-edge MLP and max of EdgeConv / DenseEdgeConv and its gradients)
EDGECONV_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_edgeconv.h"))
# and the section from gcm_hip_mp.h (gcm.nn.MessagePassing: gather, segment reductions, segment softmax)
_MP_HEADER = _abi.header("gcm_hip_mp.h")
MP_PROTOTYPES = _abi.prototypes(_MP_HEADER)
_CONSTANTS.update(_abi.constants(_MP_HEADER))
# and the section from gcm_hip_bridge.h (gcm.gcm.DenseToSparse / SparseToDense: adjacency <-> edge list and index)
_BRIDGE_HEADER = _abi.header("gcm_hip_bridge.h")
BRIDGE_PROTOTYPES = _abi.prototypes(_BRIDGE_HEADER)
_CONSTANTS.update(_abi.constants(_BRIDGE_HEADER))
# and the section from gcm_hip_window.h (SparseGCM.drop_oldest / reset_hidden / overflow="wrap")
_WINDOW_HEADER = _abi.header("gcm_hip_window.h")
WINDOW_PROTOTYPES = _abi.prototypes(_WINDOW_HEADER)
_CONSTANTS.update(_abi.constants(_WINDOW_HEADER))
# and the section from gcm_hip_segments.h (SparseGCM.rollout(x, reset=mask): resets inside one call)
_SEGMENT_HEADER = _abi.header("gcm_hip_segments.h")
SEGMENT_PROTOTYPES = _abi.prototypes(_SEGMENT_HEADER)
_CONSTANTS.update(_abi.constants(_SEGMENT_HEADER))
# and the section from gcm_hip_head.h (the head of a rollout as one launch: packed vector, weight image, zero state)
HEAD_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_head.h"))
# and the section from gcm_hip_run.h (lean cached steps captured back to back as one graph node)
RUN_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_run.h"))
# and the section from gcm_hip_run_head.h (the rollout's head launch absorbed into that node)
RUN_HEAD_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_run_head.h"))
# and the section from gcm_hip_run_mfma.h (that node's layers on the fp32 matrix cores, and the switch back)
RUN_MFMA_PROTOTYPES = _abi.prototypes(_abi.header("gcm_hip_run_mfma.h"))
# and the section from gcm_hip_knn.h (KNNEdge: the distance modes that carry k)
_KNN_HEADER = _abi.header("gcm_hip_knn.h")
KNN_PROTOTYPES = _abi.prototypes(_KNN_HEADER)
_CONSTANTS.update(_abi.constants(_KNN_HEADER))
globals().update({name[4:]: value for name, value in _CONSTANTS.items()})   # GCM_ACT_TANH -> ACT_TANH, ...
GCM_EUNSUPPORTED = _CONSTANTS["GCM_EUNSUPPORTED"]
DIR = {d: _CONSTANTS["GCM_DIR_" + d.upper()] for d in ("forward", "backward", "both")}


class SelectorDesc(ctypes.Structure):
    """struct gcm_selector_desc (include/gcm_hip.h)."""
    _fields_ = _abi.struct_fields(_HEADER, "gcm_selector_desc")


class HipLibraryError(RuntimeError):
    pass


def bind(handle, prototypes=PROTOTYPES, names=None):
    """Give the entry points `names` (default: all) of a ctypes library their restype / argtypes; -> handle."""
    for name in prototypes if names is None else names:
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = prototypes[name]
    return handle


def lib():
    """Load (once) and return the bound library; raises HipLibraryError if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise HipLibraryError(
                f"{_LIB_PATH} not found: build it with `python __graft_entry__.py` or "
                "`make -C graph-conv-memory_amd/csrc` (hipcc, --offload-arch=gfx950). "
                "This package has no CPU fallback."
            )
        # (GCM_HIP_LIB: a diagnostic build of the same library - csrc/Makefile `stamps*`, `exp` - for the
        #  dev tools under tools/; never set by the product)
        handle = bind(ctypes.CDLL(os.environ.get("GCM_HIP_LIB") or _LIB_PATH))
        bind(handle, AGGR_PROTOTYPES)
        bind(handle, LEARNED_DET_PROTOTYPES)
        bind(handle, TRANSFORMER_PROTOTYPES)
        bind(handle, RESET_PROTOTYPES)
        bind(handle, GIN_PROTOTYPES)
        bind(handle, GINE_PROTOTYPES)
        bind(handle, GATV2_PROTOTYPES)
        bind(handle, TRE_PROTOTYPES)
        bind(handle, BPTT_HOPS_PROTOTYPES)
        bind(handle, BPTT_HOPS_UNFOLDED_PROTOTYPES)
        bind(handle, RESGATED_PROTOTYPES)
        bind(handle, GATED_PROTOTYPES)
        bind(handle, TAG_PROTOTYPES)
        bind(handle, PNA_PROTOTYPES)
        bind(handle, RGCN_PROTOTYPES)
        bind(handle, GEN_PROTOTYPES)
        bind(handle, EDGECONV_PROTOTYPES)
        bind(handle, MP_PROTOTYPES)
        bind(handle, BRIDGE_PROTOTYPES)
        bind(handle, WINDOW_PROTOTYPES)
        bind(handle, SEGMENT_PROTOTYPES)
        bind(handle, HEAD_PROTOTYPES)
        bind(handle, KNN_PROTOTYPES)
        bind(handle, RUN_PROTOTYPES)
        bind(handle, RUN_HEAD_PROTOTYPES)
        bind(handle, RUN_MFMA_PROTOTYPES)
        got, want = handle.gcm_abi_version(), _CONSTANTS["GCM_ABI_VERSION"]
        if got != want:     # a library older than the header the prototypes were read from
            raise HipLibraryError(f"{_LIB_PATH} has ABI revision {got}, include/gcm_hip.h is at {want}: "
                                  "rebuild the library (`python __graft_entry__.py`)")
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().gcm_status_string(rc).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {rc})")


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    """Raw handle of the current HIP stream of the current device (what every kernel call takes).
    torch.cuda.current_stream() builds a Stream object per call (~2.5 us); this is the accessor
    underneath it."""
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def kernel_ready(t):
    """t as a kernel may read it: contiguous and with a 16-byte aligned data pointer (the kernels use 16-byte vector
    accesses).  A tensor that already is both comes back as the same object; any other - a strided or expanded view, a
    contiguous view that starts at an odd element of its storage - is copied into an allocation of its own, under
    autograd, so a gradient finds its way back to the view's base."""
    if t is None:
        return None
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def on_device(*tensors):
    """Validate that every given tensor lives on a HIP device and is contiguous."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise HipLibraryError(
                "gcm (MI355X build) runs on HIP devices only; got a tensor on "
                f"'{t.device}'. There is no CPU fallback."
            )
        if not t.is_contiguous():
            raise ValueError("gcm kernels need contiguous tensors")
        if t.device.index != torch.cuda.current_device():
            raise HipLibraryError(
                f"tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}: the "
                "kernels launch on the current device's stream - wrap the call in torch.cuda.device(...)")
