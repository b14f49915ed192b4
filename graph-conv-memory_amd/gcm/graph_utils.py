"""What a layer written against gcm.nn.MessagePassing takes from torch_geometric.utils: softmax, scatter, degree,
add_self_loops, remove_self_loops (INTEGRATION.md lists them against their PyG names).  softmax and scatter run on the
HIP kernels of csrc/message_passing.hip (float32 device tensors, no CPU fallback); the other three are plain torch.

How the two find the CSR without a sort: MessagePassing.propagate hands `index` (the sink of each edge) to message /
aggregate with the GraphIndex attached as `index.gcm_graph`, the attribute SparseGCM uses on edge_index.  Any other
index is stably sorted here, which is what GraphIndex.from_edge_index does."""
import torch

from . import _hip, _ops

_REDUCE = ("sum", "add", "mean", "max", "min")


def _num_segments(index, num):
    if num is not None:
        return int(num)
    graph = getattr(index, "gcm_graph", None)
    if graph is not None and graph.E == index.numel():
        return graph.M
    return int(index.max()) + 1 if index.numel() else 0       # (one host read, as in PyG)


def _segments(src, index, num):
    """The segment list of `index` for the rows of src: the attached GraphIndex's when it fits, else a stable sort."""
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1:
        raise TypeError("index must be a 1-D torch.int64 tensor")
    if src.dtype != torch.float32:
        raise TypeError(f"the segment kernels are float32 only; got {src.dtype}")
    if src.dim() < 1 or src.shape[0] != index.numel():
        raise ValueError(f"src has {src.shape[0] if src.dim() else 0} rows along dim 0, index {index.numel()} entries")
    _hip.on_device(src, index)
    M = _num_segments(index, num)
    graph = getattr(index, "gcm_graph", None)
    if graph is not None and graph.mask is None and graph.E == index.numel() and graph.M == M:
        return _ops.Segments.by_sink(graph)
    return _ops.Segments.from_index(index, M)


def softmax(src, index, ptr=None, num_nodes=None, dim=0):
    """torch_geometric.utils.softmax: out[e] = exp(src[e]) / sum of exp(src) over the entries with index[e], per
    trailing element; src [E, ...].  Every (segment, element) is shifted by its own maximum, so logits of any size
    are exact.  PyG's 1e-16 in the denominator is not reproduced."""
    if dim != 0:
        raise NotImplementedError(f"softmax(dim={dim}) is not implemented: the entries run along dim 0")
    if ptr is not None:
        raise NotImplementedError("softmax(ptr=...) is not implemented: pass index")
    return _ops.mp_softmax(src, _segments(src, index, num_nodes))


def scatter(src, index, dim=0, dim_size=None, reduce="sum"):
    """torch_geometric.utils.scatter along dim 0: out[i] = reduce over the entries with index[e] == i of src[e];
    src [E, ...] -> [dim_size, ...].  A segment without entries gives 0 for every reduce; "mean" divides by
    max(count, 1); the gradient of "max" / "min" goes to ONE entry, the first of its segment in the caller's order on
    a tie (torch.scatter_reduce splits it among the ties)."""
    if dim != 0:
        raise NotImplementedError(f"scatter(dim={dim}) is not implemented: the entries run along dim 0")
    if reduce not in _REDUCE:
        raise NotImplementedError(f"reduce='{reduce}' is not implemented: one of {_REDUCE}")
    return _ops.mp_reduce(src, _segments(src, index, dim_size), reduce)


def degree(index, num_nodes=None, dtype=None):
    """torch_geometric.utils.degree: the number of entries of `index` per node, [num_nodes]."""
    dtype = torch.get_default_dtype() if dtype is None else dtype
    N = _num_segments(index, num_nodes)
    graph = getattr(index, "gcm_graph", None)
    if graph is not None and graph.E == index.numel() and graph.M == N:
        return (graph.row_ptr[1:] - graph.row_ptr[:-1]).to(dtype)
    out = torch.zeros(N, dtype=dtype, device=index.device)
    return out.scatter_add_(0, index, torch.ones(index.numel(), dtype=dtype, device=index.device))


def add_self_loops(edge_index, edge_attr=None, fill_value=None, num_nodes=None):
    """torch_geometric.utils.add_self_loops: (i, i) for every node appended after the given edges; fill_value (a
    float, default 1.0) fills their attributes.  The list returned is a new tensor: it carries no gcm_graph."""
    if fill_value is not None and (isinstance(fill_value, bool) or not isinstance(fill_value, (int, float))):
        raise NotImplementedError("fill_value must be a float or None (the reductions 'add', 'mean', ... and tensor "
                                  "values are not implemented)")
    N = int(num_nodes) if num_nodes is not None else (int(edge_index.max()) + 1 if edge_index.numel() else 0)
    loop = torch.arange(N, dtype=edge_index.dtype, device=edge_index.device)
    out = torch.cat([edge_index, loop.unsqueeze(0).expand(2, N)], dim=1)
    if edge_attr is not None:
        fill = 1.0 if fill_value is None else fill_value
        edge_attr = torch.cat([edge_attr, edge_attr.new_full((N,) + tuple(edge_attr.shape[1:]), fill)], dim=0)
    return out, edge_attr


def remove_self_loops(edge_index, edge_attr=None):
    """torch_geometric.utils.remove_self_loops: the edges with source != sink, in their order."""
    keep = edge_index[0] != edge_index[1]
    return edge_index[:, keep], None if edge_attr is None else edge_attr[keep]
