"""Edge-feature layers: PyG's GINEConv, its dense twin and the RelativeEdgeAttr transform (csrc/gineconv.hip).

They live here and not in gcm.nn: gcm.nn is pinned not to carry a `GINEConv` (tests/test_gin_cpu.py), so

    from torch_geometric.nn import GINEConv      becomes      from gcm.gine import GINEConv

The calling contract, the GIN plumbing and the index are gcm.nn's.
"""
import torch

from . import _hip, _ops
from .nn import (_dense_contract, _gin_init, _gin_reset, _graph_of, _masked, _ready_grad,  # noqa: F401
                 _sparse_contract)


def _gine_init(conv, nn, eps, train_eps, edge_dim):
    """PyG's GINEConv constructor: `lin` = Linear(edge_dim, in_channels) with in_channels read off nn (its first module
    when it is a Sequential): in_features, else in_channels."""
    conv.edge_dim = edge_dim
    if edge_dim is not None:
        first = nn[0] if isinstance(nn, torch.nn.Sequential) else nn
        if hasattr(first, "in_features"):
            in_channels = first.in_features
        elif hasattr(first, "in_channels"):
            in_channels = first.in_channels
        else:
            raise ValueError("Could not infer input channels from `nn`.")
        conv.lin = torch.nn.Linear(edge_dim, in_channels)
    else:
        conv.lin = None
    _gin_init(conv, nn, eps, train_eps)


def _gine_reset(conv):
    _gin_reset(conv.nn)
    conv.eps.data.fill_(conv.initial_eps)
    if conv.lin is not None:
        conv.lin.reset_parameters()


_GINE_MISMATCH = ("Node and edge feature dimensionalities do not match. Consider setting the 'edge_dim' attribute of "
                  "'GINEConv'")


def _gine_check(conv, x, edge_attr):
    """What is refused before the contract: no edge features, and widths beyond the kernels'."""
    layer = type(conv).__name__
    if edge_attr is None:
        raise ValueError(f"{layer}: edge_attr is required (GINConv is the layer without edge features)")
    if x.shape[-1] > 128:
        raise ValueError(f"{layer}: x has {x.shape[-1]} features, the kernels take up to 128")
    if conv.edge_dim is not None and conv.edge_dim > _hip.GINE_MAX_EDGE_DIM:
        raise ValueError(f"{layer}: edge_dim={conv.edge_dim}, the kernels take up to {_hip.GINE_MAX_EDGE_DIM}")


def _gine_lin(conv, F):
    """(in_channels of the contract, width of edge_attr, w_e, b_e)"""
    if conv.lin is None:
        return None, F, None, None
    return conv.lin.out_features, conv.edge_dim, conv.lin.weight, conv.lin.bias


class DenseGINEConv(torch.nn.Module):
    """The dense twin of GINEConv: h[b,i] = s x[b,i] + sum over j with adj[b,i,j] != 0 of adj[b,i,j] relu(x[b,j] +
    e[b,i,j]), s = 1 + eps when add_loop else 0; out = nn(h), times the mask.  e = lin(edge_attr) with edge_dim, else
    edge_attr itself (its width must be x's).  adj [B,N,N] float (adj[b,i,j]: i aggregates from j; values are weights,
    the diagonal is an ordinary entry), x [B,N,F], F <= 128, edge_attr [B,N,N,D], D = edge_dim <= 32; [N,F], [1,N,N] /
    [N,N] and [1,N,N,D] / [N,N,D] broadcast as in DenseGINConv.  On a {0,1} adjacency this is GINEConv on
    DenseToSparse(transpose=True)'s list.  When adj needs no gradient, edge_attr is read at the set entries only (the
    others may hold anything, NaN included).  When it does, its gradient is the true derivative at EVERY entry,
    g_adj[b,i,j] = <g_h[b,i], relu(x[b,j] + e[b,i,j])> (DenseResGatedGraphConv's rule: a LearnedEdge child stays
    trainable through the layer), and every entry of edge_attr is read and must be finite.  edge_attr's gradient is
    zero at unset entries.  The aggregation and its gradients are HIP kernels (csrc/gineconv.hip) that never write the
    projected edge features or the messages to memory; `nn` runs under torch autograd.  state_dict keys `eps`, `nn.*`,
    `lin.{weight,bias}` (with edge_dim), shared with GINEConv."""

    def __init__(self, nn, eps=0.0, train_eps=False, edge_dim=None):
        super().__init__()
        _gine_init(self, nn, eps, train_eps, edge_dim)

    def reset_parameters(self):
        _gine_reset(self)

    def forward(self, x, adj, edge_attr=None, mask=None, add_loop=True):
        _gine_check(self, x, edge_attr)
        in_channels, width, w_e, b_e = _gine_lin(self, x.shape[-1])
        x, adj, edge_attr = _dense_contract(self, x, adj, mask, in_channels, edge_attr=edge_attr,
                                            edge_attr_width=width, edge_attr_error=_GINE_MISMATCH)
        h = _ops.dense_gine_aggregate(x, adj, edge_attr, w_e, b_e, self.eps, add_loop)
        out = _ready_grad(self.nn(h))
        return _masked(out, mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}(nn={self.nn})"


class GINEConv(torch.nn.Module):
    """PyG's GINEConv (flow source_to_target): h_i = (1 + eps) x_i + sum over the edges k = (j -> i) of relu(x_j +
    e_k), out = nn(h); e_k = lin(edge_attr[k]) with edge_dim (lin = Linear(edge_dim, in_channels), in_channels read
    off nn as PyG does), else edge_attr[k] itself, whose width must then be x's.  edge_index [2,E] = (source, sink), x
    [M,F], F <= 128, edge_attr [E,D] in edge_index order, D = edge_dim <= 32.  The edges are used as given: self
    edges and duplicates are ordinary terms.  The aggregation and its gradients (x, edge_attr, eps, lin) are HIP kernels
    (csrc/gineconv.hip): neither lin(edge_attr) [E,F] nor the messages [E,F] are written to memory, the backward
    recomputes the ReLU's argument, and edge_attr is reached through the index's permutation instead of being copied
    into CSR order.  Uses the `edge_index.gcm_graph` index SparseGCM attaches; any other edge list is indexed here.
    `eps` [1] is a Parameter when train_eps, else a buffer; state_dict keys `eps`, `nn.*`, `lin.{weight,bias}`.
    gcm.gine.RelativeEdgeAttr makes the edge features a memory has for free."""

    def __init__(self, nn, eps=0.0, train_eps=False, edge_dim=None):
        super().__init__()
        _gine_init(self, nn, eps, train_eps, edge_dim)

    def reset_parameters(self):
        _gine_reset(self)

    def forward(self, x, edge_index, edge_attr=None):
        _gine_check(self, x, edge_attr)
        in_channels, width, w_e, b_e = _gine_lin(self, x.shape[-1])
        x, edge_index, _, _, edge_attr = _sparse_contract(self, x, edge_index, in_channels, edge_attr=edge_attr,
                                                          edge_attr_width=width, edge_attr_error=_GINE_MISMATCH)
        graph = _graph_of(x, edge_index, "GINEConv")
        return _ready_grad(self.nn(_ops.csr_gine_aggregate(x, edge_attr, w_e, b_e, self.eps, graph)))

    def __repr__(self):
        return f"{self.__class__.__name__}(nn={self.nn})"


class RelativeEdgeAttr(torch.nn.Module):
    """The edge features a memory has for free, for GINEConv / DenseGINEConv: the time gap and the pose offset of the
    two nodes of an edge.  out_channels = int(time) + (width of pose_slice) is what the layer takes as edge_dim.
    sparse: forward(x [M,F], edge_index [2,E]) -> [E, D] in edge_index order, row k = [(sink_k - source_k) *
    time_scale, x[source_k, ps] - x[sink_k, ps]].  A memory's node index is its insertion order and no edge leaves its
    graph, so the first column is the time gap in steps; it does not change under drop_oldest, wrap-around or the dense
    overflow roll, which move both ends alike.
    dense: forward(x [B,N,F], adj) -> [B,N,N,D], entry (b,i,j) = [(i - j) * time_scale, x[b,j,ps] - x[b,i,ps]] for every
    entry; adj is read for its shape only (adj[b,i,j]: i aggregates from j, so i is the sink).
    The gradient goes to x through the pose columns only: per node the sum over its CSC column minus the sum over its
    CSR row in index order (dense: column sums minus row sums), no atomics; with time alone the output needs none.
    Orientation: behind DenseToSparse() in its default (reference) orientation the rows of adj are the sources, so the
    time column has the opposite sign of the dense twin's; DenseToSparse(transpose=True) matches it.
    pose_slice must be contiguous; negative bounds resolve against F at call time."""

    def __init__(self, time=True, pose_slice=None, time_scale=1.0):
        super().__init__()
        if not time and pose_slice is None:
            raise ValueError("RelativeEdgeAttr: neither time nor pose_slice: there is nothing to emit")
        self.time, self.pose_slice, self.time_scale = bool(time), pose_slice, float(time_scale)
        P = 0
        if pose_slice is not None:
            if pose_slice.step not in (None, 1):
                raise NotImplementedError("pose slices must be contiguous")
            lo = 0 if pose_slice.start is None else pose_slice.start
            hi = pose_slice.stop
            if hi is None:
                if lo >= 0:
                    raise ValueError("RelativeEdgeAttr: the width of an open pose_slice is not known before x is")
                hi = 0
            elif (lo < 0) != (hi < 0):
                raise ValueError("RelativeEdgeAttr: the width of a pose_slice with bounds of both signs is not known "
                                 "before x is")
            P = max(hi - lo, 0)
        self.out_channels = int(self.time) + P

    def _range(self, F):
        if self.pose_slice is None:
            return 0, 0
        start, stop, _ = self.pose_slice.indices(F)
        if stop - start != self.out_channels - int(self.time):
            raise ValueError(f"RelativeEdgeAttr: pose_slice {self.pose_slice} takes {max(stop - start, 0)} of x's {F} "
                             f"features, out_channels says {self.out_channels - int(self.time)}")
        return start, stop - start

    def forward(self, x, edge_index_or_adj):
        if x.dim() == 2 and edge_index_or_adj.dtype == torch.int64 and edge_index_or_adj.shape[0] == 2:
            x, edge_index, _, _ = _sparse_contract(self, x, edge_index_or_adj)
            p0, P = self._range(x.shape[1])
            return _ops.rel_edge_attr(x, edge_index, lambda: _graph_of(x, edge_index), p0, P, int(self.time),
                                      self.time_scale)
        x, _ = _dense_contract(self, x, edge_index_or_adj)
        p0, P = self._range(x.shape[2])
        return _ops.dense_rel_edge_attr(x, p0, P, int(self.time), self.time_scale)

    def extra_repr(self):
        return f"time={self.time}, pose_slice={self.pose_slice}, time_scale={self.time_scale}"
