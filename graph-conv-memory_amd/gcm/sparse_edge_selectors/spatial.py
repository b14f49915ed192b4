"""Sparse spatial selectors (reference: src/gcm/sparse_edge_selectors/spatial.py:12-115).

Both keep the reference's constructors, attributes and forward(nodes, T, taus, B) -> torch.sparse_coo [B, N, N]
with indices (batch, sink, source) and unit values.  The reference runs a Python loop over the graphs around PyG's
knn / a pairwise distance; here a count kernel, one readback of the edge total and a fill kernel
(csrc/spatial.hip) emit the edges of the whole batch in coalesced order.  DESIGN.md §3.13 lists where the
semantics are pinned.
"""
from typing import List, Sequence, Union

import torch

from .. import _hip, _ops


def resolve_columns(position_slice: Union[slice, Sequence[int]], F: int) -> List[int]:
    """The node-feature columns `nodes[..., position_slice]` selects, as a host list: any slice (step and negative
    bounds included, resolved with slice.indices(F)) or a sequence of int columns (negative ones count from the
    end, as in indexing)."""
    if isinstance(position_slice, slice):
        return list(range(*position_slice.indices(F)))
    if isinstance(position_slice, torch.Tensor):
        position_slice = position_slice.tolist()
    if isinstance(position_slice, int):
        position_slice = [position_slice]
    cols = []
    for c in position_slice:
        c = int(c)
        if not -F <= c < F:
            raise IndexError(f"position column {c} is out of range for {F} node features")
        cols.append(c % F)
    return cols


def _coo(idx, edge_off, nodes, B):
    N = nodes.shape[1]
    vals = torch.ones(idx.shape[1], device=idx.device)
    out = torch.sparse_coo_tensor(idx, vals, size=(B, N, N), is_coalesced=True)
    out.gcm_bptr = edge_off      # edges of each graph [B+1]
    return out


class SpatialKNNEdge(torch.nn.Module):
    """For every new node i of graph b (i in [T_b, T_b + tau_b)) take its k nearest nodes, by squared Euclidean
    distance over the position columns, among ALL of [0, T_b + tau_b) - i itself and the later new nodes of the
    same call included, as the reference's knn(source, sink, k) - and keep the edges (b, sink i, source j) with
    j < i.  Equal distances go to the lower source index (PyG leaves the order of ties unspecified).

    One deliberate deviation: the reference stacks the LOCAL sink index (0 .. tau_b - 1) into the COO and filters
    it against absolute source indices (spatial.py:53-56).  That is right only at T_b = 0; for T_b > 0 its edges
    land in old nodes' rows and a stepwise caller (tau = 1) gets none.  Here the sink is T_b + local index and the
    filter is source < sink, which equals the reference exactly whenever T_b = 0.

    causal=False raises NotImplementedError, as in the reference."""

    def __init__(self, position_slice, k, causal=True):
        # In meters
        super().__init__()
        self.k = k
        self.position_slice = position_slice
        self.causal = causal

    new_sinks_only = True   # every edge ends in a NEW node: SparseGCM merges without a sort

    def forward(self, nodes, T, taus, B):
        if not self.causal:
            raise NotImplementedError()
        if int(self.k) < 1:
            raise ValueError(f"SpatialKNNEdge needs k >= 1, got {self.k}")
        cols = resolve_columns(self.position_slice, nodes.shape[-1])
        idx, edge_off = _ops.spatial_edges(nodes, T, taus, cols, _hip.SPATIAL_KNN, k=int(self.k))
        return _coo(idx, edge_off, nodes, B)


class SpatialRadiusEdge(torch.nn.Module):
    """causal=True: the edge (b, sink i, source j) for every new node i and every j < i whose positions lie closer
    than `radius`: sqrt(sum_p (pos_i,p - pos_j,p)^2) < radius in fp32 (strict; the reference's formula, the sum in
    column order, correctly rounded sqrt).

    causal=False (spatial.py:95-97): the edge (b, sink j, source i) for every node j in [0, T_b + tau_b) and every
    new node i within the radius, self edges included.  Those sinks are old nodes and the self edges have
    source == sink, so this mode is for standalone use: inside SparseGCM it fails the causality check
    ("Causality violated", sparse_gcm.py:171) as the reference does."""

    def __init__(self, position_slice, radius=0.25, causal=True):
        # In meters
        super().__init__()
        self.radius = radius
        self.position_slice = position_slice
        self.causal = causal

    @property
    def new_sinks_only(self):
        """causal: every edge ends in a NEW node (SparseGCM merges without a sort); non-causal sinks are any node"""
        return bool(self.causal)

    def forward(self, nodes, T, taus, B):
        cols = resolve_columns(self.position_slice, nodes.shape[-1])
        mode = _hip.SPATIAL_RADIUS_CAUSAL if self.causal else _hip.SPATIAL_RADIUS_ALL
        idx, edge_off = _ops.spatial_edges(nodes, T, taus, cols, mode, radius=float(self.radius))
        return _coo(idx, edge_off, nodes, B)
