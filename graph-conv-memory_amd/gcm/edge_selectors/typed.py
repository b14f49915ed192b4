"""TypedEdge: a dense selector that remembers WHICH of its children selected an edge (not in the reference).

A memory built from several selectors ORs what they select into one `adj`: no layer can tell a temporal edge from a
spatial or a learned one.  TypedEdge runs its children side by side, merges their selections as Sequential would,
and records per entry the set of relations that selected it as a bit code in the memory's `weights` plane
(DenseGCM(edge_weights=True) carries it in the hidden state, rolls it on overflow and clears it on a reset).
gcm.nn.DenseRGCNConv reads that plane and applies one weight matrix per relation."""
import torch

from .. import _ops, util

MAX_RELATIONS = _ops.RGCN_MAX_RELATIONS


class TypedEdge(torch.nn.Module):
    """selectors: the children, dense selectors of plugin API #1; relations[k]: the relation index of child k
    (default k; two children may share one).  num_relations = max(relations) + 1, at most 16.

    forward(nodes, adj, weights, num_nodes, B) -> (adj, weights), `weights` of adj's shape: every child is called on
    a ZERO adjacency and a zero-size weights tensor, so a_k is exactly what child k selects at this step; then
        adj_out = util.diff_or([adj, a_0, ...])   in value and in gradient (values stay in {0, 1}; a LearnedEdge
                                                  child keeps its straight-through path),
        rel_out = weights | sum_k 2^relations[k] [a_k > 0]   (the codes of earlier steps stay as they are).
    One HIP launch (csrc/rgcnconv.hip, gcm_typed_merge) writes rel_out, and adj_out too when nothing involved
    requires a gradient; otherwise adj_out is diff_or in torch."""

    def __init__(self, selectors, relations=None):
        super().__init__()
        selectors = list(selectors)
        if not selectors:
            raise ValueError("TypedEdge needs at least one selector")
        relations = list(range(len(selectors))) if relations is None else [int(r) for r in relations]
        if len(relations) != len(selectors):
            raise ValueError(f"TypedEdge: {len(selectors)} selectors but {len(relations)} relations")
        if min(relations) < 0:
            raise ValueError("TypedEdge: relation indices must be >= 0")
        if max(relations) + 1 > MAX_RELATIONS or len(selectors) > MAX_RELATIONS:
            raise ValueError(f"TypedEdge: at most {MAX_RELATIONS} relations (the codes carry {MAX_RELATIONS} bits); "
                             f"got {max(max(relations) + 1, len(selectors))}")
        self.selectors = torch.nn.ModuleList(selectors)
        self.relations = relations

    @property
    def num_relations(self):
        return max(self.relations) + 1

    def forward(self, nodes, adj, weights, num_nodes, B):
        if weights.shape != adj.shape:
            raise ValueError(f"TypedEdge writes the relation codes into the memory's weights plane: weights must have "
                             f"adj's shape {list(adj.shape)}, got {list(weights.shape)} - build the memory with "
                             "DenseGCM(edge_weights=True)")
        no_weights = adj.new_zeros(0)
        picked = [child(nodes, torch.zeros_like(adj), no_weights, num_nodes, B)[0] for child in self.selectors]
        with_grad = torch.is_grad_enabled() and any(t.requires_grad for t in [adj] + picked)
        adj_out, rel_out = _ops.typed_merge(adj.detach(), weights.detach(), picked, self.relations, not with_grad)
        if with_grad:
            adj_out = util.diff_or([adj] + picked)
        return adj_out, rel_out

    def extra_repr(self):
        return f"relations={self.relations}"
