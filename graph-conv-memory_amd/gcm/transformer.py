"""PyG's TransformerConv with edge_dim and its dense twin on fused HIP kernels (csrc/transformer_edge.hip).

They live here and not in gcm.nn: gcm.nn.TransformerConv is pinned to raise NotImplementedError when given an edge_dim
(tests/test_transformer_cpu.py), and gcm.nn's classes and messages stay as they are.  So

    from torch_geometric.nn import TransformerConv      becomes      from gcm.transformer import TransformerConv

The calling contract, the index and the plumbing are gcm.nn's.  gcm.gine.RelativeEdgeAttr makes the edge features a
memory has for free (time gap, pose offset): its out_channels is the edge_dim to give.  Behind it the layer is attention
with a learned relative-position term in the score and in the message.  Without edge_dim both classes run gcm.nn's
kernels and give its bits.
"""
import torch

from . import _hip, _ops
from .nn import (_dense_contract, _graph_of, _masked, _no_attention_dropout, _sparse_contract, _transformer_operands,
                 _transformer_params)


def _init(conv, in_channels, out_channels, heads, concat, beta, dropout, edge_dim, bias, root_weight):
    """Both layers' constructor: PyG's parameters and the refusals that need no input."""
    layer = type(conv).__name__
    if not isinstance(in_channels, int):
        raise NotImplementedError(f"{layer}: in_channels={in_channels!r}: bipartite (tuple) in_channels are not "
                                  "implemented")
    _transformer_params(conv, in_channels, out_channels, heads, concat, beta, dropout, bias, root_weight)
    conv.edge_dim = edge_dim
    conv.lin_edge = torch.nn.Linear(edge_dim, heads * out_channels, bias=False) if edge_dim is not None else None
    conv.reset_parameters()


def _reset(conv):
    for lin in (conv.lin_key, conv.lin_query, conv.lin_value, conv.lin_edge, conv.lin_skip, conv.lin_beta):
        if lin is not None:
            lin.reset_parameters()


def _check(conv):
    """Refused at every call, before the contract and before any launch: attention dropout while training, and widths
    beyond the kernels'."""
    layer = type(conv).__name__
    _no_attention_dropout(conv)
    if conv.in_channels > 128:
        raise ValueError(f"{layer}: in_channels={conv.in_channels}, the kernels take up to 128")
    if conv.heads * conv.out_channels > 128:
        raise ValueError(f"{layer}: heads * out_channels = {conv.heads * conv.out_channels}, the kernels take up to "
                         "128")
    if conv.edge_dim is not None and conv.edge_dim > _hip.TRE_MAX_EDGE_DIM:
        raise ValueError(f"{layer}: edge_dim={conv.edge_dim}, the kernels take up to {_hip.TRE_MAX_EDGE_DIM}")


def _operands(conv):
    """(w_all [P,F], b_all [P], w_e [H*C,D] | None, w_beta [3 D] | None): gcm.nn's stacked projections and lin_edge's
    weight."""
    w_all, b_all, w_beta = _transformer_operands(conv)
    return w_all, b_all, (None if conv.lin_edge is None else conv.lin_edge.weight), w_beta


def _repr(conv):
    return f"{type(conv).__name__}({conv.in_channels}, {conv.out_channels}, heads={conv.heads})"


class DenseTransformerConv(torch.nn.Module):
    """The dense twin of TransformerConv, in gcm.nn.DenseTransformerConv's conventions: adj[b,i,j] != 0 means i attends
    to j (only the pattern matters: weighted and negative entries give the same bits, and adj gets no gradient).  x
    [B,N,F], adj [B,N,N], edge_attr [B,N,N,D] with D = edge_dim; [N,F], [1,N,N] / [N,N] and [1,N,N,D] / [N,N,D]
    broadcast as in DenseGINEConv.  edge_attr is read at the set entries only (the others may hold anything, NaN
    included) and its gradient is zero elsewhere.  With add_loop the diagonal is a term whether or not adj has it set,
    and its feature is edge_attr[b,i,i] (what RelativeEdgeAttr puts there: zero gap, zero offset); there is no
    fill_value, PyG's layer has none.  A row with no term aggregates nothing (o = 0); the output is multiplied by
    mask.  On a {0,1} adjacency with add_loop=False this is TransformerConv on DenseToSparse(transpose=True)'s list
    with edge_attr[b,i,j] gathered in that order.  Without edge_dim edge_attr is accepted and ignored and the layer is
    gcm.nn.DenseTransformerConv, bit for bit.  state_dict keys as TransformerConv's: one loads into the other.  Forward
    and backward are HIP kernels (csrc/transformer_edge.hip) that form nothing per entry wider than D."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None,
                 bias=True, root_weight=True):
        super().__init__()
        _init(self, in_channels, out_channels, heads, concat, beta, dropout, edge_dim, bias, root_weight)

    def reset_parameters(self):
        _reset(self)

    def forward(self, x, adj, edge_attr=None, mask=None, add_loop=False):
        _check(self)
        w_all, b_all, w_e, w_beta = _operands(self)
        if self.edge_dim is None:
            x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
            out = _ops.dense_transformerconv(x, adj.detach(), w_all, b_all, w_beta, self.heads, self.concat,
                                             self.root_weight, add_loop)
        else:
            if edge_attr is None:
                raise ValueError(f"{type(self).__name__}: edge_attr is required with edge_dim={self.edge_dim}")
            x, adj, edge_attr = _dense_contract(self, x, adj, mask, self.in_channels, edge_attr=edge_attr,
                                                edge_attr_width=self.edge_dim)
            out = _ops.dense_transformer_edge(x, adj, edge_attr, w_all, b_all, w_e, w_beta, self.heads, self.concat,
                                              self.root_weight, add_loop)
        return _masked(out, mask, x)

    def __repr__(self):
        return _repr(self)


class TransformerConv(torch.nn.Module):
    """PyG's TransformerConv (flow source_to_target) with edge_dim: q, k, v = lin_query(x), lin_key(x), lin_value(x)
    viewed [M,H,C]; for an edge k = (j -> i) with e_k = lin_edge(edge_attr[k]) viewed [H,C], the score is s_k[h] =
    <q_i[h], k_j[h] + e_k[h]> / sqrt(C), alpha = the softmax of s over the in-edges of i (duplicates are separate
    terms), o_i[h] = sum_k alpha_k[h] (v_j[h] + e_k[h]), heads concatenated (or averaged); skip and beta gate as
    gcm.nn.TransformerConv.  edge_index [2,E] = (source, sink), x [M,F], edge_attr [E,D] in edge_index order, D =
    edge_dim <= 32; F and heads * out_channels <= 128.  The edges are used as given: no loop is added or removed; a
    node with no in-edge has o = 0.  Without edge_dim edge_attr is accepted and ignored and the layer is
    gcm.nn.TransformerConv, bit for bit.  Forward and backward are HIP kernels (csrc/transformer_edge.hip): lin_edge is
    never applied per edge - not lin_edge(edge_attr) [E,H*C], not the keys k_j + e_k, not the messages v_j + e_k are
    written; per edge the kernels read the D features and add O(H D) work.  edge_attr is reached through the index's
    permutation.  Uses the `edge_index.gcm_graph` index SparseGCM attaches; any other edge list (unsorted ones too) is
    indexed here.  Not implemented (NotImplementedError): tuple in_channels, return_attention_weights, and attention
    dropout in training mode (eval mode runs)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None,
                 bias=True, root_weight=True):
        super().__init__()
        _init(self, in_channels, out_channels, heads, concat, beta, dropout, edge_dim, bias, root_weight)

    def reset_parameters(self):
        _reset(self)

    def forward(self, x, edge_index, edge_attr=None, return_attention_weights=None):
        if return_attention_weights is not None:
            raise NotImplementedError("TransformerConv(return_attention_weights=...) is not implemented")
        _check(self)
        w_all, b_all, w_e, w_beta = _operands(self)
        if self.edge_dim is None:
            x, edge_index, _, _ = _sparse_contract(self, x, edge_index, self.in_channels, edge_attr=edge_attr)
            graph = _graph_of(x, edge_index, "TransformerConv")
            return _ops.csr_transformerconv(x, w_all, b_all, w_beta, graph, self.heads, self.concat, self.root_weight)
        if edge_attr is None:
            raise ValueError(f"TransformerConv: edge_attr is required with edge_dim={self.edge_dim}")
        x, edge_index, _, _, edge_attr = _sparse_contract(self, x, edge_index, self.in_channels, edge_attr=edge_attr,
                                                          edge_attr_width=self.edge_dim)
        graph = _graph_of(x, edge_index, "TransformerConv")
        return _ops.csr_transformer_edge(x, edge_attr, w_all, b_all, w_e, w_beta, graph, self.heads, self.concat,
                                         self.root_weight)

    def __repr__(self):
        return _repr(self)
