"""PyG's GATv2Conv (with edge_dim) and its dense twin on fused HIP kernels (csrc/gatv2conv.hip).

They live here and not in gcm.nn: gcm.nn is pinned to carry a `GATv2Conv` that raises NotImplementedError (the
placeholder of the time before these kernels; tests/test_gat_cpu.py and five more), and that stays as it is.  So

    from torch_geometric.nn import GATv2Conv      becomes      from gcm.gatv2 import GATv2Conv

The calling contract, the index and the plumbing are gcm.nn's.  gcm.gine.RelativeEdgeAttr makes the edge features a
memory has for free (time gap, pose offset): its out_channels is the edge_dim to give.
"""
import numbers

import torch

from . import _hip, _ops
from .nn import _dense_contract, _graph_of, _masked, _no_attention_dropout, _sparse_contract


def _gatv2_init(conv, in_channels, out_channels, heads, concat, negative_slope, dropout, edge_dim, fill_value, bias,
                share_weights):
    """Both layers' constructor: PyG's parameters and the refusals that need no input."""
    layer = type(conv).__name__
    if not isinstance(in_channels, int):
        raise NotImplementedError(f"{layer}: in_channels={in_channels!r}: bipartite (tuple) in_channels are not "
                                  "implemented")
    if dropout < 0 or dropout > 1:
        raise ValueError(f"{layer}: dropout must be in [0, 1]; got {dropout}")
    if isinstance(fill_value, bool) or not (fill_value == "mean" or isinstance(fill_value, numbers.Real)):
        raise NotImplementedError(f"{layer}: fill_value={fill_value!r} is not implemented: a number or 'mean'")
    conv.in_channels, conv.out_channels, conv.heads, conv.concat = in_channels, out_channels, heads, concat
    conv.negative_slope, conv.dropout, conv.edge_dim, conv.fill_value = negative_slope, dropout, edge_dim, fill_value
    conv.share_weights = share_weights
    conv.lin_l = torch.nn.Linear(in_channels, heads * out_channels, bias=bias)
    conv.lin_r = conv.lin_l if share_weights else torch.nn.Linear(in_channels, heads * out_channels, bias=bias)
    conv.att = torch.nn.Parameter(torch.empty(1, heads, out_channels))
    conv.lin_edge = torch.nn.Linear(edge_dim, heads * out_channels, bias=False) if edge_dim is not None else None
    conv.bias = torch.nn.Parameter(torch.empty(heads * out_channels if concat else out_channels)) if bias else None
    conv.reset_parameters()


def _gatv2_reset(conv):
    for lin in (conv.lin_l, conv.lin_r, conv.lin_edge):
        if lin is not None:
            torch.nn.init.xavier_uniform_(lin.weight)
            if lin.bias is not None:
                torch.nn.init.zeros_(lin.bias)
    bound = (6.0 / (conv.heads + conv.out_channels)) ** 0.5      # PyG's glorot on [.., H, C]
    torch.nn.init.uniform_(conv.att, -bound, bound)
    if conv.bias is not None:
        torch.nn.init.zeros_(conv.bias)


def _gatv2_check(conv):
    """Refused at every call, before the contract and before any launch: attention dropout while training, and widths
    beyond the kernels'."""
    layer = type(conv).__name__
    _no_attention_dropout(conv)
    if conv.in_channels > 128:
        raise ValueError(f"{layer}: in_channels={conv.in_channels}, the kernels take up to 128")
    if conv.heads * conv.out_channels > 128:
        raise ValueError(f"{layer}: heads * out_channels = {conv.heads * conv.out_channels}, the kernels take up to "
                         "128")
    if conv.edge_dim is not None and conv.edge_dim > _hip.GATV2_MAX_EDGE_DIM:
        raise ValueError(f"{layer}: edge_dim={conv.edge_dim}, the kernels take up to {_hip.GATV2_MAX_EDGE_DIM}")


def _gatv2_operands(conv):
    """(w_l, b_l, w_r, b_r, att, w_e, bias); w_r is None when lin_r is lin_l."""
    shared = conv.lin_r is conv.lin_l
    return (conv.lin_l.weight, conv.lin_l.bias, None if shared else conv.lin_r.weight,
            None if shared else conv.lin_r.bias, conv.att, None if conv.lin_edge is None else conv.lin_edge.weight,
            conv.bias)


def _gatv2_repr(conv):
    return f"{type(conv).__name__}({conv.in_channels}, {conv.out_channels}, heads={conv.heads})"


class DenseGATv2Conv(torch.nn.Module):
    """The dense twin of GATv2Conv, in DenseGATConv's conventions: adj[b,i,j] != 0 means i attends to j (only the
    pattern matters: weighted and negative entries give the same bits, and adj gets no gradient).  x [B,N,F], adj
    [B,N,N], edge_attr [B,N,N,D] with D = edge_dim; [N,F], [1,N,N] / [N,N] and [1,N,N,D] / [N,N,D] broadcast as in
    DenseGINEConv.  edge_attr is read at the set entries only (the others may hold anything, NaN included) and its
    gradient is zero elsewhere.  With add_loop the diagonal is a term whether or not adj has it set, and its edge
    feature is fill_value: the number, or ("mean") the mean of edge_attr over the row's set off-diagonal entries (zero
    when there are none).  With add_loop=False the diagonal is an ordinary entry.  A row with no term outputs bias; the
    output is multiplied by mask.  On a {0,1} adjacency this is GATv2Conv on DenseToSparse(transpose=True)'s list with
    add_self_loops = add_loop.  Without edge_dim edge_attr is accepted and ignored.  state_dict keys as GATv2Conv's:
    one loads into the other.  Forward and backward are HIP kernels (csrc/gatv2conv.hip) that write nothing per
    entry."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, edge_dim=None,
                 fill_value="mean", bias=True, share_weights=False):
        super().__init__()
        _gatv2_init(self, in_channels, out_channels, heads, concat, negative_slope, dropout, edge_dim, fill_value, bias,
                    share_weights)

    def reset_parameters(self):
        _gatv2_reset(self)

    def forward(self, x, adj, edge_attr=None, mask=None, add_loop=True):
        _gatv2_check(self)
        if self.edge_dim is None:
            x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
            edge_attr = None
        else:
            if edge_attr is None:
                raise ValueError(f"{type(self).__name__}: edge_attr is required with edge_dim={self.edge_dim}")
            x, adj, edge_attr = _dense_contract(self, x, adj, mask, self.in_channels, edge_attr=edge_attr,
                                                edge_attr_width=self.edge_dim)
        cfg = _ops.GATv2Config(self.heads, self.out_channels, self.concat, add_loop, self.fill_value,
                               self.negative_slope)
        w_l, b_l, w_r, b_r, att, w_e, bias = _gatv2_operands(self)
        out = _ops.dense_gatv2conv(x, adj, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr, cfg)
        return _masked(out, mask, x)

    def __repr__(self):
        return _gatv2_repr(self)


class GATv2Conv(torch.nn.Module):
    """PyG's GATv2Conv (flow source_to_target): x_l = lin_l(x), x_r = lin_r(x) viewed [M,H,C]; for an edge k = (j -> i)
    z_k = x_l[j] + x_r[i] (+ lin_edge(edge_attr[k])), score s_k[h] = sum_c att[h,c] leaky_relu(z_k[h,c]), alpha = the
    softmax of s over the in-edges of i (duplicates are separate terms), out_i[h] = sum_k alpha_k[h] x_l[j], heads
    concatenated (or averaged), + bias.  edge_index [2,E] = (source, sink), x [M,F], edge_attr [E,D] in edge_index
    order, D = edge_dim <= 32; F and heads * out_channels <= 128.  With add_self_loops every i -> i edge is skipped and
    each node gets one loop term after its edges, whose edge feature is fill_value: a number, broadcast over the D
    columns, or "mean", the mean of edge_attr over the node's remaining in-edges (zero when it has none).  A node
    without a term outputs bias.  Without edge_dim edge_attr is accepted and ignored, as GATConv does.  With
    share_weights lin_r is lin_l (both key sets are in the state_dict, parameters() yields the weight once).
    Forward and backward are HIP kernels (csrc/gatv2conv.hip): no per-edge array is written - not z, not
    lin_edge(edge_attr) [E,H*C], not the scores, not the messages; the backward recomputes them from x_l, x_r and the
    softmax's row maximum and sum; edge_attr is reached through the index's permutation.  Uses the
    `edge_index.gcm_graph` index SparseGCM attaches; any other edge list (unsorted ones too) is indexed here.
    Not implemented (NotImplementedError): residual=True, tuple in_channels, a fill_value other than a number or
    "mean", return_attention_weights, and attention dropout in training mode (eval mode runs)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
                 add_self_loops=True, edge_dim=None, fill_value="mean", bias=True, share_weights=False,
                 residual=False):
        super().__init__()
        if residual:
            raise NotImplementedError("GATv2Conv(residual=True) is not implemented")
        self.add_self_loops = add_self_loops
        _gatv2_init(self, in_channels, out_channels, heads, concat, negative_slope, dropout, edge_dim, fill_value, bias,
                    share_weights)

    def reset_parameters(self):
        _gatv2_reset(self)

    def forward(self, x, edge_index, edge_attr=None, return_attention_weights=None):
        if return_attention_weights is not None:
            raise NotImplementedError("GATv2Conv(return_attention_weights=...) is not implemented")
        _gatv2_check(self)
        if self.edge_dim is None:
            x, edge_index, _, _ = _sparse_contract(self, x, edge_index, self.in_channels, edge_attr=edge_attr)
            edge_attr = None
        else:
            if edge_attr is None:
                raise ValueError(f"GATv2Conv: edge_attr is required with edge_dim={self.edge_dim}")
            x, edge_index, _, _, edge_attr = _sparse_contract(self, x, edge_index, self.in_channels,
                                                              edge_attr=edge_attr, edge_attr_width=self.edge_dim)
        graph = _graph_of(x, edge_index, "GATv2Conv")
        cfg = _ops.GATv2Config(self.heads, self.out_channels, self.concat, self.add_self_loops, self.fill_value,
                               self.negative_slope)
        w_l, b_l, w_r, b_r, att, w_e, bias = _gatv2_operands(self)
        return _ops.csr_gatv2conv(x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr, graph, cfg)

    def __repr__(self):
        return _gatv2_repr(self)
