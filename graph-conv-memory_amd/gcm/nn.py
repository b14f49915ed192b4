"""GNN building blocks the reference takes from torch_geometric (not vendored
by the reference; call sites README.md:52-62, tests/test_gcm.py:95-99,249-256,
tests/test_sparse_gcm.py:310-323).  Parameter names/layout follow modern PyG
(`lin_rel.{weight,bias}`, `lin_root.weight`) so state_dicts interchange between
the dense and sparse layers (tests/test_sparse_gcm.py:326-330).
"""
import itertools

import torch

from . import _hip, _ops

_FUSABLE = {torch.nn.Tanh: _hip.ACT_TANH, torch.nn.ReLU: _hip.ACT_RELU}


class SkinnyLinear(torch.nn.Linear):
    """torch.nn.Linear (same parameters, same state_dict keys) for inputs with very many rows and
    <= 64 features in and out - the layers of LearnedEdge's default edge network (learned.py:38-51).
    Forward and input gradient are gcm_rows_linear (csrc/rows_linear.hip); the weight gradient runs as
    the row-split kernel gcm_skinny_wgrad.  Anything else (CPU tensors, wide layers, few rows, other dtypes)
    behaves exactly like nn.Linear."""

    MIN_ROWS = 2048

    def forward(self, x):
        if (x.is_cuda and x.dtype == torch.float32 and self.in_features <= 64 and self.out_features <= 64
                and x.numel() // self.in_features >= self.MIN_ROWS and torch.is_grad_enabled()
                and (self.weight.requires_grad or (self.bias is not None and self.bias.requires_grad))):
            return _ops.skinny_linear(x, self.weight, self.bias)
        return super().forward(x)


_AGGRS = ("add", "mean", "max")


_F32, _I64 = (torch.float32,), (torch.int64,)
_MASK_DTYPES = (torch.bool, torch.float32)
_CODE_DTYPES = (torch.float32, torch.int64)      # RGCN's relation codes


def _state(conv):
    """[(name, tensor)] over the parameters and buffers of a layer (walked once per call)."""
    return list(itertools.chain(conv.named_parameters(), conv.named_buffers()))


def _check_dtypes(layer, state, operands):
    """Step 1 of the calling contract.  operands: (name, tensor | None, accepted dtypes).  Nothing is cast: a float64
    pipeline would lose its precision without a word, and a narrower type would be read past its end."""
    for name, t, dtypes in operands:
        if t is not None and t.dtype not in dtypes:
            want = " or ".join(str(d).replace("torch.", "") for d in dtypes)
            raise TypeError(f"{layer}: {name} must be {want}; got {t.dtype}")
    for name, p in state:
        if p.is_floating_point() and p.dtype != torch.float32:
            raise TypeError(f"{layer}: parameter {name} must be float32; got {p.dtype} (the kernels are float32: "
                            "module.double() / .half() are not supported)")


def _check_devices(layer, state, operands):
    """Step 3 of the calling contract: every operand, then every parameter and buffer, on the current HIP device."""
    tensors = [(name, t) for name, t, _ in operands if t is not None]
    tensors += [("parameter " + name, p) for name, p in state]
    for name, t in tensors:
        if not t.is_cuda:
            raise _hip.HipLibraryError(f"{layer}: {name} is on '{t.device}': gcm (MI355X build) runs on HIP devices "
                                       "only. There is no CPU fallback.")
    cur = torch.cuda.current_device()
    for name, t in tensors:
        if t.device.index != cur:
            raise _hip.HipLibraryError(f"{layer}: {name} is on {t.device} but the current device is cuda:{cur}: the "
                                       "kernels launch on the current device's stream - wrap the call in "
                                       "torch.cuda.device(...)")


def _check_width(layer, F, in_channels, max_channels, width_error):
    """x of F features beside the layer's in_channels (`width_error(F)`: a layer's own wording of the mismatch), or
    beside GatedGraphConv's rule, in PyG's words: any width up to out_channels."""
    if in_channels is not None and F != in_channels:
        raise ValueError(f"{layer}: " + (width_error(F) if width_error else
                                         f"x has {F} features, the layer has in_channels={in_channels}"))
    if max_channels is not None and F > max_channels:
        raise ValueError(f"{layer}: The number of input channels is not allowed to be larger than the number of "
                         "output channels")


def _check_edge_attr(layer, edge_attr, lead, width, width_error):
    """edge_attr of a layer that reads it (`edge_attr_width`): `lead` = the accepted leading shapes, then `width`
    features."""
    s = tuple(edge_attr.shape)
    if len(s) < 2 or s[:-1] not in lead:
        want = " or ".join(str(list(l) + ["D"]).replace("'", "") for l in lead)
        raise ValueError(f"{layer}: edge_attr must be {want}; got {list(s)}")
    if s[-1] != width:
        raise ValueError(width_error or f"{layer}: edge_attr has {s[-1]} features, the layer has edge_dim={width}")


def _dense_contract(conv, x, adj, mask=None, in_channels=None, planes=(), device=True, width_error=None,
                    max_channels=None, edge_attr=None, edge_attr_width=None, edge_attr_error=None):
    """The calling contract of the dense layers, checked before anything else runs -> (x [B,N,F], adj [B,N,N], *planes
    [B,N,N]) as the kernels read them.  With `edge_attr_width` (a layer that reads edge features: DenseGINEConv),
    edge_attr [B,N,N,D], [1,N,N,D] or [N,N,D] with D == edge_attr_width is checked and made ready like adj and comes
    back last (`edge_attr_error`: the layer's own wording of a wrong D).  In this order, so that the first two fail alike on a machine without a GPU:
    1. dtype (TypeError): x, adj and every floating parameter and buffer float32, mask bool or float32, `planes`
       ((name, tensor) pairs of adj's shape: RGCN's relation codes) float32 or int64.  Nothing is cast.
    2. shape (ValueError): x [B,N,F] or [N,F], F == in_channels or F <= max_channels when one is given; adj and the
       planes [B,N,N], [1,N,N] or [N,N]; mask with B * N elements.
    3. device (_hip.HipLibraryError): every operand and every parameter and buffer on the current HIP device.
    4. layout: any strides go, zero strides of an expand included.  What comes back is contiguous and 16-byte aligned
       (_hip.kernel_ready): a copy where the operand was not, the operand itself where it was; a broadcast adjacency is
       materialised per batch entry.  The copies are made under autograd.  The mask is not copied (_masked reshapes it).
    Not checked: the alignment of the parameters (a misaligned view assigned as a module's parameter is handed to the
    kernels as it is).  `device=False` skips step 3 alone (the CPU tests of steps 1, 2 and 4)."""
    layer = type(conv).__name__
    planes = list(planes)
    operands = [("x", x, _F32), ("adj", adj, _F32), ("mask", mask, _MASK_DTYPES)]
    operands += [(name, t, _CODE_DTYPES) for name, t in planes]
    if edge_attr_width is not None:
        operands.append(("edge_attr", edge_attr, _F32))
    state = _state(conv)
    _check_dtypes(layer, state, operands)
    xs = tuple(x.shape)
    if len(xs) not in (2, 3):
        raise ValueError(f"{layer}: x must be [B,N,F] or [N,F]; got {list(xs)}")
    _check_width(layer, xs[-1], in_channels, max_channels, width_error)
    B, N = (1, xs[0]) if len(xs) == 2 else xs[:2]
    for name, t in [("adj", adj)] + planes:
        s = tuple(t.shape)
        if len(s) not in (2, 3) or s[-2:] != (N, N) or (len(s) == 3 and s[0] not in (1, B)):
            raise ValueError(f"{layer}: {name} must be [{B},{N},{N}], [1,{N},{N}] or [{N},{N}] beside x {list(xs)}; "
                             f"got {list(s)}")
    if mask is not None and mask.numel() != B * N:
        raise ValueError(f"{layer}: mask must hold B * N = {B * N} entries; got {list(mask.shape)}")
    if edge_attr_width is not None:
        _check_edge_attr(layer, edge_attr, [(B, N, N), (1, N, N), (N, N)], edge_attr_width, edge_attr_error)
    if device:
        _check_devices(layer, state, operands)
    out = [_hip.kernel_ready(x.unsqueeze(0) if len(xs) == 2 else x)]
    for _, t in [("adj", adj)] + planes:
        t = t.unsqueeze(0) if t.dim() == 2 else t
        out.append(_hip.kernel_ready(t.expand(B, -1, -1) if t.shape[0] != B else t))
    if edge_attr_width is not None:
        t = edge_attr.unsqueeze(0) if edge_attr.dim() == 3 else edge_attr
        out.append(_hip.kernel_ready(t.expand(B, -1, -1, -1) if t.shape[0] != B else t))
    return out


def _sparse_contract(conv, x, edge_index, in_channels=None, edge_weight=None, edge_attr=None, edge_type=None,
                     type_dtypes=_I64, device=True, width_error=None, weight_per_edge=False, max_channels=None,
                     edge_attr_width=None, edge_attr_error=None):
    """The calling contract of the sparse layers, checked before anything else runs -> (x [M,F], edge_index [2,E],
    edge_weight, edge_type) as the kernels and the indexing read them.  Steps and order as _dense_contract:
    1. dtype (TypeError): x, edge_weight, edge_attr and every floating parameter and buffer float32; edge_index
       int64, as in PyG; edge_type one of `type_dtypes`.  Nothing is cast.
    2. shape (ValueError): x [M,F], F == in_channels or F <= max_channels when one is given; edge_index [2,E].  The
       length of edge_weight / edge_type stays each layer's own rule: GraphConv and its relatives ignore a weight
       vector of another length, GCNConv (`weight_per_edge`) refuses it here.
    3. device (_hip.HipLibraryError): every operand and every parameter and buffer on the current HIP device.
    4. layout: any strides go (`pairs.t()` of an [E,2] list, a slice of a wider buffer).  What comes back is
       contiguous and 16-byte aligned (_hip.kernel_ready): a copy where the operand was not, the operand itself where
       it was.  An edge_index that carries a `gcm_graph` for these M nodes comes back as it is: the index is the
       library's own and the list is not read again.  edge_attr is ignored and not copied by every layer but one
       that reads edge features and says so with `edge_attr_width` (GINEConv): then edge_attr must be [E,D] with D ==
       edge_attr_width (step 2; `edge_attr_error`: the layer's own wording of a wrong D), is made ready like x and
       comes back as a fifth value.
    Not checked: node ids in edge_index outside [0, M) (finding them takes a pass over the list and a device
    synchronisation), and the alignment of the parameters.  `device=False` skips step 3 alone."""
    layer = type(conv).__name__
    operands = [("x", x, _F32), ("edge_index", edge_index, _I64), ("edge_weight", edge_weight, _F32),
                ("edge_attr", edge_attr, _F32), ("edge_type", edge_type, type_dtypes)]
    state = _state(conv)
    _check_dtypes(layer, state, operands)
    xs, es = tuple(x.shape), tuple(edge_index.shape)
    if len(xs) != 2:
        raise ValueError(f"{layer}: x must be [M,F]; got {list(xs)}")
    _check_width(layer, xs[1], in_channels, max_channels, width_error)
    if len(es) != 2 or es[0] != 2:
        raise ValueError(f"{layer}: edge_index must be [2,E] = (source, sink); got {list(es)}")
    if weight_per_edge and edge_weight is not None and edge_weight.numel() != es[1]:
        raise ValueError(f"{layer}: edge_weight has {edge_weight.numel()} entries for {es[1]} edges")
    if edge_attr_width is not None:
        _check_edge_attr(layer, edge_attr, [(es[1],)], edge_attr_width, edge_attr_error)
    if device:
        _check_devices(layer, state, operands)
    graph = getattr(edge_index, "gcm_graph", None)
    if graph is None or graph.M != xs[0]:
        edge_index = _hip.kernel_ready(edge_index)
    w = _hip.kernel_ready(edge_weight)
    if w is not edge_weight and getattr(edge_weight, "gcm_unit_weights", False):
        w.gcm_unit_weights = True
    out = _hip.kernel_ready(x), edge_index, w, _hip.kernel_ready(edge_type)
    return out if edge_attr_width is None else out + (_hip.kernel_ready(edge_attr),)


def _ready_grad(out):
    """Behind the torch modules that end a layer (GINConv's nn, GENConv's mlp, PNAConv's deeper post layers): the
    output's gradient reaches their backward contiguous and aligned too, as the conv Functions make it in theirs
    (_hip.kernel_ready; a contiguous one passes untouched).  Without it a transposed or zero-stride grad_output - the
    latter is what out.sum().backward() produces - takes another path through torch's GEMMs, and the layer's gradients
    would depend on how its caller laid grad_output out."""
    if out.requires_grad:
        out.register_hook(_hip.kernel_ready)
    return out


def _masked(out, mask, x):
    return out if mask is None else out * mask.reshape(x.shape[0], x.shape[1], 1).to(x.dtype)


def _graph_of(x, edge_index, layer=None):
    """The index SparseGCM attached (`edge_index.gcm_graph`) when it fits x, else one built here on the device.
    With `layer` named, a masked index is refused."""
    graph = getattr(edge_index, "gcm_graph", None)
    if graph is None or graph.M != x.shape[0]:
        graph = _ops.GraphIndex.from_edge_index(edge_index, x.shape[0])
    if layer is not None and graph.mask is not None:
        raise ValueError(f"{layer} does not take a masked GraphIndex (k-hop subgraphs reach it relabelled)")
    return graph


def _csr_weights(edge_weight, graph):
    """GraphConv's rules for edge weights, in CSR order.  PyG: a weight vector of the wrong length is ignored.  Unit
    weights without a gradient (what SparseGCM passes unless a learned selector is in play: sparse_gcm.py:160-164)
    multiply by exactly 1: the kernels then skip the weight loads altogether."""
    w = edge_weight
    if w is not None and (w.numel() != graph.E or getattr(w, "gcm_unit_weights", False)):
        return None
    if w is not None and graph.csr_perm is not None:
        w = w[graph.csr_perm]
    return w


def _no_attention_dropout(conv):
    if conv.training and conv.dropout > 0:
        raise NotImplementedError("attention dropout is not implemented: use dropout=0 or eval mode")


def _dense_aggr(conv, x, adj, mask, w_rel, w_root, bias, aggr):
    """The mean / max form of DenseGraphConv and DenseSAGEConv (csrc/aggrconv.hip).  Max reads only the
    pattern of adj, which then gets no gradient."""
    x, adj = _dense_contract(conv, x, adj, mask, conv.in_channels)
    out = _ops.dense_aggrconv(x, adj.detach() if aggr == "max" else adj, w_rel, w_root, bias, aggr)
    return _masked(out, mask, x)


def _sparse_aggr(conv, x, edge_index, edge_weight, w_rel, w_root, bias, aggr, name):
    """The mean / max form of GraphConv and SAGEConv (csrc/aggrconv.hip)."""
    x, edge_index, edge_weight, _ = _sparse_contract(conv, x, edge_index, conv.in_channels, edge_weight=edge_weight)
    graph = _graph_of(x, edge_index, name)
    w = _csr_weights(edge_weight, graph)
    return _ops.csr_aggrconv(x, w, w_rel, w_root, bias, graph, aggr)


class DenseGraphConv(torch.nn.Module):
    """out = lin_rel(agg) + lin_root(x), adj [B,N,N] float (adj[b,i,j]: i aggregates from j), x [B,N,F].
    aggr="add": agg = adj @ x, one fused fp32-MFMA kernel (csrc/graphconv.hip).
    aggr="mean": agg_i = (adj @ x)_i / clamp(rowsum(adj)_i, min=1); adj values are weights and get a gradient.
    aggr="max": agg_ic = max of x_jc over {j: adj_ij != 0}, 0 for an empty row; only the pattern of adj is
    read and adj gets no gradient.  Mean and max run in csrc/aggrconv.hip; the fused DenseGCM / Sequential
    paths apply to aggr="add" only."""

    def __init__(self, in_channels, out_channels, aggr="add", bias=True):
        super().__init__()
        if aggr not in _AGGRS:
            raise NotImplementedError(f"aggr='{aggr}' is not implemented: one of {_AGGRS}")
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        self.lin_rel = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_rel.reset_parameters()
        self.lin_root.reset_parameters()

    def forward(self, x, adj, mask=None, _act=_hip.ACT_NONE):
        if self.aggr != "add":
            if _act != _hip.ACT_NONE:
                raise ValueError("activation fusion is available for aggr='add' only")
            return _dense_aggr(self, x, adj, mask, self.lin_rel.weight, self.lin_root.weight, self.lin_rel.bias,
                               self.aggr)
        x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
        if mask is not None and _act != _hip.ACT_NONE:
            raise ValueError("activation fusion is not available together with a mask")
        out = _ops.dense_graphconv(x, adj, self.lin_rel.weight, self.lin_rel.bias,
                                   self.lin_root.weight, _act)
        return _masked(out, mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"


class GraphConv(torch.nn.Module):
    """out[i] = lin_rel(sum_{(j->i)} w_ji * x_j) + lin_root(x_i);  edge_index [2,E] = (source,
    sink), x [M,F].  The neighbour reduction is a CSR gather fused with the two linears on
    the matrix cores (csrc/graphconv.hip, k_csr_graphconv_fwd).  When SparseGCM built the
    edge list it attaches a ready CSR (`edge_index.gcm_graph`); any other edge_index is
    indexed here on the device.
    aggr="mean": the weighted sum divided by the number of edges into i (not by the weight sum).
    aggr="max": per channel the largest w_ji * x_j; the gradient goes to the winning edge, the first in CSR
    order on a tie; duplicate edges compete separately.  A node without an in-edge aggregates 0.  Mean and max
    run in csrc/aggrconv.hip; SparseGCM's one-call and masked k-hop paths apply to aggr="add" only."""

    def __init__(self, in_channels, out_channels, aggr="add", bias=True):
        super().__init__()
        if aggr not in _AGGRS:
            raise NotImplementedError(f"aggr='{aggr}' is not implemented: one of {_AGGRS}")
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        self.lin_rel = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_rel.reset_parameters()
        self.lin_root.reset_parameters()

    def forward(self, x, edge_index, edge_weight=None, _act=_hip.ACT_NONE):
        if self.aggr != "add":
            if _act != _hip.ACT_NONE:
                raise ValueError("activation fusion is available for aggr='add' only")
            return _sparse_aggr(self, x, edge_index, edge_weight, self.lin_rel.weight, self.lin_root.weight,
                                self.lin_rel.bias, self.aggr, "GraphConv(aggr='%s')" % self.aggr)
        x, edge_index, edge_weight, _ = _sparse_contract(self, x, edge_index, self.in_channels, edge_weight=edge_weight)
        graph = _graph_of(x, edge_index)
        w = _csr_weights(edge_weight, graph)
        return _ops.csr_graphconv(x, w, self.lin_rel.weight, self.lin_rel.bias,
                                  self.lin_root.weight, graph, _act)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"


class SAGEConv(torch.nn.Module):
    """PyG's SAGEConv (flow source_to_target): out_i = lin_l(aggr_{j -> i} x_j) + lin_r(x_i), edge_index [2,E] =
    (source, sink), x [M,F]; aggr "mean" or "max"; no edge weights.  Parameters as PyG 2.x: `lin_l.{weight,bias}`
    on the aggregate, `lin_r.weight` (absent with root_weight=False).  The same kernels as
    GraphConv(aggr=...) (csrc/aggrconv.hip).  Not implemented (NotImplementedError): normalize, project, other
    aggregations.  Not a GraphConv: SparseGCM runs a SAGE stack through its generic path."""

    def __init__(self, in_channels, out_channels, aggr="mean", normalize=False, root_weight=True, project=False,
                 bias=True):
        super().__init__()
        if aggr not in ("mean", "max"):
            raise NotImplementedError(f"SAGEConv(aggr='{aggr}') is not implemented: 'mean' or 'max'")
        if normalize:
            raise NotImplementedError("SAGEConv(normalize=True) is not implemented")
        if project:
            raise NotImplementedError("SAGEConv(project=True) is not implemented")
        self.in_channels, self.out_channels, self.aggr = in_channels, out_channels, aggr
        self.normalize, self.root_weight, self.project = normalize, root_weight, project
        self.lin_l = torch.nn.Linear(in_channels, out_channels, bias=bias)
        if root_weight:
            self.lin_r = torch.nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        if self.root_weight:
            self.lin_r.reset_parameters()

    def forward(self, x, edge_index):
        return _sparse_aggr(self, x, edge_index, None, self.lin_l.weight,
                            self.lin_r.weight if self.root_weight else None, self.lin_l.bias, self.aggr, "SAGEConv")

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, aggr={self.aggr})"


class DenseSAGEConv(torch.nn.Module):
    """PyG's DenseSAGEConv (mean only): out = lin_rel(adj @ x / clamp(rowsum(adj), min=1)) + lin_root(x), * mask;
    adj [B,N,N] float (adj[b,i,j]: i aggregates from j; values are weights and get a gradient), x [B,N,F].
    Parameters as PyG 2.x: `lin_rel.weight` (no bias), `lin_root.{weight,bias}`.  The same kernels as
    DenseGraphConv(aggr="mean") (csrc/aggrconv.hip).  normalize=True raises NotImplementedError.  Not a
    DenseGraphConv: DenseGCM runs a SAGE stack through its layered path."""

    def __init__(self, in_channels, out_channels, normalize=False, bias=True):
        super().__init__()
        if normalize:
            raise NotImplementedError("DenseSAGEConv(normalize=True) is not implemented")
        self.in_channels, self.out_channels, self.normalize = in_channels, out_channels, normalize
        self.lin_rel = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=bias)

    def reset_parameters(self):
        self.lin_rel.reset_parameters()
        self.lin_root.reset_parameters()

    def forward(self, x, adj, mask=None):
        return _dense_aggr(self, x, adj, mask, self.lin_rel.weight, self.lin_root.weight, self.lin_root.bias, "mean")

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"


def _glorot_zero(lin, bias):
    torch.nn.init.xavier_uniform_(lin.weight)
    if bias is not None:
        torch.nn.init.zeros_(bias)


class DenseGCNConv(torch.nn.Module):
    """PyG's DenseGCNConv: A = adj with the diagonal set to 1 (2 if improved) when add_loop,
    d = clamp(rowsum(A), min=1)^-1/2, out = d_i * sum_j A_ij d_j (x W^T)_j + bias; adj [B,N,N] float
    (adj[b,i,j]: edge j -> i), x [B,N,F].  Forward and backward are HIP kernels (csrc/gcnconv.hip).
    Parameters `lin.weight`, `bias` as in PyG 2.x; GCNConv loads the same state_dict.  Not a
    DenseGraphConv: the fused GraphConv paths of Sequential and DenseGCM do not apply to it."""

    def __init__(self, in_channels, out_channels, improved=False, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.improved = in_channels, out_channels, improved
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        _glorot_zero(self.lin, self.bias)

    def forward(self, x, adj, mask=None, add_loop=True):
        x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
        out = _ops.dense_gcnconv(x, adj, self.lin.weight, self.bias, add_loop, 2.0 if self.improved else 1.0)
        return _masked(out, mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"


class GCNConv(torch.nn.Module):
    """PyG's GCNConv (flow source_to_target): edge_index [2,E] = (source, sink), x [M,F].  With
    normalize, gcn_norm: add_remaining_self_loops (fill 2 if improved, else 1; an existing loop keeps
    its weight), in-degree, deg^-1/2 with inf -> 0; then out = A~ (x W^T) + bias.  The normalisation
    and the CSR aggregation fused with the linear are HIP kernels (csrc/gcnconv.hip).  Uses the
    `edge_index.gcm_graph` index SparseGCM attaches; any other edge list is indexed here.  Not a
    GraphConv: SparseGCM runs a GCN stack through its generic path."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True,
                 normalize=True, bias=True):
        super().__init__()
        if cached:
            raise NotImplementedError("cached=True is not implemented: every GCM call builds a new graph")
        self.in_channels, self.out_channels, self.improved = in_channels, out_channels, improved
        self.cached, self.add_self_loops, self.normalize = cached, add_self_loops, normalize
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        _glorot_zero(self.lin, self.bias)

    def forward(self, x, edge_index, edge_weight=None):
        x, edge_index, w, _ = _sparse_contract(self, x, edge_index, self.in_channels, edge_weight=edge_weight,
                                               weight_per_edge=True)
        graph = _graph_of(x, edge_index, "GCNConv")
        w = _csr_weights(w, graph)     # unit weights without a gradient: the kernels count 1 per edge
        return _ops.csr_gcnconv(x, w, self.lin.weight, self.bias, graph, self.normalize,
                                self.add_self_loops, 2.0 if self.improved else 1.0)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"


def _gin_init(conv, nn, eps, train_eps):
    conv.nn, conv.initial_eps = nn, float(eps)
    if train_eps:
        conv.eps = torch.nn.Parameter(torch.empty(1))
    else:
        conv.register_buffer("eps", torch.empty(1))
    conv.reset_parameters()


def _gin_reset(module):
    """PyG's `reset`: reset_parameters() of every submodule that has one."""
    if hasattr(module, "reset_parameters"):
        module.reset_parameters()
    else:
        for child in module.children():
            _gin_reset(child)


class DenseGINConv(torch.nn.Module):
    """PyG's DenseGINConv: h = adj @ x, plus (1 + eps) x when add_loop; out = nn(h), times the mask.  adj [B,N,N]
    float (adj[b,i,j]: i aggregates from j): its values are weights and get a gradient, and its diagonal is an
    ordinary entry that add_loop does not overwrite.  x [B,N,F], F <= 128.  The aggregation and its gradients
    (x, adj, eps) are HIP kernels (csrc/ginconv.hip) that read eps on the device; `nn` is any module and runs under
    torch autograd (pass gcm.nn.SkinnyLinear layers for no library GEMM).  `eps` [1] is a Parameter when train_eps,
    else a buffer; state_dict keys `eps`, `nn.*`, shared with GINConv.  Not a DenseGraphConv: DenseGCM runs a GIN
    stack through its layered path."""

    def __init__(self, nn, eps=0.0, train_eps=False):
        super().__init__()
        _gin_init(self, nn, eps, train_eps)

    def reset_parameters(self):
        _gin_reset(self.nn)
        self.eps.data.fill_(self.initial_eps)

    def forward(self, x, adj, mask=None, add_loop=True):
        x, adj = _dense_contract(self, x, adj, mask)
        h = _ops.dense_gin_aggregate(x, adj, self.eps, add_loop)
        out = _ready_grad(self.nn(h))
        return _masked(out, mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}(nn={self.nn})"


class GINConv(torch.nn.Module):
    """PyG's GINConv (flow source_to_target): h_i = (1 + eps) x_i + sum over the edges j -> i of x_j, out = nn(h);
    edge_index [2,E] = (source, sink), x [M,F], F <= 128.  The edges are used as given: no self-loop is added or
    removed, an i -> i edge is an ordinary term, duplicates count once each; there are no edge weights.  The CSR
    aggregation and its gradients (x, eps) are HIP kernels (csrc/ginconv.hip); `nn` runs under torch autograd.  Uses
    the `edge_index.gcm_graph` index SparseGCM attaches; any other edge list is indexed here.  Parameters as
    DenseGINConv.  Not a GraphConv: SparseGCM runs a GIN stack through its generic path."""

    def __init__(self, nn, eps=0.0, train_eps=False):
        super().__init__()
        _gin_init(self, nn, eps, train_eps)

    def reset_parameters(self):
        _gin_reset(self.nn)
        self.eps.data.fill_(self.initial_eps)

    def forward(self, x, edge_index):
        x, edge_index, _, _ = _sparse_contract(self, x, edge_index)
        graph = _graph_of(x, edge_index, "GINConv")
        return _ready_grad(self.nn(_ops.csr_gin_aggregate(x, self.eps, graph)))

    def __repr__(self):
        return f"{self.__class__.__name__}(nn={self.nn})"


def _gat_check(dropout, edge_dim=None):
    """Widths beyond the kernels' (in_channels or heads * out_channels > 128) raise at the first call."""
    if dropout < 0 or dropout > 1:
        raise ValueError(f"dropout must be in [0, 1]; got {dropout}")
    if edge_dim is not None:
        raise NotImplementedError("GATConv(edge_dim=...) is not implemented: edge features are not attended to")


def _gat_params(conv, in_channels, out_channels, heads, concat, bias, att_shape):
    conv.in_channels, conv.out_channels, conv.heads, conv.concat = in_channels, out_channels, heads, concat
    conv.lin = torch.nn.Linear(in_channels, heads * out_channels, bias=False)
    conv.att_src = torch.nn.Parameter(torch.empty(att_shape))
    conv.att_dst = torch.nn.Parameter(torch.empty(att_shape))
    conv.bias = torch.nn.Parameter(torch.empty(heads * out_channels if concat else out_channels)) if bias else None


def _gat_reset(conv):
    torch.nn.init.xavier_uniform_(conv.lin.weight)
    bound = (6.0 / (conv.heads + conv.out_channels)) ** 0.5      # PyG's glorot on [.., H, C]
    for att in (conv.att_src, conv.att_dst):
        torch.nn.init.uniform_(att, -bound, bound)
    if conv.bias is not None:
        torch.nn.init.zeros_(conv.bias)


class DenseGATConv(torch.nn.Module):
    """PyG's DenseGATConv (GAT v1): adj[b,i,j] != 0 means i attends to j (only the pattern matters; the
    diagonal is set when add_loop); y = x W^T viewed [B,N,H,C], e_ij = leaky_relu(<y_i, att_dst> +
    <y_j, att_src>), alpha = softmax_j over the pattern, out_i = sum_j alpha_ij y_j, heads concatenated
    (or averaged), + bias, * mask.  A row with no neighbour aggregates nothing (out = bias), where PyG's
    dense formula gives NaN.  Forward and backward are HIP kernels (csrc/gatconv.hip); adj gets no
    gradient.  Attention dropout is not implemented (dropout > 0 raises in training mode).  Not a
    DenseGraphConv: DenseGCM runs a GAT stack through its layered path."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
                 bias=True):
        super().__init__()
        _gat_params(self, in_channels, out_channels, heads, concat, bias, (1, 1, heads, out_channels))
        self.negative_slope, self.dropout = negative_slope, dropout
        _gat_check(dropout)
        self.reset_parameters()

    def reset_parameters(self):
        _gat_reset(self)

    def forward(self, x, adj, mask=None, add_loop=True):
        _no_attention_dropout(self)
        x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
        out = _ops.dense_gatconv(x, adj.detach(), self.lin.weight, self.att_src, self.att_dst, self.bias,
                                 self.heads, self.concat, add_loop, self.negative_slope)
        return _masked(out, mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads})"


class GATConv(torch.nn.Module):
    """PyG's GATConv (GAT v1, flow source_to_target): edge_index [2,E] = (source, sink), x [M,F].  With
    add_self_loops every i -> i edge is removed and one loop per node added; duplicate edges are separate
    terms of the softmax, which runs per destination over its incoming edges (a node with none: out =
    bias).  edge_attr is accepted and ignored, as PyG does without edge_dim.  Uses the
    `edge_index.gcm_graph` index SparseGCM attaches; any other edge list is indexed here.  Forward and
    backward are HIP kernels (csrc/gatconv.hip).  Not implemented (NotImplementedError): attention
    dropout in training mode, edge_dim, return_attention_weights.  Not a GraphConv: SparseGCM runs a GAT
    stack through its generic path."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0,
                 add_self_loops=True, edge_dim=None, fill_value="mean", bias=True):
        super().__init__()
        _gat_params(self, in_channels, out_channels, heads, concat, bias, (1, heads, out_channels))
        self.negative_slope, self.dropout = negative_slope, dropout
        self.add_self_loops, self.edge_dim, self.fill_value = add_self_loops, edge_dim, fill_value
        _gat_check(dropout, edge_dim)
        self.reset_parameters()

    def reset_parameters(self):
        _gat_reset(self)

    def forward(self, x, edge_index, edge_attr=None, return_attention_weights=None):
        if return_attention_weights is not None:
            raise NotImplementedError("GATConv(return_attention_weights=...) is not implemented")
        _no_attention_dropout(self)
        x, edge_index, _, _ = _sparse_contract(self, x, edge_index, self.in_channels, edge_attr=edge_attr)
        graph = _graph_of(x, edge_index, "GATConv")
        return _ops.csr_gatconv(x, self.lin.weight, self.att_src, self.att_dst, self.bias, graph, self.heads,
                                self.concat, self.add_self_loops, self.negative_slope)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads})"


class GATv2Conv(torch.nn.Module):
    """Placeholder for PyG's GATv2Conv, so a port fails with a clear message instead of an ImportError."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("GATv2Conv is not implemented; gcm.nn has GATConv / DenseGATConv (GAT v1)")


def _transformer_params(conv, in_channels, out_channels, heads, concat, beta, dropout, bias, root_weight):
    if not isinstance(in_channels, int):
        raise NotImplementedError("TransformerConv with a tuple in_channels (bipartite graphs) is not implemented")
    if dropout < 0 or dropout > 1:
        raise ValueError(f"dropout must be in [0, 1]; got {dropout}")
    conv.in_channels, conv.out_channels, conv.heads, conv.concat = in_channels, out_channels, heads, concat
    conv.root_weight, conv.beta, conv.dropout = root_weight, bool(beta and root_weight), dropout
    width = heads * out_channels if concat else out_channels
    conv.lin_key = torch.nn.Linear(in_channels, heads * out_channels)
    conv.lin_query = torch.nn.Linear(in_channels, heads * out_channels)
    conv.lin_value = torch.nn.Linear(in_channels, heads * out_channels)
    conv.lin_skip = torch.nn.Linear(in_channels, width, bias=bias) if root_weight else None
    conv.lin_beta = torch.nn.Linear(3 * width, 1, bias=False) if conv.beta else None


def _transformer_reset(conv):
    for lin in (conv.lin_key, conv.lin_query, conv.lin_value, conv.lin_skip, conv.lin_beta):
        if lin is not None:
            lin.reset_parameters()


def _transformer_operands(conv):
    """(w_all [P,F], b_all [P], w_beta [3 D] | None): the projections stacked [query; key; value; skip], so the
    kernels make one pass over x and autograd hands each Linear its slice of the stacked gradient."""
    lins = [conv.lin_query, conv.lin_key, conv.lin_value] + ([conv.lin_skip] if conv.root_weight else [])
    w_all = torch.cat([lin.weight for lin in lins])
    b_all = torch.cat([lin.bias if lin.bias is not None else lin.weight.new_zeros(lin.out_features) for lin in lins])
    return w_all, b_all, (conv.lin_beta.weight.view(-1) if conv.beta else None)


class DenseTransformerConv(torch.nn.Module):
    """The dense form of PyG's TransformerConv: adj[b,i,j] != 0 means i attends to j (only the pattern matters; the
    diagonal counts as set when add_loop, which defaults to False so that dense and sparse agree on one edge set).
    q, k, v = lin_query(x), lin_key(x), lin_value(x) viewed [B,N,H,C]; alpha = softmax_j(<q_i, k_j> / sqrt(C)) over
    the pattern, o_i = sum_j alpha_ij v_j, heads concatenated (or averaged); with root_weight r = lin_skip(x) and out
    = o + r, or with beta the gate b = sigmoid(lin_beta([o, r, o - r])), out = b r + (1 - b) o; * mask.  A row with
    no neighbour aggregates nothing (o = 0).  Same parameters as TransformerConv: the state_dicts interchange.
    Forward and backward are HIP kernels (csrc/transformerconv.hip); adj gets no gradient.  Attention dropout is
    not implemented (dropout > 0 raises in training mode).  Not a DenseGraphConv: DenseGCM runs a stack of these
    through its layered path."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, bias=True,
                 root_weight=True):
        super().__init__()
        _transformer_params(self, in_channels, out_channels, heads, concat, beta, dropout, bias, root_weight)
        self.reset_parameters()

    def reset_parameters(self):
        _transformer_reset(self)

    def forward(self, x, adj, mask=None, add_loop=False):
        _no_attention_dropout(self)
        x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
        w_all, b_all, w_beta = _transformer_operands(self)
        out = _ops.dense_transformerconv(x, adj.detach(), w_all, b_all, w_beta, self.heads, self.concat,
                                         self.root_weight, add_loop)
        return _masked(out, mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads})"


class TransformerConv(torch.nn.Module):
    """PyG's TransformerConv (flow source_to_target) without edge features: edge_index [2,E] = (source, sink), x
    [M,F].  The edges are used as given: no loop is added or removed, duplicates are separate terms of the softmax,
    which runs per destination over its incoming edges (a node with none: out = lin_skip(x), or 0 without
    root_weight).  edge_attr is accepted and ignored, as PyG does without edge_dim.  Uses the `edge_index.gcm_graph`
    index SparseGCM attaches; any other edge list is indexed here.  Forward and backward are HIP kernels
    (csrc/transformerconv.hip).  Not implemented (NotImplementedError): attention dropout in training mode,
    edge_dim, return_attention_weights, a tuple in_channels.  Not a GraphConv: SparseGCM runs a stack of these
    through its generic path."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None,
                 bias=True, root_weight=True):
        super().__init__()
        if edge_dim is not None:
            raise NotImplementedError("TransformerConv(edge_dim=...) is not implemented: edge features are not "
                                      "attended to")
        _transformer_params(self, in_channels, out_channels, heads, concat, beta, dropout, bias, root_weight)
        self.edge_dim = edge_dim
        self.reset_parameters()

    def reset_parameters(self):
        _transformer_reset(self)

    def forward(self, x, edge_index, edge_attr=None, return_attention_weights=None):
        if return_attention_weights is not None:
            raise NotImplementedError("TransformerConv(return_attention_weights=...) is not implemented")
        _no_attention_dropout(self)
        x, edge_index, _, _ = _sparse_contract(self, x, edge_index, self.in_channels, edge_attr=edge_attr)
        graph = _graph_of(x, edge_index, "TransformerConv")
        w_all, b_all, w_beta = _transformer_operands(self)
        return _ops.csr_transformerconv(x, w_all, b_all, w_beta, graph, self.heads, self.concat, self.root_weight)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, heads={self.heads})"


def _resgated_params(conv, name, in_channels, out_channels, act, root_weight, bias):
    if not isinstance(in_channels, int):
        raise NotImplementedError(f"{name} with a tuple in_channels (bipartite graphs) is not implemented")
    if act is not None and not isinstance(act, torch.nn.Sigmoid):
        raise NotImplementedError(f"{name}(act=...) is not implemented for gates other than torch.nn.Sigmoid(); "
                                  f"got {act!r}")
    conv.in_channels, conv.out_channels, conv.root_weight = in_channels, out_channels, root_weight
    conv.act = torch.nn.Sigmoid() if act is None else act
    conv.lin_key = torch.nn.Linear(in_channels, out_channels)
    conv.lin_query = torch.nn.Linear(in_channels, out_channels)
    conv.lin_value = torch.nn.Linear(in_channels, out_channels)
    conv.lin_skip = torch.nn.Linear(in_channels, out_channels, bias=False) if root_weight else None
    conv.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
    conv.reset_parameters()


def _resgated_reset(conv):
    for lin in (conv.lin_key, conv.lin_query, conv.lin_value, conv.lin_skip):
        if lin is not None:
            lin.reset_parameters()
    if conv.bias is not None:
        torch.nn.init.zeros_(conv.bias)


def _resgated_operands(conv):
    """(w_all [P,F], b_all [P]): the projections stacked [key; query; value; skip] (the skip's bias slots zero), so
    the kernels make one pass over x and autograd hands each Linear its slice of the stacked gradient."""
    lins = [conv.lin_key, conv.lin_query, conv.lin_value]
    w = [lin.weight for lin in lins]
    b = [lin.bias for lin in lins]
    if conv.root_weight:
        w.append(conv.lin_skip.weight)
        b.append(conv.lin_skip.weight.new_zeros(conv.out_channels))
    return torch.cat(w), torch.cat(b)


class DenseResGatedGraphConv(torch.nn.Module):
    """The dense form of PyG's ResGatedGraphConv (Bresson & Laurent): k, q, v = lin_key(x), lin_query(x),
    lin_value(x); out_i = lin_skip(x_i) + sum_j adj_ij sigmoid(k_i + q_j) * v_j + bias, * mask.  adj [B,N,N] float
    (adj[b,i,j]: the edge j -> i): its values are weights and get a gradient when they ask for one, an entry equal
    to 0 is no edge and is skipped; add_loop (default False, so that dense and sparse agree on one edge set)
    overwrites the diagonal with 1.  The gate is per edge and per channel and is not normalised over the
    neighbourhood; a row with no neighbour outputs lin_skip(x_i) + bias.  x [B,N,F]; F, out_channels <= 128.  Same
    parameters as ResGatedGraphConv: the state_dicts interchange.  Forward and backward are HIP kernels
    (csrc/resgatedconv.hip) that visit the set entries only and store no gate.  Not a DenseGraphConv: DenseGCM runs
    a stack of these through its layered path."""

    def __init__(self, in_channels, out_channels, act=None, root_weight=True, bias=True):
        super().__init__()
        _resgated_params(self, "DenseResGatedGraphConv", in_channels, out_channels, act, root_weight, bias)

    def reset_parameters(self):
        _resgated_reset(self)

    def forward(self, x, adj, mask=None, add_loop=False):
        x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
        w_all, b_all = _resgated_operands(self)
        out = _ops.dense_resgatedconv(x, adj, w_all, b_all, self.bias, self.root_weight, add_loop)
        return _masked(out, mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"


class ResGatedGraphConv(torch.nn.Module):
    """PyG's ResGatedGraphConv (flow source_to_target) without edge features: edge_index [2,E] = (source, sink), x
    [M,F]; out_i = lin_skip(x_i) + sum over the edges j -> i of sigmoid(lin_key(x_i) + lin_query(x_j)) *
    lin_value(x_j) + bias.  The edges are used as given: no loop is added or removed, duplicates count once each; a
    node without an in-edge outputs lin_skip(x_i) + bias.  edge_attr is accepted and ignored, as PyG does without
    edge_dim.  Uses the `edge_index.gcm_graph` index SparseGCM attaches; any other edge list is indexed here.
    Forward and backward are HIP kernels (csrc/resgatedconv.hip).  Not implemented (NotImplementedError): edge_dim,
    a tuple in_channels, a gate `act` other than torch.nn.Sigmoid().  Not a GraphConv: SparseGCM runs a stack of
    these through its generic path."""

    def __init__(self, in_channels, out_channels, act=None, edge_dim=None, root_weight=True, bias=True):
        super().__init__()
        if edge_dim is not None:
            raise NotImplementedError("ResGatedGraphConv(edge_dim=...) is not implemented: edge features do not "
                                      "enter the gate")
        self.edge_dim = edge_dim
        _resgated_params(self, "ResGatedGraphConv", in_channels, out_channels, act, root_weight, bias)

    def reset_parameters(self):
        _resgated_reset(self)

    def forward(self, x, edge_index, edge_attr=None):
        x, edge_index, _, _ = _sparse_contract(self, x, edge_index, self.in_channels, edge_attr=edge_attr)
        graph = _graph_of(x, edge_index, "ResGatedGraphConv")
        w_all, b_all = _resgated_operands(self)
        return _ops.csr_resgatedconv(x, w_all, b_all, self.bias, graph, self.root_weight)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"


def _gated_params(conv, out_channels, num_layers, bias):
    if num_layers < 1:
        raise ValueError(f"num_layers must be at least 1; got {num_layers}")
    conv.out_channels, conv.num_layers = out_channels, num_layers
    conv.weight = torch.nn.Parameter(torch.empty(num_layers, out_channels, out_channels))
    conv.rnn = torch.nn.GRUCell(out_channels, out_channels, bias=bias)
    conv.reset_parameters()


def _gated_reset(conv):
    bound = 1.0 / conv.out_channels ** 0.5      # PyG's uniform(out_channels, weight)
    torch.nn.init.uniform_(conv.weight, -bound, bound)
    conv.rnn.reset_parameters()


def _gated_cell(conv):
    """(w_ih, w_hh, b_ih, b_hh) of the GRU cell, whose own forward is never called."""
    rnn = conv.rnn
    return rnn.weight_ih, rnn.weight_hh, getattr(rnn, "bias_ih", None), getattr(rnn, "bias_hh", None)


class DenseGatedGraphConv(torch.nn.Module):
    """The dense form of PyG's GatedGraphConv (Li et al., Gated Graph Sequence Neural Networks): h_0 = x zero-padded
    to out_channels columns; num_layers rounds of m = adj @ (h weight[l]), h = GRUCell(m, h); out = h, * mask.  adj
    [B,N,N] float (adj[b,i,j]: the edge j -> i): its values are weights and get a gradient when they ask for one
    (for every entry, also where adj is 0), an entry equal to 0 is no edge and is skipped; add_loop (default False,
    so that dense and sparse agree on one edge set) overwrites the diagonal with 1.  A row with no neighbour still
    updates through the cell with m = 0.  x [B,N,F] with F <= out_channels <= 128.  Same parameters as
    GatedGraphConv (`weight` [num_layers,C,C], `rnn`: a torch.nn.GRUCell): the state_dicts interchange.  Forward
    and backward are HIP kernels (csrc/gatedgraphconv.hip): one launch per round, the gates never leave the
    registers.  Not a DenseGraphConv: DenseGCM runs a stack of these through its layered path."""

    def __init__(self, out_channels, num_layers, bias=True):
        super().__init__()
        _gated_params(self, out_channels, num_layers, bias)

    def reset_parameters(self):
        _gated_reset(self)

    def forward(self, x, adj, mask=None, add_loop=False):
        x, adj = _dense_contract(self, x, adj, mask, max_channels=self.out_channels)
        out = _ops.dense_gatedgraphconv(x, adj, self.weight, *_gated_cell(self), add_loop)
        return _masked(out, mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.out_channels}, num_layers={self.num_layers})"


class GatedGraphConv(torch.nn.Module):
    """PyG's GatedGraphConv (flow source_to_target), aggr="add": edge_index [2,E] = (source, sink), x [M,F] with F <=
    out_channels <= 128, zero-padded to out_channels; num_layers rounds of m_i = sum over the edges j -> i of w_ji
    (h weight[l])_j, h = GRUCell(m, h).  The edges are used as given: no loop is added or removed, duplicates are
    separate terms; a node without an in-edge still updates through the cell with m = 0.  edge_weight follows
    GraphConv's rules (a wrong-length vector is ignored, SparseGCM's unit weights are not loaded) and gets a gradient
    when it asks for one.  Uses the `edge_index.gcm_graph` index SparseGCM attaches; any other edge list is indexed
    here.  Forward and backward are HIP kernels (csrc/gatedgraphconv.hip).  Other aggregations raise
    NotImplementedError.  Not a GraphConv: SparseGCM runs a stack of these through its generic path."""

    def __init__(self, out_channels, num_layers, aggr="add", bias=True):
        super().__init__()
        if aggr != "add":
            raise NotImplementedError(f"GatedGraphConv(aggr='{aggr}') is not implemented: aggr must be 'add'")
        self.aggr = aggr
        _gated_params(self, out_channels, num_layers, bias)

    def reset_parameters(self):
        _gated_reset(self)

    def forward(self, x, edge_index, edge_weight=None):
        x, edge_index, edge_weight, _ = _sparse_contract(self, x, edge_index, edge_weight=edge_weight,
                                                         max_channels=self.out_channels)
        graph = _graph_of(x, edge_index, "GatedGraphConv")
        w = _csr_weights(edge_weight, graph)
        return _ops.csr_gatedgraphconv(x, w, self.weight, *_gated_cell(self), graph)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.out_channels}, num_layers={self.num_layers})"


def _tag_params(conv, in_channels, out_channels, K, bias, normalize):
    if K < 0:
        raise ValueError(f"K must be at least 0; got {K}")
    conv.in_channels, conv.out_channels, conv.K, conv.normalize = in_channels, out_channels, K, normalize
    conv.lins = torch.nn.ModuleList(torch.nn.Linear(in_channels, out_channels, bias=False) for _ in range(K + 1))
    if bias:
        conv.bias = torch.nn.Parameter(torch.zeros(out_channels))
    else:
        conv.register_parameter("bias", None)


def _tag_reset(conv):
    for lin in conv.lins:
        lin.reset_parameters()
    if conv.bias is not None:
        torch.nn.init.zeros_(conv.bias)


def _tag_weight(conv):
    """The hop matrices stacked [K+1, out, in]: the kernels' operand (the stack's backward hands each its slice)."""
    return torch.stack([lin.weight for lin in conv.lins])


class DenseTAGConv(torch.nn.Module):
    """The dense form of PyG's TAGConv (Du et al., Topology Adaptive Graph Convolutional Networks), a K-hop polynomial
    filter in one layer: h_0 = x, h_k = A^ h_{k-1}, out = (sum_{k=0..K} h_k lins[k].weight^T + bias) * mask.  adj
    [B,N,N] float32 (adj[b,i,j]: the weight of the edge j -> i; 2-D and a batch of one are broadcast) gets a gradient
    when it asks for one, for every entry, also where adj is 0, the degree term of its row included; add_loop (default
    False, so that dense and sparse agree on one edge set) overwrites the diagonal with 1 before the degrees are
    taken, and that diagonal gets gradient 0.  With normalize (the default) A^ = D^-1/2 A D^-1/2, deg_i = sum_j A_ij,
    d_i = deg_i^-1/2 and 0 where deg_i == 0 (no clamp to 1 as in DenseGCNConv: dense and sparse agree); otherwise A^
    = adj.  Faithful to PyG on directed graphs: with normalize a node WITHOUT in-edges has d = 0 and sends nothing -
    in a TemporalBackedge memory that is the oldest node; add_loop=True or normalize=False avoids it.  K = 0 is the
    plain linear layer.  x [B,N,F]; in_channels, out_channels <= 128; float32.  Same parameters as TAGConv
    (lins.k.weight, bias): the state_dicts interchange.  Forward and backward are HIP kernels (csrc/tagconv.hip): for
    N <= 128 every hop runs in one launch with the adjacency read once.  Not a DenseGraphConv: DenseGCM runs a stack
    of these through its layered path."""

    def __init__(self, in_channels, out_channels, K=3, bias=True, normalize=True):
        super().__init__()
        _tag_params(self, in_channels, out_channels, K, bias, normalize)

    def reset_parameters(self):
        _tag_reset(self)

    def forward(self, x, adj, mask=None, add_loop=False):
        x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
        out = _ops.dense_tagconv(x, adj, _tag_weight(self), self.bias, self.normalize, add_loop)
        return _masked(out, mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, K={self.K})"


class TAGConv(torch.nn.Module):
    """PyG's TAGConv (flow source_to_target), a K-hop polynomial filter in one layer: edge_index [2,E] = (source,
    sink), x [M,F]; h_0 = x, h_k[i] = sum over the edges j -> i of c_e h_{k-1}[j], out = sum_{k=0..K} h_k
    lins[k].weight^T + bias.  With normalize (the default) c_e is PyG's gcn_norm(add_self_loops=False): deg_i = the
    sum of the weights INTO i, d_i = deg_i^-1/2 and 0 where deg_i == 0, c_e = d_src w_e d_dst; otherwise c_e = w_e.
    The edges are used as given: no loop is added or removed (i -> i is an ordinary edge), duplicates are separate
    terms.  Faithful to PyG on directed graphs: with normalize a node WITHOUT in-edges has d = 0 and sends nothing -
    in a TemporalBackedge memory that is the oldest node; normalize=False avoids it.  edge_weight follows
    GatedGraphConv's rules (a wrong-length vector is ignored, SparseGCM's unit weights are not loaded) and gets a
    gradient when it asks for one.  K = 0 is the plain linear layer.  in_channels, out_channels <= 128; float32.
    Parameters as PyG's (lins.k.weight, bias).  Uses the `edge_index.gcm_graph` index SparseGCM attaches; any other
    edge list is indexed here.  Forward and backward are HIP kernels (csrc/tagconv.hip), one launch per hop.  Not a
    GraphConv: SparseGCM runs a stack of these through its generic path."""

    def __init__(self, in_channels, out_channels, K=3, bias=True, normalize=True):
        super().__init__()
        _tag_params(self, in_channels, out_channels, K, bias, normalize)

    def reset_parameters(self):
        _tag_reset(self)

    def forward(self, x, edge_index, edge_weight=None):
        x, edge_index, edge_weight, _ = _sparse_contract(self, x, edge_index, self.in_channels, edge_weight=edge_weight)
        graph = _graph_of(x, edge_index, "TAGConv")
        w = _csr_weights(edge_weight, graph)
        return _ops.csr_tagconv(x, w, _tag_weight(self), self.bias, graph, self.normalize)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, K={self.K})"


def degree_histogram(adj_or_edge_index, num_nodes=None):
    """The `deg` argument of PNAConv / DensePNAConv from a graph at hand (a memory user has no dataset loader to take
    it from: a rollout's final adjacency will do): a LongTensor whose entry d is the number of nodes with in-degree d.
    An integer tensor [2,E] is an edge list (source, sink) over num_nodes nodes (default: the largest index + 1); any
    other tensor is an adjacency [N,N] or [B,N,N] whose row i has one neighbour per non-zero entry.  Plain torch ops."""
    t = adj_or_edge_index
    if t.dim() == 2 and t.shape[0] == 2 and not t.is_floating_point() and t.dtype != torch.bool:
        if num_nodes is None:
            num_nodes = int(t.max()) + 1 if t.numel() else 0
        deg = torch.bincount(t[1].reshape(-1), minlength=num_nodes)
    else:
        deg = (t != 0).sum(-1).reshape(-1)
    return torch.bincount(deg)


_PNA_ACTS = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid, "elu": torch.nn.ELU,
             "leaky_relu": torch.nn.LeakyReLU, "gelu": torch.nn.GELU, "silu": torch.nn.SiLU}


class _DegreeScalers(torch.nn.Module):
    """Holds PyG's `aggr_module.avg_deg_lin` / `aggr_module.avg_deg_log` buffers ([1] each) of a degree histogram."""

    def __init__(self, deg):
        super().__init__()
        deg = torch.as_tensor(deg).detach().to("cpu", torch.float64).reshape(-1)     # a histogram from the device too
        n = float(deg.sum())
        if n <= 0:
            raise ValueError("deg must count at least one node")
        d = torch.arange(deg.numel(), dtype=torch.float64)
        self.register_buffer("avg_deg_lin", ((d * deg).sum() / n).to(torch.float32).reshape(1))
        self.register_buffer("avg_deg_log", (((d + 1).log() * deg).sum() / n).to(torch.float32).reshape(1))


def _pna_params(conv, name, in_channels, out_channels, aggregators, scalers, deg, towers, pre_layers, post_layers,
                divide_input, act, act_kwargs, train_norm):
    if not isinstance(in_channels, int):
        raise NotImplementedError(f"{name} with a tuple in_channels (bipartite graphs) is not implemented")
    if pre_layers != 1:
        raise NotImplementedError(f"{name}(pre_layers={pre_layers}) is not implemented: the kernels rely on a message "
                                  "that is linear in x_i and x_j (pre_layers=1)")
    if train_norm:
        raise NotImplementedError(f"{name}(train_norm=True) is not implemented: the degree statistics are buffers")
    aggregators, scalers = list(aggregators), list(scalers)
    for a in aggregators:
        if a not in _ops.PNA_AGGREGATORS:
            raise ValueError(f"unknown aggregator '{a}': one of {sorted(_ops.PNA_AGGREGATORS)}")
    for s in scalers:
        if s not in _ops.PNA_SCALERS:
            raise ValueError(f"unknown scaler '{s}': one of {sorted(_ops.PNA_SCALERS)}")
    if not 1 <= len(aggregators) <= 8 or not 1 <= len(scalers) <= 8:
        raise ValueError("aggregators and scalers take 1 to 8 names each")
    if post_layers < 1:
        raise ValueError(f"post_layers must be at least 1; got {post_layers}")
    if divide_input:
        assert in_channels % towers == 0
    assert out_channels % towers == 0
    conv.in_channels, conv.out_channels, conv.towers, conv.divide_input = in_channels, out_channels, towers, divide_input
    conv.aggregators, conv.scalers = aggregators, scalers
    conv.pre_layers, conv.post_layers = pre_layers, post_layers
    conv.F_in = in_channels // towers if divide_input else in_channels
    conv.F_out = out_channels // towers
    conv.aggr_module = _DegreeScalers(deg)
    conv.pre_nns, conv.post_nns = torch.nn.ModuleList(), torch.nn.ModuleList()
    for _ in range(towers):
        conv.pre_nns.append(torch.nn.Sequential(torch.nn.Linear(2 * conv.F_in, conv.F_in)))
        mods = [torch.nn.Linear((len(aggregators) * len(scalers) + 1) * conv.F_in, conv.F_out)]
        for _ in range(post_layers - 1):
            if isinstance(act, str):
                if act not in _PNA_ACTS:
                    raise ValueError(f"unknown activation '{act}': one of {sorted(_PNA_ACTS)} or a module")
                mods.append(_PNA_ACTS[act](**(act_kwargs or {})))
            else:
                mods.append(torch.nn.Identity() if act is None else act)
            mods.append(torch.nn.Linear(conv.F_out, conv.F_out))
        conv.post_nns.append(torch.nn.Sequential(*mods))
    conv.lin = torch.nn.Linear(out_channels, out_channels)
    conv._cfg = _ops.PNAConfig(in_channels, out_channels, towers, divide_input, aggregators, scalers)


def _pna_reset(conv):
    for nns in (conv.pre_nns, conv.post_nns):
        for seq in nns:
            _gin_reset(seq)
    conv.lin.reset_parameters()


def _pna_operands(conv):
    """(w_pre [T,2Fi,Fi], b_pre [T,2Fi], w_post [T,Fo,K1], b_post [T,Fo], w_lin, b_lin, avg_deg [2]): each tower's pre
    weight split into its destination and source halves, stacked [dst; src] (the bias pads with zeros for the source
    half), and the first post linears stacked; autograd hands every Linear its slice of the stacked gradients.  With
    post_layers > 1 the final linear is not the kernels' (w_lin = b_lin = None)."""
    Fi = conv.F_in
    pre = [seq[0] for seq in conv.pre_nns]
    post = [seq[0] for seq in conv.post_nns]
    w_pre = torch.stack([torch.cat([lin.weight[:, :Fi], lin.weight[:, Fi:]]) for lin in pre])
    b_pre = torch.stack([torch.cat([lin.bias, lin.bias.new_zeros(Fi)]) for lin in pre])
    w_post = torch.stack([lin.weight for lin in post])
    b_post = torch.stack([lin.bias for lin in post])
    fused = conv.post_layers == 1
    agg = conv.aggr_module
    return (w_pre, b_pre, w_post, b_post, conv.lin.weight if fused else None, conv.lin.bias if fused else None,
            torch.cat([agg.avg_deg_lin, agg.avg_deg_log]))


def _pna_tail(conv, h):
    """post_layers > 1: what follows each tower's first post linear, and the final linear, as torch modules."""
    if conv.post_layers == 1:
        return h
    Fo = conv.F_out
    hs = [seq[1:](h[..., t * Fo:(t + 1) * Fo]) for t, seq in enumerate(conv.post_nns)]
    return _ready_grad(conv.lin(torch.cat(hs, -1)))


_PNA_DOC = """Per tower t (x_t: the tower's in_channels / towers columns of x with divide_input, else all of x): the
    message of every edge j -> i is m = pre_nns[t]([x_i | x_j]); the aggregators listed - sum, mean, min, max, var =
    mean(m^2) - mean(m)^2, std = sqrt(clamp(var, 1e-5)) set to 0 where that is <= sqrt(1e-5) - are taken per channel
    over the n_i messages of i and concatenated in list order; each scaler listed - identity, amplification log(n+1) /
    avg_deg_log, attenuation avg_deg_log / log(max(n,1)+1), linear n / avg_deg_lin, inverse_linear avg_deg_lin /
    max(n,1) - multiplies that block, the results concatenated in list order; h_t = post_nns[t]([x_t | scaled]); out =
    lin(cat_t h_t).  Every aggregator is 0 where n_i = 0; a tie in min / max goes to the first candidate, which alone
    gets the gradient.  `deg` is the histogram of in-degrees of the training graphs (gcm.nn.degree_histogram makes
    one): avg_deg_lin = sum d deg[d] / sum deg, avg_deg_log = sum log(d+1) deg[d] / sum deg.  Parameters and buffers
    carry PyG 2.3+'s names - pre_nns.t.0.{weight [F_in, 2 F_in], bias}, post_nns.t.0.{weight [F_out, (A S + 1) F_in],
    bias}, post_nns.t.{2,4,..} with post_layers > 1, lin.{weight, bias}, aggr_module.avg_deg_lin / avg_deg_log [1] -
    a layout written from PyG's source as remembered, which no test here can pin against an installed PyG.  Forward
    and backward are HIP kernels (csrc/pnaconv.hip): one pass over a neighbourhood produces every statistic, and no
    per-edge message is stored; with post_layers > 1 what follows each tower's first post linear runs as torch
    modules.  in_channels, out_channels <= 128 (wider: RuntimeError, code -2); float32.  Not implemented
    (NotImplementedError): edge_dim, pre_layers != 1, train_norm=True, a tuple in_channels."""


class DensePNAConv(torch.nn.Module):
    __doc__ = """The dense form of PyG's PNAConv (Corso et al., Principal Neighbourhood Aggregation; PyG has no dense
    twin): adj [B,N,N] float32, adj[b,i,j] != 0 means i aggregates from j; only the pattern is read and adj gets no
    gradient; add_loop (default False, so that dense and sparse agree on one edge set) sets the diagonal; x [B,N,F];
    the mask is applied last.  A tie in min / max goes to the lowest j.
    """ + _PNA_DOC + """  Same parameters as PNAConv: the state_dicts interchange.  Not a DenseGraphConv: DenseGCM
    runs a stack of these through its layered path."""

    def __init__(self, in_channels, out_channels, aggregators, scalers, deg, towers=1, pre_layers=1, post_layers=1,
                 divide_input=False, act="relu", act_kwargs=None, train_norm=False):
        super().__init__()
        _pna_params(self, "DensePNAConv", in_channels, out_channels, aggregators, scalers, deg, towers, pre_layers,
                    post_layers, divide_input, act, act_kwargs, train_norm)

    def reset_parameters(self):
        _pna_reset(self)

    def forward(self, x, adj, mask=None, add_loop=False):
        x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
        h = _ops.dense_pnaconv(x, adj.detach(), *_pna_operands(self), self._cfg, add_loop)
        return _masked(_pna_tail(self, h), mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, towers={self.towers})"


class PNAConv(torch.nn.Module):
    __doc__ = """PyG's PNAConv (Corso et al., Principal Neighbourhood Aggregation; flow source_to_target) without
    edge features: edge_index [2,E] = (source, sink), x [M,F].  The edges are used as given: no loop is added or
    removed, duplicates and self loops are separate messages, in CSR order (the edges stably sorted by sink): the
    first of them wins a tie in min / max.  Uses the `edge_index.gcm_graph` index SparseGCM attaches; any other edge
    list is indexed here.  edge_attr is accepted and ignored.
    """ + _PNA_DOC + """  Not a GraphConv: SparseGCM runs a stack of these through its generic path."""

    def __init__(self, in_channels, out_channels, aggregators, scalers, deg, edge_dim=None, towers=1, pre_layers=1,
                 post_layers=1, divide_input=False, act="relu", act_kwargs=None, train_norm=False):
        super().__init__()
        if edge_dim is not None:
            raise NotImplementedError("PNAConv(edge_dim=...) is not implemented: edge features do not enter the "
                                      "message")
        self.edge_dim = edge_dim
        _pna_params(self, "PNAConv", in_channels, out_channels, aggregators, scalers, deg, towers, pre_layers,
                    post_layers, divide_input, act, act_kwargs, train_norm)

    def reset_parameters(self):
        _pna_reset(self)

    def forward(self, x, edge_index, edge_attr=None):
        x, edge_index, _, _ = _sparse_contract(self, x, edge_index, self.in_channels, edge_attr=edge_attr)
        graph = _graph_of(x, edge_index, "PNAConv")
        return _pna_tail(self, _ops.csr_pnaconv(x, *_pna_operands(self), graph, self._cfg))

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, towers={self.towers})"


_RGCN_AGGRS = ("mean", "add", "sum")


def _rgcn_params(conv, name, in_channels, out_channels, num_relations, num_bases, num_blocks, aggr, root_weight, bias):
    """PyG 2.x's parameters: weight [R or num_bases, Fin, Fout], comp [R, num_bases] with bases, root [Fin, Fout],
    bias [Fout]."""
    if num_blocks is not None:
        raise NotImplementedError(f"{name}(num_blocks=...) is not implemented: the block-diagonal decomposition has "
                                  "no kernel; use num_bases or full weights")
    if not isinstance(in_channels, int) or isinstance(in_channels, bool):
        raise NotImplementedError(f"{name}: in_channels must be an int (a tuple is a bipartite graph and None an "
                                  "embedding lookup; neither is implemented)")
    if aggr not in _RGCN_AGGRS:
        raise NotImplementedError(f"{name}: aggr='{aggr}' is not implemented: one of {_RGCN_AGGRS}")
    if num_relations > _ops.RGCN_MAX_RELATIONS:
        raise NotImplementedError(f"{name}: num_relations={num_relations} is not implemented: the relation codes "
                                  f"carry {_ops.RGCN_MAX_RELATIONS} bits")
    if num_relations < 1 or (num_bases is not None and num_bases < 1):
        raise ValueError(f"{name}: num_relations and num_bases must be >= 1")
    conv.in_channels, conv.out_channels, conv.num_relations = in_channels, out_channels, num_relations
    conv.num_bases, conv.num_blocks, conv.aggr = num_bases, num_blocks, aggr
    if num_bases is not None:
        conv.weight = torch.nn.Parameter(torch.empty(num_bases, in_channels, out_channels))
        conv.comp = torch.nn.Parameter(torch.empty(num_relations, num_bases))
    else:
        conv.weight = torch.nn.Parameter(torch.empty(num_relations, in_channels, out_channels))
        conv.register_parameter("comp", None)
    if root_weight:
        conv.root = torch.nn.Parameter(torch.empty(in_channels, out_channels))
    else:
        conv.register_parameter("root", None)
    if bias:
        conv.bias = torch.nn.Parameter(torch.empty(out_channels))
    else:
        conv.register_parameter("bias", None)
    conv.reset_parameters()


def _rgcn_reset(conv):
    """PyG's glorot (uniform within sqrt(6 / (size(-2) + size(-1)))) for weight, comp and root; zeros for bias."""
    for p in (conv.weight, conv.comp, conv.root):
        if p is not None:
            bound = (6.0 / (p.shape[-2] + p.shape[-1])) ** 0.5
            torch.nn.init.uniform_(p, -bound, bound)
    if conv.bias is not None:
        torch.nn.init.zeros_(conv.bias)


def _rgcn_weight(conv):
    """[R, Fin, Fout]: the weights, or with bases comp . weight composed in torch under autograd."""
    if conv.comp is None:
        return conv.weight
    return (conv.comp @ conv.weight.view(conv.num_bases, -1)).view(conv.num_relations, conv.in_channels,
                                                                   conv.out_channels)


def _rgcn_codes(t, what):
    """Relation bit codes as the kernels read them; int64 codes keep their low 16 bits (more than any layer has)."""
    if t.dtype == torch.int64:
        return t.clamp(min=0) & 0xFFFF
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (holding integers) or int64; got {t.dtype}")
    return t


def _rgcn_repr(conv):
    return f"{conv.__class__.__name__}({conv.in_channels}, {conv.out_channels}, num_relations={conv.num_relations})"


_RGCN_DOC = """out_i = sum_r s_r(i) sum_j m_r(i,j) a(i,j) x_j W_r + x_i root + bias (Schlichtkrull et al., Modeling
    Relational Data with Graph Convolutional Networks): one weight matrix per relation.  s_r(i) = 1 / max(1, number of
    neighbours of i in relation r) for aggr="mean" - a count of the pattern, not of the values - and 1 for "add" /
    "sum"; a node without neighbours in a relation gets nothing from it.  Parameters as PyG 2.x: weight [R, Fin, Fout]
    (with num_bases: weight [num_bases, Fin, Fout] and comp [R, num_bases], composed in torch), root [Fin, Fout], bias
    [Fout]; glorot / zeros; the dense and the sparse layer load each other's state_dict.  Forward and backward are HIP
    kernels (csrc/rgcnconv.hip), float32, Fin, Fout <= 128, num_relations <= 16, bitwise reproducible.  num_blocks, a
    tuple or None for in_channels and other aggregations raise NotImplementedError."""


class DenseRGCNConv(torch.nn.Module):
    __doc__ = """The relational GCN on a dense adjacency with a RELATION PLANE: x [B,N,Fin], adj [B,N,N] float
    (adj[b,i,j]: i aggregates from j; its values are weights a(i,j) and get a gradient - a LearnedEdge stays trainable
    through this layer), rel of adj's shape, float32 holding integers or int64: bit r of rel[b,i,j] set means the entry
    lies in relation r; an entry may lie in several; codes <= 0 are no edge and bits >= num_relations are ignored.
    rel never gets a gradient.  In a DenseGCM(edge_weights=True) the plane is the memory's `weights`, written by
    edge_selectors.typed.TypedEdge: (DenseRGCNConv(F, H, sel.num_relations), "x, adj, weights -> x").  2-D input, a
    broadcast [1,N,N] adjacency and `mask` as in the other dense layers.
    """ + _RGCN_DOC + """  Not a DenseGraphConv: DenseGCM runs a stack of these through its layered path."""

    def __init__(self, in_channels, out_channels, num_relations, num_bases=None, num_blocks=None, aggr="mean",
                 root_weight=True, bias=True):
        super().__init__()
        _rgcn_params(self, "DenseRGCNConv", in_channels, out_channels, num_relations, num_bases, num_blocks, aggr,
                     root_weight, bias)

    def reset_parameters(self):
        _rgcn_reset(self)

    def forward(self, x, adj, rel, mask=None):
        x, adj, rel = _dense_contract(self, x, adj, mask, self.in_channels, planes=[("rel", rel)])
        rel = _rgcn_codes(rel, "rel")
        out = _ops.dense_rgcnconv(x, adj, rel.detach().to(torch.float32), _rgcn_weight(self), self.root, self.bias,
                                  self.aggr == "mean")
        return _masked(out, mask, x)

    def __repr__(self):
        return _rgcn_repr(self)


class RGCNConv(torch.nn.Module):
    __doc__ = """PyG's RGCNConv (flow source_to_target): x [M,Fin], edge_index [2,E] = (source, sink), edge_type [E]
    int64 relation ids.  An id outside [0, num_relations) contributes nothing; duplicate edges and self loops are
    separate messages, no loop is added; every edge has the value 1.  is_sorted is accepted and ignored.
    relation_mask=True (an extension): edge_type holds bit codes instead (int64, or float32 holding integers), so an
    edge may lie in several relations - the values of DenseToSparse(transpose=True, edge_values=True)(x, rel) go
    straight in.  Uses the `edge_index.gcm_graph` index when one is attached; any other edge list is indexed here.
    """ + _RGCN_DOC + """  Not a GraphConv: SparseGCM runs a stack of these through its generic path."""

    def __init__(self, in_channels, out_channels, num_relations, num_bases=None, num_blocks=None, aggr="mean",
                 root_weight=True, is_sorted=False, bias=True, relation_mask=False):
        super().__init__()
        self.is_sorted, self.relation_mask = is_sorted, bool(relation_mask)
        _rgcn_params(self, "RGCNConv", in_channels, out_channels, num_relations, num_bases, num_blocks, aggr,
                     root_weight, bias)

    def reset_parameters(self):
        _rgcn_reset(self)

    def forward(self, x, edge_index, edge_type):
        x, edge_index, _, edge_type = _sparse_contract(
            self, x, edge_index, self.in_channels, edge_type=edge_type,
            type_dtypes=_CODE_DTYPES if self.relation_mask else _I64)
        graph = _graph_of(x, edge_index, "RGCNConv")
        if edge_type is None or edge_type.numel() != graph.E:
            raise ValueError(f"RGCNConv: edge_type must hold one entry per edge ({graph.E})")
        if self.relation_mask:
            et = _rgcn_codes(edge_type.detach(), "edge_type").to(torch.int64)
        elif edge_type.dtype != torch.int64:
            raise TypeError(f"RGCNConv: edge_type must be int64 relation ids; got {edge_type.dtype}")
        else:
            et = edge_type
        if graph.csr_perm is not None:
            et = et[graph.csr_perm]
        return _ops.csr_rgcnconv(x, et, _rgcn_weight(self), self.root, self.bias, graph, self.aggr == "mean",
                                 self.relation_mask)

    def __repr__(self):
        return _rgcn_repr(self)


class _SoftmaxAggr(torch.nn.Module):
    """Holder of GENConv's temperature under PyG's key `aggr_module.t` [1]: a Parameter when learnt, else a
    persistent buffer."""

    def __init__(self, learn):
        super().__init__()
        if learn:
            self.t = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_buffer("t", torch.empty(1))


class _MessageNorm(torch.nn.Module):
    """PyG's MessageNorm: msg / max(|msg|_2, 1e-12) * |x|_2 * scale; `scale` [1] is trained with learn_scale."""

    def __init__(self, learn_scale):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.empty(1), requires_grad=learn_scale)
        self.reset_parameters()

    def reset_parameters(self):
        self.scale.data.fill_(1.0)

    def forward(self, x, msg):
        msg = torch.nn.functional.normalize(msg, p=2.0, dim=-1)
        return msg * x.norm(p=2, dim=-1, keepdim=True) * self.scale


_GEN_NORMS = {"batch": torch.nn.BatchNorm1d, "layer": torch.nn.LayerNorm}


def _gen_init(conv, name, in_channels, out_channels, aggr, t, learn_t, p, learn_p, msg_norm, learn_msg_scale, norm,
              num_layers, expansion, eps, bias, edge_dim):
    if edge_dim is not None:
        raise NotImplementedError(f"{name}(edge_dim=...) is not implemented: edge features do not enter the message")
    if aggr != "softmax":
        raise NotImplementedError(f"{name}(aggr={aggr!r}) is not implemented: 'softmax' only")
    if learn_p:
        raise NotImplementedError(f"{name}(learn_p=True) is not implemented: p belongs to the power mean")
    if norm == "instance":
        raise NotImplementedError(f"{name}(norm='instance') is not implemented: 'batch', 'layer' or None")
    if norm is not None and norm not in _GEN_NORMS:
        raise ValueError(f"{name}: unknown norm {norm!r}: 'batch', 'layer' or None")
    if not isinstance(in_channels, int):
        raise NotImplementedError(f"{name}: a tuple of in_channels (bipartite graphs) is not implemented")
    conv.in_channels, conv.out_channels, conv.aggr, conv.eps = in_channels, out_channels, aggr, float(eps)
    conv.initial_t, conv.learn_t, conv.p, conv.norm = float(t), bool(learn_t), p, norm
    conv.num_layers, conv.expansion = num_layers, expansion
    if in_channels != out_channels:
        conv.lin_src = torch.nn.Linear(in_channels, out_channels, bias=bias)
        conv.lin_dst = torch.nn.Linear(in_channels, out_channels, bias=bias)
    conv.aggr_module = _SoftmaxAggr(learn_t)
    if msg_norm:
        conv.msg_norm = _MessageNorm(learn_msg_scale)
    channels = [out_channels] + [out_channels * expansion] * (num_layers - 1) + [out_channels]
    layers = []
    for i in range(1, len(channels)):
        layers.append(torch.nn.Linear(channels[i - 1], channels[i], bias=bias))
        if i < len(channels) - 1:
            if norm is not None:
                layers.append(_GEN_NORMS[norm](channels[i]))
            layers += [torch.nn.ReLU(), torch.nn.Dropout(0.0)]
    conv.mlp = torch.nn.Sequential(*layers)
    conv.reset_parameters()


def _gen_reset(conv):
    _gin_reset(conv.mlp)
    for name in ("lin_src", "lin_dst", "msg_norm"):
        if hasattr(conv, name):
            getattr(conv, name).reset_parameters()
    conv.aggr_module.t.data.fill_(conv.initial_t)


def _gen_source(conv, x):
    """xs, what the aggregation kernels read: lin_src(x), or x itself when the widths agree."""
    return conv.lin_src(x) if hasattr(conv, "lin_src") else x


def _gen_tail(conv, x, agg):
    """Message norm, the residual with x_dst and the mlp over the rows [rows, C] (torch modules)."""
    if hasattr(conv, "msg_norm"):
        agg = conv.msg_norm(x, agg)
    out = agg + (conv.lin_dst(x) if hasattr(conv, "lin_dst") else x)
    return _ready_grad(conv.mlp(out.reshape(-1, conv.out_channels)).view(*out.shape[:-1], conv.out_channels))


_GEN_DOC = """m = relu(xs) + eps with xs = lin_src(x) (x itself when in_channels == out_channels); per channel c a
    node i averages the m_jc of its in-neighbours with the weights softmax_j(t m_jc): t = 0 is the mean, t -> inf the
    max, and every neighbour gets a gradient.  A node without in-edges aggregates 0.  With msg_norm the aggregate is
    scaled to agg / max(|agg|_2, 1e-12) * |x_i|_2 * scale (x the raw input).  out = mlp(agg + x_dst), x_dst =
    lin_dst(x) or x.  The aggregation and its gradients (xs, t) are HIP kernels (csrc/genconv.hip): one online-softmax
    pass per destination row, shifted by the row's own maximum, so logits of any size are exact; t is read on the
    device, so a layer with learn_t is HIP-graph capturable.  lin_src, lin_dst, the message norm and the mlp are torch
    modules.  Parameters as PyG 2.x: `lin_src.*` / `lin_dst.*` (only when the widths differ), `aggr_module.t` [1]
    (Parameter with learn_t, else a buffer), `msg_norm.scale` [1] (only with msg_norm; trained with learn_msg_scale),
    `mlp.*`: Linear, norm, ReLU, Dropout(0) per hidden layer of width out_channels * expansion, then a Linear
    (`mlp.0`, `mlp.1`, `mlp.4` with the defaults); `bias` governs every Linear.  norm: "batch" (BatchNorm1d), "layer"
    (LayerNorm) or None.  float32, out_channels <= 128.  Not implemented (NotImplementedError): edge_dim, any aggr but
    "softmax" (lists included), learn_p, norm="instance", a tuple of in_channels."""


class DenseGENConv(torch.nn.Module):
    __doc__ = """DeeperGCN's GENConv with softmax aggregation (PyG's GENConv) on a dense adjacency: x [B,N,F] or
    [N,F], adj [B,N,N], [1,N,N] or [N,N] float32 (adj[b,i,j] != 0: i aggregates from j).  Only the pattern of adj is
    read, as in the max aggregation: its values do not matter and it gets no gradient; the diagonal is an ordinary
    entry and no loop is added.  The output is multiplied by the mask.
    """ + _GEN_DOC + """  The mlp sees the rows as [B * N, C]: norm="batch" takes its statistics over padded rows
    too - inside a memory use norm="layer" or None.  Loads GENConv's state_dict.  Not a DenseGraphConv: DenseGCM runs
    a stack of these through its layered path."""

    def __init__(self, in_channels, out_channels, aggr="softmax", t=1.0, learn_t=False, p=1.0, learn_p=False,
                 msg_norm=False, learn_msg_scale=False, norm="batch", num_layers=2, expansion=2, eps=1e-7, bias=False,
                 edge_dim=None):
        super().__init__()
        _gen_init(self, "DenseGENConv", in_channels, out_channels, aggr, t, learn_t, p, learn_p, msg_norm,
                  learn_msg_scale, norm, num_layers, expansion, eps, bias, edge_dim)

    def reset_parameters(self):
        _gen_reset(self)

    def forward(self, x, adj, mask=None):
        x, adj = _dense_contract(self, x, adj, mask, self.in_channels)
        agg = _ops.dense_genagg(_gen_source(self, x), adj, self.aggr_module.t, self.eps)
        return _masked(_gen_tail(self, x, agg), mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, aggr={self.aggr})"


class GENConv(torch.nn.Module):
    __doc__ = """DeeperGCN's GENConv with softmax aggregation (PyG's GENConv, flow source_to_target) without edge
    features: edge_index [2,E] = (source, sink), x [M,F].  The edges are used as given: no loop is added or removed,
    an i -> i edge is an ordinary term, duplicates count once each; there are no edge weights.  Uses the
    `edge_index.gcm_graph` index SparseGCM attaches; any other edge list is indexed here.
    """ + _GEN_DOC + """  Loads DenseGENConv's state_dict.  Not a GraphConv: SparseGCM runs a stack of these through
    its generic path."""

    def __init__(self, in_channels, out_channels, aggr="softmax", t=1.0, learn_t=False, p=1.0, learn_p=False,
                 msg_norm=False, learn_msg_scale=False, norm="batch", num_layers=2, expansion=2, eps=1e-7, bias=False,
                 edge_dim=None):
        super().__init__()
        _gen_init(self, "GENConv", in_channels, out_channels, aggr, t, learn_t, p, learn_p, msg_norm,
                  learn_msg_scale, norm, num_layers, expansion, eps, bias, edge_dim)

    def reset_parameters(self):
        _gen_reset(self)

    def forward(self, x, edge_index):
        x, edge_index, _, _ = _sparse_contract(self, x, edge_index, self.in_channels)
        xs = _gen_source(self, x)
        graph = _graph_of(x, edge_index, "GENConv")
        return _gen_tail(self, x, _ops.csr_genagg(xs, self.aggr_module.t, graph, self.eps))

    def __repr__(self):
        return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, aggr={self.aggr})"


_EDGE_NN_FORM = ("torch.nn.Sequential(Linear(2 * F, H), ReLU() or LeakyReLU(s), Linear(H, C)); a monotone activation "
                 "behind the last Linear commutes with the max and can follow the layer instead")


def _edge_init(conv, name, nn, aggr):
    if aggr != "max":
        raise NotImplementedError(f"{name}(aggr={aggr!r}) is not implemented: 'max' only, with nn = {_EDGE_NN_FORM}")
    ok = (isinstance(nn, torch.nn.Sequential) and len(nn) == 3 and isinstance(nn[0], torch.nn.Linear)
          and isinstance(nn[1], (torch.nn.ReLU, torch.nn.LeakyReLU)) and isinstance(nn[2], torch.nn.Linear)
          and nn[0].in_features % 2 == 0 and nn[0].out_features == nn[2].in_features)
    if not ok:
        raise NotImplementedError(f"{name}: this nn is not implemented; the accepted form is {_EDGE_NN_FORM}")
    conv.nn, conv.aggr = nn, aggr
    conv.in_channels, conv.out_channels = nn[0].in_features // 2, nn[2].out_features


def _edge_width(conv):
    """in_channels as nn[0] has it now, and the wording of a mismatch, for the calling contract."""
    two_f = conv.nn[0].in_features
    return dict(in_channels=two_f / 2, width_error=lambda F: f"nn[0] takes {two_f} features, but [x_i, x_j - x_i] "
                                                             f"has 2 * {F}")


def _edge_terms(conv, x):
    """(P, Q, W2, b2, slope): the first Linear as two node-level products (torch), W1 = [A | Bm]:
    W1 [x_i, x_j - x_i] + b1 = P_i + Q_j with P = x (A - Bm)^T + b1, Q = x Bm^T."""
    lin1, act, lin2 = conv.nn[0], conv.nn[1], conv.nn[2]
    F = x.shape[-1]
    A, Bm = lin1.weight[:, :F], lin1.weight[:, F:]
    P = torch.nn.functional.linear(x, A - Bm, lin1.bias)
    Q = torch.nn.functional.linear(x, Bm)
    slope = act.negative_slope if isinstance(act, torch.nn.LeakyReLU) else 0.0
    return P, Q, lin2.weight, lin2.bias, slope


_EDGE_DOC = """x_i' = max over the in-neighbours j of i of nn([x_i, x_j - x_i]), per channel (Wang et al., Dynamic
    Graph CNN): the one layer here whose message depends on the relative feature x_j - x_i.  `nn` must be a
    torch.nn.Sequential of exactly Linear(2F -> H), ReLU() or LeakyReLU(s), Linear(H -> C) (subclasses of Linear such
    as SkinnyLinear count, biases are optional): state_dict keys `nn.0.weight`, `nn.0.bias`, `nn.2.weight`,
    `nn.2.bias`, PyG's own.  With nn.0.weight = [A | Bm] the first Linear is two node-level products, P = x (A - Bm)^T
    + b1 and Q = x Bm^T (torch, under autograd); the per-edge stage act(P_i + Q_j), the second Linear and the running
    max with its winner are HIP kernels (csrc/edgeconv.hip) that write neither the hidden activations nor the messages
    to memory; the gradient flows through the winning edge of every (node, channel) alone.  A node without in-edges
    gets 0 and sends no gradient.  Of bitwise equal messages the first wins: the lowest source index (dense), the first
    edge of the node in the list's order (sparse).  float32, H and C up to 128.  Not implemented
    (NotImplementedError at construction): any other nn - a single Linear, a trailing activation, norm layers inside
    the MLP, deeper MLPs - and any aggr but "max"; a monotone activation behind the last Linear commutes with the max
    and can follow the layer.  nn[0].in_features != 2 * x.shape[-1] raises ValueError at the call."""


class DenseEdgeConv(torch.nn.Module):
    __doc__ = """PyG's EdgeConv on a dense adjacency, which PyG does not have: x [B,N,F] or [N,F], adj [B,N,N],
    [1,N,N] or [N,N] float32 (adj[b,i,j] != 0: i receives from j).  Only the pattern of adj is read: its values do not
    matter and it gets no gradient; the diagonal is an ordinary entry (x_j - x_i = 0) and no loop is added.  The
    output is multiplied by the mask.
    """ + _EDGE_DOC + """  Loads EdgeConv's state_dict.  Not a DenseGraphConv: DenseGCM runs a stack of these through
    its layered path."""

    def __init__(self, nn, aggr="max"):
        super().__init__()
        _edge_init(self, "DenseEdgeConv", nn, aggr)

    def reset_parameters(self):
        _gin_reset(self.nn)

    def forward(self, x, adj, mask=None):
        x, adj = _dense_contract(self, x, adj, mask, **_edge_width(self))
        P, Q, w2, b2, slope = _edge_terms(self, x)
        return _masked(_ops.dense_edgemax(P, Q, adj, w2, b2, slope), mask, x)

    def __repr__(self):
        return f"{self.__class__.__name__}(nn={self.nn})"


class EdgeConv(torch.nn.Module):
    __doc__ = """PyG's EdgeConv (flow source_to_target): edge_index [2,E] = (source, sink), x [M,F].  The edges are
    used as given: no loop is added or removed, an i -> i edge is an ordinary entry with x_j - x_i = 0, duplicate
    edges compete separately.  Uses the `edge_index.gcm_graph` index SparseGCM attaches; any other edge list is indexed
    here.  DynamicEdgeConv is not provided: KNNEdge / SpatialKNNEdge + EdgeConv is the memory's form of it.
    """ + _EDGE_DOC + """  Loads DenseEdgeConv's state_dict.  Not a GraphConv: SparseGCM runs a stack of these through
    its generic path."""

    def __init__(self, nn, aggr="max"):
        super().__init__()
        _edge_init(self, "EdgeConv", nn, aggr)

    def reset_parameters(self):
        _gin_reset(self.nn)

    def forward(self, x, edge_index):
        x, edge_index, _, _ = _sparse_contract(self, x, edge_index, **_edge_width(self))
        P, Q, w2, b2, slope = _edge_terms(self, x)
        graph = _graph_of(x, edge_index, "EdgeConv")
        return _ops.csr_edgemax(P, Q, w2, b2, slope, graph)

    def __repr__(self):
        return f"{self.__class__.__name__}(nn={self.nn})"


class Sequential(torch.nn.Module):
    """Stand-in for torch_geometric.nn.Sequential: a chain of modules wired by
    name, e.g. Sequential("x, adj, weights, B, N", [(conv, "x, adj -> x"), Tanh()]).
    Sub-modules are registered as module_0, module_1, ... (PyG's naming), so
    state_dicts are key compatible.  A DenseGraphConv / GraphConv with aggr="add" immediately followed by a
    bare Tanh/ReLU is executed as ONE kernel (activation in the MFMA epilogue)."""

    def __init__(self, input_args, modules):
        super().__init__()

        def names(text):    # ("x, adj, -> ..." is accepted as PyG accepts it: the empty name is ignored)
            return [a.strip() for a in text.split(",") if a.strip()]

        self.arg_names = names(input_args)
        self._plan = []
        for i, entry in enumerate(modules):
            if isinstance(entry, (tuple, list)):
                mod, sig = entry
                lhs, rhs = sig.split("->")
                ins, outs = names(lhs), names(rhs)
            else:
                mod = entry
                prev = self._plan[-1][2] if self._plan else self.arg_names[:1]
                ins, outs = list(prev), list(prev)
            if isinstance(mod, torch.nn.Module):
                self.add_module(f"module_{i}", mod)
            elif callable(mod):     # a plain function (`lambda x: x`): a stage without parameters, same numbering
                setattr(self, f"module_{i}", mod)
            else:
                raise TypeError(f"Sequential: stage {i} is neither a Module nor a callable: {mod!r}")
            self._plan.append((f"module_{i}", ins, outs))

    def stages(self):
        """[(module, inputs, outputs)] in execution order."""
        return [(getattr(self, n), i, o) for n, i, o in self._plan]

    def forward(self, *args):
        env = dict(zip(self.arg_names, args))
        plan, out, i = self._plan, None, 0
        while i < len(plan):
            name, ins, outs = plan[i]
            mod = getattr(self, name)
            fused = None
            if isinstance(mod, (DenseGraphConv, GraphConv)) and mod.aggr == "add" and i + 1 < len(plan):
                nxt_name, nxt_in, nxt_out = plan[i + 1]
                nxt = getattr(self, nxt_name)
                if type(nxt) in _FUSABLE and nxt_in == outs and nxt_out == outs:
                    fused = _FUSABLE[type(nxt)]
            if fused is not None:
                out = mod(*[env[k] for k in ins], _act=fused)
                i += 2
            else:
                out = mod(*[env[k] for k in ins])
                i += 1
            if len(outs) == 1:
                env[outs[0]] = out
            else:
                for k, v in zip(outs, out):
                    env[k] = v
        return out


# the base class for layers this module does not fuse by hand, and the torch_geometric.utils functions such layers
# are written with (imported last: they build on _ops alone)
from .graph_utils import add_self_loops, degree, remove_self_loops, scatter, softmax  # noqa: E402,F401
from .message_passing import MessagePassing  # noqa: E402,F401
