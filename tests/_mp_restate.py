"""Pure-torch restatement of gcm.nn.MessagePassing and gcm.graph_utils, in any dtype on the CPU: index_select,
index_add_, and explicit first-in-stable-order winners for max / min (never scatter_reduce's backward, which splits the
gradient among ties).  The semantics it pins:

  * a segment without entries reduces to 0 for every aggr; mean divides by max(count, 1);
  * duplicate edges are separate terms, a loop is an ordinary edge, nothing is added or removed;
  * the gradient of max / min goes to ONE entry, the earliest edge of that sink in the caller's order;
  * softmax is per sink and per trailing element, without PyG's 1e-16 in the denominator.

The layer bodies further down are written ONCE against a base class and a utilities namespace (`layers(base, utils)`),
so the same class runs over this restatement and over gcm.nn.MessagePassing."""
import inspect
import types

import torch


# ---- utilities ------------------------------------------------------------------------------------
def _expand(index, like):
    return index.view((-1,) + (1,) * (like.dim() - 1)).expand_as(like)


def _winners(src, index, M, largest):
    """[M, ...] int64: the first entry e (in the given order) that attains the max / min of its segment, E where the
    segment is empty.  No gradient."""
    E = src.shape[0]
    s = src.detach()
    shape = (M,) + tuple(s.shape[1:])
    idx = _expand(index, s)
    best = torch.full(shape, float("-inf") if largest else float("inf"), dtype=s.dtype)
    best = best.scatter_reduce(0, idx, s, "amax" if largest else "amin", include_self=True)
    pos = torch.arange(E).view((-1,) + (1,) * (s.dim() - 1)).expand_as(s)
    cand = torch.where(s == best.gather(0, idx), pos, torch.full_like(pos, E))
    return torch.full(shape, E, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin", include_self=True)


def scatter(src, index, dim=0, dim_size=None, reduce="sum"):
    assert dim == 0
    M = int(dim_size) if dim_size is not None else (int(index.max()) + 1 if index.numel() else 0)
    shape = (M,) + tuple(src.shape[1:])
    if reduce in ("sum", "add", "mean"):
        out = torch.zeros(shape, dtype=src.dtype).index_add_(0, index, src)
        if reduce == "mean":
            count = torch.zeros(M, dtype=src.dtype).index_add_(0, index, torch.ones(index.numel(), dtype=src.dtype))
            out = out / count.clamp(min=1).view((-1,) + (1,) * (src.dim() - 1))
        return out
    assert reduce in ("max", "min")
    E = src.shape[0]
    if E == 0:
        return torch.zeros(shape, dtype=src.dtype) + 0 * src.sum()
    win = _winners(src, index, M, reduce == "max")
    picked = src.gather(0, win.clamp(max=E - 1))              # gather's backward: the whole gradient to that entry
    return torch.where(win < E, picked, torch.zeros_like(picked))


def softmax(src, index, ptr=None, num_nodes=None, dim=0):
    assert dim == 0 and ptr is None
    M = int(num_nodes) if num_nodes is not None else (int(index.max()) + 1 if index.numel() else 0)
    if src.shape[0] == 0:
        return src.clone()
    shape = (M,) + tuple(src.shape[1:])
    idx = _expand(index, src)
    mx = torch.full(shape, float("-inf"), dtype=src.dtype).scatter_reduce(0, idx, src.detach(), "amax")
    ex = torch.exp(src - mx.gather(0, idx))
    den = torch.zeros(shape, dtype=src.dtype).index_add_(0, index, ex)
    return ex / den.index_select(0, index)


def degree(index, num_nodes=None, dtype=None):
    N = int(num_nodes) if num_nodes is not None else (int(index.max()) + 1 if index.numel() else 0)
    dtype = torch.get_default_dtype() if dtype is None else dtype
    return torch.zeros(N, dtype=dtype).index_add_(0, index, torch.ones(index.numel(), dtype=dtype))


def add_self_loops(edge_index, edge_attr=None, fill_value=None, num_nodes=None):
    N = int(num_nodes) if num_nodes is not None else (int(edge_index.max()) + 1 if edge_index.numel() else 0)
    loop = torch.arange(N).unsqueeze(0).repeat(2, 1)
    if edge_attr is not None:
        fill = torch.full((N,) + tuple(edge_attr.shape[1:]), 1.0 if fill_value is None else fill_value,
                          dtype=edge_attr.dtype)
        edge_attr = torch.cat([edge_attr, fill], 0)
    return torch.cat([edge_index, loop], 1), edge_attr


def remove_self_loops(edge_index, edge_attr=None):
    keep = edge_index[0] != edge_index[1]
    return edge_index[:, keep], None if edge_attr is None else edge_attr[keep]


UTILS = types.SimpleNamespace(softmax=softmax, scatter=scatter, degree=degree, add_self_loops=add_self_loops,
                              remove_self_loops=remove_self_loops)


# ---- the base class -------------------------------------------------------------------------------
class RefMessagePassing(torch.nn.Module):
    """The contract of gcm.nn.MessagePassing (source_to_target, one node set) restated: index_select for the gathers,
    the scatter above for the default aggregate."""

    def __init__(self, aggr="add", *, flow="source_to_target", node_dim=-2):
        super().__init__()
        assert flow == "source_to_target" and node_dim in (0, -2)
        assert aggr is None or aggr in ("add", "sum", "mean", "max", "min")
        self.aggr, self.flow, self.node_dim = aggr, flow, node_dim

    def message(self, x_j):
        return x_j

    def aggregate(self, inputs, index, ptr=None, dim_size=None):
        return scatter(inputs, index, dim=0, dim_size=dim_size, reduce=self.aggr)

    def update(self, inputs):
        return inputs

    def propagate(self, edge_index, size=None, **kwargs):
        M = None if size is None else size[0]
        fns = ((self.message, 0), (self.aggregate, 1), (self.update, 1))
        names = [[p for p in list(inspect.signature(fn).parameters.values())[skip:]] for fn, skip in fns]
        coll = {}
        for p in (p for ps in names for p in ps):
            name = p.name
            if name[-2:] in ("_i", "_j") and name[:-2] in kwargs:
                side = 0 if name.endswith("_j") else 1
                data = kwargs[name[:-2]]
                if isinstance(data, (tuple, list)):
                    data = data[side]
                if isinstance(data, torch.Tensor):
                    assert self.node_dim == 0 or data.dim() == 2
                    M = data.shape[0] if M is None else M
                    assert data.shape[0] == M
                    data = data.index_select(0, edge_index[side])
                coll[name] = data
            elif name in kwargs:
                coll[name] = kwargs[name]
        coll.update(edge_index=edge_index, edge_index_i=edge_index[1], edge_index_j=edge_index[0], index=edge_index[1],
                    ptr=None, size=(M, M), size_i=M, size_j=M, dim_size=M)

        def args_of(ps):
            return {p.name: coll[p.name] for p in ps if p.name in coll or p.default is inspect.Parameter.empty}

        out = self.message(**args_of(names[0]))
        out = self.aggregate(out, **args_of(names[1]))
        return self.update(out, **args_of(names[2]))


# ---- layer bodies, written once -----------------------------------------------------------------------
_LAYERS = {}


def layers(base, utils=UTILS):
    """A namespace of layers (GraphConv, GCN, GIN, EdgeConv, GATv2) subclassing `base`, with `utils`' functions."""
    if base in _LAYERS:
        return _LAYERS[base]

    class GraphConv(base):
        """gcm.nn.GraphConv's parameters; edge_weight passes through to message in the caller's edge order."""

        def __init__(self, in_channels, out_channels, aggr="add", bias=True):
            super().__init__(aggr=aggr)
            self.in_channels, self.out_channels = in_channels, out_channels
            self.lin_rel = torch.nn.Linear(in_channels, out_channels, bias=bias)
            self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=False)

        def forward(self, x, edge_index, edge_weight=None):
            out = self.propagate(edge_index, x=x, edge_weight=edge_weight)
            return self.lin_rel(out) + self.lin_root(x)

        def message(self, x_j, edge_weight):
            return x_j if edge_weight is None else edge_weight.view(-1, 1) * x_j

    class GCN(base):
        """Kipf & Welling: D^-1/2 (A + I) D^-1/2 X W + b, the norm computed with degree / add_self_loops and handed to
        message as a kwarg."""

        def __init__(self, in_channels, out_channels):
            super().__init__(aggr="add")
            self.in_channels, self.out_channels = in_channels, out_channels
            self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
            self.bias = torch.nn.Parameter(torch.zeros(out_channels))

        def forward(self, x, edge_index):
            M = x.shape[0]
            edge_index, _ = utils.add_self_loops(edge_index, num_nodes=M)
            row, col = edge_index[0], edge_index[1]
            deg = utils.degree(col, M, dtype=x.dtype)
            dis = deg.pow(-0.5)
            dis = dis.masked_fill(dis == float("inf"), 0)
            norm = dis[row] * dis[col]
            return self.propagate(edge_index, x=self.lin(x), norm=norm) + self.bias

        def message(self, x_j, norm):
            return norm.view(-1, 1) * x_j

    class GIN(base):
        """gcm.nn.GINConv's parameters (eps [1], nn.*)."""

        def __init__(self, nn, eps=0.0, train_eps=False):
            super().__init__(aggr="add")
            self.nn = nn
            if train_eps:
                self.eps = torch.nn.Parameter(torch.full((1,), float(eps)))
            else:
                self.register_buffer("eps", torch.full((1,), float(eps)))

        def forward(self, x, edge_index):
            return self.nn((1 + self.eps) * x + self.propagate(edge_index, x=x))

    class EdgeConv(base):
        """Dynamic Graph CNN's layer: max over the in-edges of nn([x_i, x_j - x_i])."""

        def __init__(self, nn):
            super().__init__(aggr="max")
            self.nn = nn

        def forward(self, x, edge_index):
            return self.propagate(edge_index, x=x)

        def message(self, x_i, x_j):
            return self.nn(torch.cat([x_i, x_j - x_i], dim=-1))

    class GATv2(base):
        """Brody et al., "How Attentive are Graph Attention Networks?": e_ij = a^T LeakyReLU(W_l x_j + W_r x_i),
        alpha = softmax over the in-edges of i, out_i = sum_j alpha_ij W_l x_j, heads concatenated.  The edges are used
        as given.  [M, H, C] tensors, gathered along dim 0."""

        def __init__(self, in_channels, out_channels, heads=1, negative_slope=0.2):
            super().__init__(aggr="add", node_dim=0)
            self.in_channels, self.out_channels, self.heads, self.slope = in_channels, out_channels, heads, negative_slope
            self.lin_l = torch.nn.Linear(in_channels, heads * out_channels)
            self.lin_r = torch.nn.Linear(in_channels, heads * out_channels)
            self.att = torch.nn.Parameter(torch.randn(1, heads, out_channels) * 0.5)
            self.bias = torch.nn.Parameter(torch.zeros(heads * out_channels))

        def forward(self, x, edge_index):
            H, C = self.heads, self.out_channels
            x_l, x_r = self.lin_l(x).view(-1, H, C), self.lin_r(x).view(-1, H, C)
            out = self.propagate(edge_index, x=(x_l, x_r))
            return out.reshape(-1, H * C) + self.bias

        def message(self, x_j, x_i, index, ptr, size_i):
            e = torch.nn.functional.leaky_relu(x_i + x_j, self.slope)
            alpha = utils.softmax((e * self.att).sum(dim=-1), index, ptr, size_i)
            return x_j * alpha.unsqueeze(-1)

    _LAYERS[base] = types.SimpleNamespace(GraphConv=GraphConv, GCN=GCN, GIN=GIN, EdgeConv=EdgeConv, GATv2=GATv2)
    return _LAYERS[base]
