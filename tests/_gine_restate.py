"""Eager restatement of PyG's GINEConv, of its dense twin and of RelativeEdgeAttr (the contract gcm.nn's classes
implement), dtype generic so the tests can evaluate it in float64 to bound the kernels' fp32 error; and the quantised
test inputs that keep every ReLU argument off the kink by construction."""
import torch


def gine(x, edge_index, edge_attr, eps, nn, lin=None):
    """edge_index [2, E] = (source, sink), used as given; edge_attr [E, D] in edge_index order."""
    src, dst = edge_index[0], edge_index[1]
    e = edge_attr if lin is None else lin(edge_attr)
    if e.shape[-1] != x.shape[-1]:
        raise ValueError("Node and edge feature dimensionalities do not match. Consider setting the 'edge_dim' "
                         "attribute of 'GINEConv'")
    agg = torch.zeros_like(x).index_add(0, dst, torch.relu(x[src] + e))
    return nn((1 + eps) * x + agg)


def dense_gine(x, adj, edge_attr, eps, nn, lin=None, mask=None, add_loop=True):
    """adj[b, i, j]: i aggregates from j; the values of adj are weights, an entry equal to 0 is no edge, the diagonal
    is an ordinary entry.  edge_attr [B, N, N, D] is read at the set entries only, unless adj needs a gradient: that
    is then the derivative at every entry and every entry of edge_attr counts."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    edge_attr = edge_attr.unsqueeze(0) if edge_attr.dim() == 3 else edge_attr
    B, N, _ = x.shape
    adj, edge_attr = adj.expand(B, N, N), edge_attr.expand(B, N, N, -1)
    if not adj.requires_grad:
        edge_attr = torch.where((adj != 0).unsqueeze(-1), edge_attr, torch.zeros((), dtype=x.dtype))
    e = edge_attr if lin is None else lin(edge_attr)
    msg = torch.relu(x.unsqueeze(1) + e)                      # [b, i, j, :] = relu(x[b, j] + e[b, i, j])
    out = (adj.unsqueeze(-1) * msg).sum(2)
    if add_loop:
        out = (1 + eps) * x + out
    out = nn(out)
    if mask is not None:
        out = out * mask.reshape(B, N, 1).to(out.dtype)
    return out


def infer_in_channels(nn):
    first = nn[0] if isinstance(nn, torch.nn.Sequential) else nn
    if hasattr(first, "in_features"):
        return first.in_features
    if hasattr(first, "in_channels"):
        return first.in_channels
    raise ValueError("Could not infer input channels from `nn`.")


class _GINERefBase(torch.nn.Module):
    """Parameter layout of gcm.nn.GINEConv / DenseGINEConv (eps [1], nn.*, lin.{weight,bias} with edge_dim)."""

    def __init__(self, nn, eps=0.0, train_eps=False, edge_dim=None):
        super().__init__()
        self.initial_eps, self.edge_dim = float(eps), edge_dim
        self.lin = None if edge_dim is None else torch.nn.Linear(edge_dim, infer_in_channels(nn))
        self.nn = nn
        if train_eps:
            self.eps = torch.nn.Parameter(torch.full((1,), float(eps)))
        else:
            self.register_buffer("eps", torch.full((1,), float(eps)))


class GINERef(_GINERefBase):
    def forward(self, x, edge_index, edge_attr):
        return gine(x, edge_index, edge_attr, self.eps, self.nn, self.lin)


class DenseGINERef(_GINERefBase):
    def forward(self, x, adj, edge_attr, mask=None, add_loop=True):
        return dense_gine(x, adj, edge_attr, self.eps, self.nn, self.lin, mask, add_loop)


def _pose(x, pose_slice):
    if pose_slice is None:
        return x[..., :0]
    return x[..., pose_slice]


def rel_edge_attr(x, edge_index, time=True, pose_slice=None, time_scale=1.0):
    """[E, D]: row k = [(sink_k - source_k) * time_scale, x[source_k, ps] - x[sink_k, ps]]."""
    src, dst = edge_index[0], edge_index[1]
    cols = [((dst - src).to(x.dtype) * time_scale).unsqueeze(-1)] if time else []
    p = _pose(x, pose_slice)
    return torch.cat(cols + [p[src] - p[dst]], -1)


def dense_rel_edge_attr(x, time=True, pose_slice=None, time_scale=1.0):
    """[B, N, N, D]: entry (b, i, j) = [(i - j) * time_scale, x[b, j, ps] - x[b, i, ps]]."""
    B, N, _ = x.shape
    n = torch.arange(N)
    cols = [((n.view(N, 1) - n.view(1, N)).to(x.dtype) * time_scale).view(1, N, N, 1).expand(B, N, N, 1)] if time else []
    p = _pose(x, pose_slice)
    return torch.cat(cols + [p.unsqueeze(1) - p.unsqueeze(2)], -1)


class RelativeEdgeAttrRef(torch.nn.Module):
    def __init__(self, time=True, pose_slice=None, time_scale=1.0):
        super().__init__()
        self.time, self.pose_slice, self.time_scale = time, pose_slice, time_scale

    def forward(self, x, edges):
        if x.dim() == 2:
            return rel_edge_attr(x, edges, self.time, self.pose_slice, self.time_scale)
        return dense_rel_edge_attr(x, self.time, self.pose_slice, self.time_scale)


# ---------------------------------------------------------------------------
# quantised inputs.  With edge_dim: x in eighths, edge_attr and W_e in quarters, b_e in sixteenths + 1/32, all small
# integers over those denominators: every x_j + W_e a + b_e is a multiple of 1/16 plus 1/32, exact in fp32 in any
# summation order, at least 1/32 from the kink.  Without: x in eighths, edge_attr in eighths + 1/16.
# ---------------------------------------------------------------------------
def quant(shape, denom, lim, gen, offset=0.0):
    return torch.randint(-lim, lim + 1, shape, generator=gen).double() / denom + offset


def quant_lin(lin, gen, half_cols=()):
    """lin's parameters overwritten in place with quantised ones (columns `half_cols` of the weight in halves: for
    edge features that are in eighths themselves, such as a pose offset of eighth-quantised observations)."""
    with torch.no_grad():
        w = quant(tuple(lin.weight.shape), 4, 4, gen)
        for c in half_cols:
            w[:, c] = quant((w.shape[0],), 2, 2, gen)
        lin.weight.copy_(w)
        lin.bias.copy_(quant(tuple(lin.bias.shape), 16, 8, gen, 1 / 32))


# (M, E, F, D); D None: the no-lin form
SPARSE_CASES = [(1, 0, 3, 2), (7, 15, 3, 1), (40, 90, 8, 5), (33, 200, 32, 4), (20, 60, 65, 3), (20, 60, 128, 32),
                (40, 90, 6, None)]


def sparse_case(M, E, F, D, seed=0):
    """-> (x [M,F], edge_index [2,E], edge_attr [E,D or F]) in float64; duplicates, self edges and isolated nodes."""
    gen = torch.Generator().manual_seed(1000 + seed + 7 * M + E + F)
    x = quant((M, F), 8, 16, gen)
    hi = max(M - 3, 1)                                        # the last nodes stay isolated
    ei = torch.randint(0, hi, (2, E), generator=gen)
    if E >= 8:
        ei[:, 1] = ei[:, 0]                                   # a duplicate
        ei[1, 2] = ei[0, 2]                                   # a self edge
        ei[:, 3] = ei[:, 2]                                   # twice
    ea = quant((E, D), 4, 8, gen) if D is not None else quant((E, F), 8, 16, gen, 1 / 16)
    return x, ei, ea


# (B, N, F, D, options)
DENSE_CASES = [(3, 7, 3, 2, {}), (5, 1, 4, 1, {}), (3, 33, 8, 3, {"mask": True}), (2, 40, 16, 4, {"add_loop": False}),
               (2, 130, 64, 4, {"weighted": True}), (2, 20, 128, 8, {}), (1, 20, 6, 2, {"two_d": True}),
               (4, 20, 6, 2, {"broadcast": True})]


def dense_case(B, N, F, D, opts, seed=0):
    """-> (x, adj, edge_attr, mask | None) in float64 in the shapes the options ask for."""
    gen = torch.Generator().manual_seed(2000 + seed + 7 * B + N + F)
    Ba = 1 if opts.get("broadcast") else B
    x = quant((B, N, F), 8, 16, gen)
    adj = (torch.rand(Ba, N, N, generator=gen) < 0.3).double()
    if N > 2:
        adj[:, 2] = 0                                         # an empty row
        adj[:, 1, 1] = 1                                      # a diagonal entry
    if opts.get("weighted"):
        adj = adj * quant((Ba, N, N), 4, 8, gen, 1 / 8)       # both signs, never 0
    ea = quant((Ba, N, N, D), 4, 8, gen)
    mask = (torch.rand(B, N, generator=gen) < 0.7) if opts.get("mask") else None
    if opts.get("two_d"):
        x, adj, ea = x[0], adj[0], ea[0]
    return x, adj, ea, mask


def min_abs_pre(x, src, e):
    """min |x_j + e_k| over edges and channels (inf without an edge)."""
    pre = x[src] + e
    return float(pre.abs().min()) if pre.numel() else float("inf")
