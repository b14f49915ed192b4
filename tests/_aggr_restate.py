"""Eager restatement of the mean / max aggregation of gcm.nn's GraphConv(aggr=...), DenseGraphConv(aggr=...),
SAGEConv and DenseSAGEConv (the contract the kernels of csrc/aggrconv.hip implement), dtype generic so the tests can
evaluate it in float64 to bound the kernels' fp32 error.

Conventions: adj[b, i, j]: i aggregates from j; edge_index = (source, sink).
  dense mean:  agg_i  = (sum_j adj_ij x_j) / clamp(sum_j adj_ij, min=1)      adj values are weights
  dense max:   agg_ic = max over {j : adj_ij != 0} of x_jc, 0 for an empty row; ties: the lowest j
  sparse mean: agg_i  = sum_{e -> i} w_e x_src(e) / #{e -> i}, 0 without in-edges
  sparse max:  agg_ic = max over e -> i of w_e x_src(e),c, 0 without in-edges; ties: the first edge in CSR order
               (edges stably sorted by sink); duplicate edges are separate candidates
  out = lin_rel(agg) + lin_root(x), mask applied last (dense)."""
import torch
import torch.nn.functional as F


def dense_mean_agg(x, adj):
    return (adj @ x) / adj.sum(-1, keepdim=True).clamp(min=1)


def dense_max_agg(x, adj):
    """torch.argmax returns the first maximal index: the lowest j on a tie."""
    B, N, _ = x.shape
    step = max(1, (1 << 24) // max(1, N * N * x.shape[-1]))         # graphs per pass: bounds the [b, i, j, c] temporaries
    if B > step:
        return torch.cat([dense_max_agg(x[b:b + step], adj[b:b + step]) for b in range(0, B, step)])
    A = adj.detach() != 0                                           # [B, i, j]
    cand = x.unsqueeze(1).expand(B, N, N, x.shape[-1])              # [B, i, j, c] = x[b, j, c]
    neg = torch.full_like(cand, float("-inf"))
    win = torch.where(A.unsqueeze(-1), cand.detach(), neg).argmax(2, keepdim=True)     # [B, i, 1, c]
    agg = cand.gather(2, win).squeeze(2)
    return torch.where(A.any(-1, keepdim=True), agg, torch.zeros_like(agg))


def _dense_inputs(x, adj):
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    return x, adj.expand(x.shape[0], -1, -1)


def dense_aggr_conv(x, adj, w_rel, w_root=None, bias=None, aggr="mean", mask=None):
    """bias: the one bias of the layer, whichever linear carries it."""
    x, adj = _dense_inputs(x, adj)
    agg = dense_mean_agg(x, adj) if aggr == "mean" else dense_max_agg(x, adj)
    out = F.linear(agg, w_rel)
    if w_root is not None:
        out = out + F.linear(x, w_root)
    if bias is not None:
        out = out + bias
    if mask is not None:
        out = out * mask.view(x.shape[0], x.shape[1], 1).to(out.dtype)
    return out


def _padded(x, edge_index, edge_weight):
    """Candidates per destination in CSR order: cand [M, D, F] (w_e x_src), valid [M, D], D = the largest in-degree."""
    M, E = x.shape[0], edge_index.shape[1]
    order = torch.sort(edge_index[1], stable=True)[1]
    src, dst = edge_index[0][order], edge_index[1][order]
    count = torch.bincount(dst, minlength=M)
    D = max(int(count.max()) if E else 0, 1)
    start = torch.cumsum(count, 0) - count
    slot = torch.arange(E) - start[dst]
    msg = x[src] if edge_weight is None else edge_weight[order].unsqueeze(-1) * x[src]
    cand = torch.zeros(M, D, x.shape[1], dtype=x.dtype).index_put((dst, slot), msg)
    valid = torch.zeros(M, D, dtype=torch.bool).index_put((dst, slot), torch.ones(E, dtype=torch.bool))
    return cand, valid, count


def sparse_mean_agg(x, edge_index, edge_weight=None):
    M = x.shape[0]
    src, dst = edge_index[0], edge_index[1]
    msg = x[src] if edge_weight is None else edge_weight.unsqueeze(-1) * x[src]
    total = torch.zeros(M, x.shape[1], dtype=x.dtype).index_add(0, dst, msg)
    count = torch.bincount(dst, minlength=M).clamp(min=1)
    return total / count.unsqueeze(-1).to(x.dtype)


def sparse_max_agg(x, edge_index, edge_weight=None):
    cand, valid, count = _padded(x, edge_index, edge_weight)
    neg = torch.full_like(cand, float("-inf"))
    win = torch.where(valid.unsqueeze(-1), cand.detach(), neg).argmax(1, keepdim=True)
    agg = cand.gather(1, win).squeeze(1)
    return torch.where((count > 0).unsqueeze(-1), agg, torch.zeros_like(agg))


def sparse_max_margin(x, edge_index, edge_weight=None):
    """[M, F] relative gap between the two largest candidates of every (node, channel), inf with fewer than two."""
    cand, valid, _ = _padded(x.double(), edge_index, None if edge_weight is None else edge_weight.double())
    cand = torch.where(valid.unsqueeze(-1), cand, torch.full_like(cand, float("-inf")))
    if cand.shape[1] < 2:
        return torch.full(cand[:, 0].shape, float("inf"), dtype=torch.float64)
    top = cand.topk(2, dim=1).values
    gap = (top[:, 0] - top[:, 1]) / top[:, 0].abs().clamp(min=1e-30)
    return torch.where(torch.isfinite(top[:, 1]), gap, torch.full_like(gap, float("inf")))


def sparse_aggr_conv(x, edge_index, w_rel, w_root=None, bias=None, edge_weight=None, aggr="mean"):
    if edge_weight is not None and edge_weight.numel() != edge_index.shape[1]:
        edge_weight = None                                  # PyG: a weight vector of the wrong length is ignored
    agg = (sparse_mean_agg if aggr == "mean" else sparse_max_agg)(x, edge_index, edge_weight)
    out = F.linear(agg, w_rel)
    if w_root is not None:
        out = out + F.linear(x, w_root)
    return out if bias is None else out + bias


class DenseGraphConvRef(torch.nn.Module):
    """Parameter layout of gcm.nn.DenseGraphConv (lin_rel.{weight,bias}, lin_root.weight)."""

    def __init__(self, cin, cout, aggr="mean", bias=True):
        super().__init__()
        self.aggr = aggr
        self.lin_rel = torch.nn.Linear(cin, cout, bias=bias)
        self.lin_root = torch.nn.Linear(cin, cout, bias=False)

    def forward(self, x, adj, mask=None):
        return dense_aggr_conv(x, adj, self.lin_rel.weight, self.lin_root.weight, self.lin_rel.bias, self.aggr, mask)


class GraphConvRef(torch.nn.Module):
    """Parameter layout of gcm.nn.GraphConv."""

    def __init__(self, cin, cout, aggr="mean", bias=True):
        super().__init__()
        self.aggr = aggr
        self.lin_rel = torch.nn.Linear(cin, cout, bias=bias)
        self.lin_root = torch.nn.Linear(cin, cout, bias=False)

    def forward(self, x, edge_index, edge_weight=None):
        return sparse_aggr_conv(x, edge_index, self.lin_rel.weight, self.lin_root.weight, self.lin_rel.bias,
                                edge_weight, self.aggr)


class DenseSAGERef(torch.nn.Module):
    """Parameter layout of gcm.nn.DenseSAGEConv (lin_rel.weight, lin_root.{weight,bias})."""

    def __init__(self, cin, cout, bias=True):
        super().__init__()
        self.lin_rel = torch.nn.Linear(cin, cout, bias=False)
        self.lin_root = torch.nn.Linear(cin, cout, bias=bias)

    def forward(self, x, adj, mask=None):
        return dense_aggr_conv(x, adj, self.lin_rel.weight, self.lin_root.weight, self.lin_root.bias, "mean", mask)


class SAGERef(torch.nn.Module):
    """Parameter layout of gcm.nn.SAGEConv (lin_l.{weight,bias}, lin_r.weight)."""

    def __init__(self, cin, cout, aggr="mean", root_weight=True, bias=True):
        super().__init__()
        self.aggr, self.root_weight = aggr, root_weight
        self.lin_l = torch.nn.Linear(cin, cout, bias=bias)
        if root_weight:
            self.lin_r = torch.nn.Linear(cin, cout, bias=False)

    def forward(self, x, edge_index):
        return sparse_aggr_conv(x, edge_index, self.lin_l.weight, self.lin_r.weight if self.root_weight else None,
                                self.lin_l.bias, None, self.aggr)


def random_edges(M, E, seed, extras=True):
    """[2, E (+5)] random (source, sink) pairs; the last 3 nodes stay isolated.  extras: duplicate loops (0, 0) and a
    duplicate edge 1 -> 2 in the middle of the list."""
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, M - 3), (2, E), generator=gen)
    if E and extras and M > 5:
        extra = torch.tensor([[0, 1, 0, 2, 1], [0, 2, 0, 2, 2]])
        ei = torch.cat([ei[:, : E // 2], extra, ei[:, E // 2:]], 1)
    return ei


def weighted_max_case(M, E, Fi, seed):
    """(x [M, Fi], edge_index, edge_weight) of a weighted sparse-max test: weights of both signs, away from 0."""
    ei = random_edges(M, E, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(M, Fi, generator=gen)
    w = (torch.rand(ei.shape[1], generator=gen) + 0.25) * (torch.randint(0, 4, (ei.shape[1],), generator=gen) > 0).float().mul(2).sub(1)
    return x, ei, w
