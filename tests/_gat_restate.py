"""Eager restatement of PyG's DenseGATConv and GATConv (GAT v1: the contract gcm.nn's layers implement),
dtype generic so the tests can evaluate it in float64 to bound the kernels' fp32 error.  One departure from
eager PyG, which the layers share: a row with nothing to attend to aggregates nothing (its output is bias),
where PyG's dense formula gives NaN."""
import torch
import torch.nn.functional as F


def _heads(out, bias, concat):
    out = out.flatten(-2) if concat else out.mean(-2)
    return out if bias is None else out + bias


def dense_gat(x, adj, weight, att_src, att_dst, bias=None, heads=1, concat=True, negative_slope=0.2, mask=None,
              add_loop=True):
    """adj[b, i, j] != 0: i attends to j (only the pattern matters; the diagonal is set when add_loop)."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    B, N, _ = x.shape
    A = adj.detach().expand(B, N, N) != 0
    if add_loop:
        A = A.clone()
        idx = torch.arange(N)
        A[:, idx, idx] = True
    H = heads
    C = weight.shape[0] // H
    y = (x @ weight.t()).view(B, N, H, C)
    s_src = (y * att_src.reshape(H, C)).sum(-1)                        # [B, N, H]
    s_dst = (y * att_dst.reshape(H, C)).sum(-1)
    e = F.leaky_relu(s_dst.unsqueeze(2) + s_src.unsqueeze(1), negative_slope)   # [B, i, j, H]
    on = A.unsqueeze(-1)
    emax = e.masked_fill(~on, float("-inf")).amax(2, keepdim=True).detach()
    emax = torch.where(torch.isinf(emax), torch.zeros_like(emax), emax)
    p = torch.exp(e - emax) * on
    l = p.sum(2, keepdim=True)
    alpha = p / torch.where(l > 0, l, torch.ones_like(l))
    out = _heads(torch.einsum("bijh,bjhc->bihc", alpha, y), bias, concat)
    if mask is not None:
        out = out * mask.view(B, N, 1).to(out.dtype)
    return out


def gat(x, edge_index, weight, att_src, att_dst, bias=None, heads=1, concat=True, negative_slope=0.2,
        add_self_loops=True):
    """edge_index [2, E] = (source, sink); with add_self_loops every i -> i edge is removed and one loop per
    node appended; duplicate edges are separate terms of the softmax."""
    M = x.shape[0]
    src, dst = edge_index[0], edge_index[1]
    if add_self_loops:
        keep = src != dst
        loops = torch.arange(M)
        src, dst = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
    H = heads
    C = weight.shape[0] // H
    y = (x @ weight.t()).view(M, H, C)
    s_src = (y * att_src.reshape(H, C)).sum(-1)                        # [M, H]
    s_dst = (y * att_dst.reshape(H, C)).sum(-1)
    e = F.leaky_relu(s_dst[dst] + s_src[src], negative_slope)          # [E, H]
    idx = dst.unsqueeze(-1).expand(-1, H)
    emax = torch.full((M, H), float("-inf"), dtype=x.dtype).scatter_reduce(0, idx, e.detach(), "amax")
    emax = torch.where(torch.isinf(emax), torch.zeros_like(emax), emax)
    p = torch.exp(e - emax[dst])
    l = torch.zeros(M, H, dtype=x.dtype).index_add(0, dst, p)
    alpha = p / l[dst]
    out = torch.zeros(M, H, C, dtype=x.dtype).index_add(0, dst, alpha.unsqueeze(-1) * y[src])
    return _heads(out, bias, concat)


class _GATRefBase(torch.nn.Module):
    def __init__(self, cin, cout, heads, concat, negative_slope, bias, att_shape):
        super().__init__()
        self.heads, self.concat, self.negative_slope = heads, concat, negative_slope
        self.lin = torch.nn.Linear(cin, heads * cout, bias=False)
        self.att_src = torch.nn.Parameter(torch.randn(att_shape) * 0.5)
        self.att_dst = torch.nn.Parameter(torch.randn(att_shape) * 0.5)
        self.bias = torch.nn.Parameter(torch.zeros(heads * cout if concat else cout)) if bias else None


class DenseGATRef(_GATRefBase):
    """Parameter layout of gcm.nn.DenseGATConv (lin.weight, att_src / att_dst [1, 1, H, C], bias)."""

    def __init__(self, cin, cout, heads=1, concat=True, negative_slope=0.2, bias=True):
        super().__init__(cin, cout, heads, concat, negative_slope, bias, (1, 1, heads, cout))

    def forward(self, x, adj, mask=None, add_loop=True):
        return dense_gat(x, adj, self.lin.weight, self.att_src, self.att_dst, self.bias, self.heads, self.concat,
                         self.negative_slope, mask, add_loop)


class GATRef(_GATRefBase):
    """Parameter layout of gcm.nn.GATConv (lin.weight, att_src / att_dst [1, H, C], bias)."""

    def __init__(self, cin, cout, heads=1, concat=True, negative_slope=0.2, add_self_loops=True, bias=True):
        super().__init__(cin, cout, heads, concat, negative_slope, bias, (1, heads, cout))
        self.add_self_loops = add_self_loops

    def forward(self, x, edge_index, edge_attr=None):
        return gat(x, edge_index, self.lin.weight, self.att_src, self.att_dst, self.bias, self.heads, self.concat,
                   self.negative_slope, self.add_self_loops)
