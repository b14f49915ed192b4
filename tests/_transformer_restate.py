"""Eager restatement of PyG's TransformerConv (without edge features) and of its dense form (the contract gcm.nn's
TransformerConv / DenseTransformerConv implement), dtype generic so the tests can evaluate it in float64 to bound the
kernels' fp32 error.  Two departures from eager PyG, which the layers share: a node with nothing to attend to
aggregates nothing (its output is the skip term, or 0), and the softmax denominator carries no +1e-16."""
import math

import torch


def _finish(o, r, w_beta, concat, mask=None):
    """o [.., H, C] -> heads concatenated or averaged, then the skip r and the gate w_beta [1, 3 D]."""
    o = o.flatten(-2) if concat else o.mean(-2)
    if r is not None:
        if w_beta is not None:
            b = torch.sigmoid(torch.cat([o, r, o - r], -1) @ w_beta.reshape(-1, 1))
            o = b * r + (1 - b) * o
        else:
            o = o + r
    if mask is not None:
        o = o * mask.view(*o.shape[:-1], 1).to(o.dtype)
    return o


def _lin(x, w, b):
    return x @ w.t() if b is None else x @ w.t() + b


def dense_transformer(x, adj, wq, bq, wk, bk, wv, bv, w_skip=None, b_skip=None, w_beta=None, heads=1, concat=True,
                      mask=None, add_loop=False):
    """adj[b, i, j] != 0: i attends to j (only the pattern matters; the diagonal is set when add_loop).  w_skip None:
    no root term."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    B, N, _ = x.shape
    A = adj.detach().expand(B, N, N) != 0
    if add_loop:
        A = A.clone()
        idx = torch.arange(N)
        A[:, idx, idx] = True
    H = heads
    C = wq.shape[0] // H
    q, k, v = (_lin(x, w, b).view(B, N, H, C) for w, b in ((wq, bq), (wk, bk), (wv, bv)))
    s = torch.einsum("bihc,bjhc->bijh", q, k) / math.sqrt(C)
    on = A.unsqueeze(-1)
    smax = s.masked_fill(~on, float("-inf")).amax(2, keepdim=True).detach()
    smax = torch.where(torch.isinf(smax), torch.zeros_like(smax), smax)
    p = torch.exp(s - smax) * on
    l = p.sum(2, keepdim=True)
    alpha = p / torch.where(l > 0, l, torch.ones_like(l))
    o = torch.einsum("bijh,bjhc->bihc", alpha, v)
    r = None if w_skip is None else _lin(x, w_skip, b_skip)
    return _finish(o, r, w_beta, concat, mask)


def transformer(x, edge_index, wq, bq, wk, bk, wv, bv, w_skip=None, b_skip=None, w_beta=None, heads=1, concat=True):
    """edge_index [2, E] = (source, sink), used as given: loops and duplicates are ordinary terms of the softmax."""
    M = x.shape[0]
    src, dst = edge_index[0], edge_index[1]
    H = heads
    C = wq.shape[0] // H
    q, k, v = (_lin(x, w, b).view(M, H, C) for w, b in ((wq, bq), (wk, bk), (wv, bv)))
    s = (q[dst] * k[src]).sum(-1) / math.sqrt(C)                       # [E, H]
    idx = dst.unsqueeze(-1).expand(-1, H)
    smax = torch.full((M, H), float("-inf"), dtype=x.dtype).scatter_reduce(0, idx, s.detach(), "amax")
    smax = torch.where(torch.isinf(smax), torch.zeros_like(smax), smax)
    p = torch.exp(s - smax[dst])
    l = torch.zeros(M, H, dtype=x.dtype).index_add(0, dst, p)
    alpha = p / l[dst]
    o = torch.zeros(M, H, C, dtype=x.dtype).index_add(0, dst, alpha.unsqueeze(-1) * v[src])
    r = None if w_skip is None else _lin(x, w_skip, b_skip)
    return _finish(o, r, w_beta, concat)


class _TransformerRefBase(torch.nn.Module):
    """Parameter layout of gcm.nn.TransformerConv / DenseTransformerConv (lin_key, lin_query, lin_value, lin_skip,
    lin_beta)."""

    def __init__(self, cin, cout, heads=1, concat=True, beta=False, bias=True, root_weight=True):
        super().__init__()
        self.heads, self.concat = heads, concat
        width = heads * cout if concat else cout
        self.lin_key = torch.nn.Linear(cin, heads * cout)
        self.lin_query = torch.nn.Linear(cin, heads * cout)
        self.lin_value = torch.nn.Linear(cin, heads * cout)
        self.lin_skip = torch.nn.Linear(cin, width, bias=bias) if root_weight else None
        self.lin_beta = torch.nn.Linear(3 * width, 1, bias=False) if beta and root_weight else None

    def operands(self):
        skip, beta = self.lin_skip, self.lin_beta
        return (self.lin_query.weight, self.lin_query.bias, self.lin_key.weight, self.lin_key.bias,
                self.lin_value.weight, self.lin_value.bias, None if skip is None else skip.weight,
                None if skip is None else skip.bias, None if beta is None else beta.weight)


class DenseTransformerRef(_TransformerRefBase):
    def forward(self, x, adj, mask=None, add_loop=False):
        return dense_transformer(x, adj, *self.operands(), heads=self.heads, concat=self.concat, mask=mask,
                                 add_loop=add_loop)


class TransformerRef(_TransformerRefBase):
    def forward(self, x, edge_index, edge_attr=None):
        return transformer(x, edge_index, *self.operands(), heads=self.heads, concat=self.concat)
