"""Eager restatements of PyG's TransformerConv with edge_dim and of its dense form (the contract gcm.transformer's layers
implement), dtype generic so the tests can evaluate them in float64 to bound the kernels' fp32 error.

Two forms.  The per-edge form is PyG's `message` body: e_k = lin_edge(edge_attr[k]) is formed for every edge and added
to the key and to the value.  It is written so that with e = 0 it runs tests/_transformer_restate.py's operations in
the same order (the edge-free bits).  The factored form is the algebra the kernels use (lin_edge applied per node, not
per edge) with its backward written out by hand; the tests hold it against autograd of the per-edge form.
The departures from eager PyG are _transformer_restate's: a node with nothing to attend to aggregates nothing, and the
softmax denominator carries no +1e-16.  Also the case tables of the GPU tests."""
import math

import torch

from _transformer_restate import _finish, _lin


# ---------------------------------------------------------------------------
# the per-edge form
# ---------------------------------------------------------------------------
def transformer_edge(x, edge_index, edge_attr, wq, bq, wk, bk, wv, bv, w_e, w_skip=None, b_skip=None, w_beta=None,
                     heads=1, concat=True):
    """edge_index [2, E] = (source, sink), used as given; edge_attr [E, D] in its order; w_e [H*C, D]."""
    M = x.shape[0]
    src, dst = edge_index[0], edge_index[1]
    H = heads
    C = wq.shape[0] // H
    q, k, v = (_lin(x, w, b).view(M, H, C) for w, b in ((wq, bq), (wk, bk), (wv, bv)))
    e = (edge_attr @ w_e.t()).view(-1, H, C)                           # [E, H, C]: per edge, on purpose
    s = (q[dst] * (k[src] + e)).sum(-1) / math.sqrt(C)                 # [E, H]
    idx = dst.unsqueeze(-1).expand(-1, H)
    smax = torch.full((M, H), float("-inf"), dtype=x.dtype).scatter_reduce(0, idx, s.detach(), "amax")
    smax = torch.where(torch.isinf(smax), torch.zeros_like(smax), smax)
    p = torch.exp(s - smax[dst])
    l = torch.zeros(M, H, dtype=x.dtype).index_add(0, dst, p)
    alpha = p / l[dst]
    o = torch.zeros(M, H, C, dtype=x.dtype).index_add(0, dst, alpha.unsqueeze(-1) * (v[src] + e))
    r = None if w_skip is None else _lin(x, w_skip, b_skip)
    return _finish(o, r, w_beta, concat)


def dense_transformer_edge(x, adj, edge_attr, wq, bq, wk, bk, wv, bv, w_e, w_skip=None, b_skip=None, w_beta=None,
                           heads=1, concat=True, mask=None, add_loop=False):
    """adj[b, i, j] != 0: i attends to j (only the pattern matters; the diagonal is a term when add_loop, with the
    feature edge_attr[b, i, i]).  edge_attr [B, N, N, D] is read at the terms only."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    edge_attr = edge_attr.unsqueeze(0) if edge_attr.dim() == 3 else edge_attr
    B, N, _ = x.shape
    A = adj.detach().expand(B, N, N) != 0
    if add_loop:
        A = A.clone()
        idx = torch.arange(N)
        A[:, idx, idx] = True
    H = heads
    C = wq.shape[0] // H
    on = A.unsqueeze(-1)
    a = torch.where(on, edge_attr.expand(B, N, N, -1), torch.zeros((), dtype=x.dtype))
    q, k, v = (_lin(x, w, b).view(B, N, H, C) for w, b in ((wq, bq), (wk, bk), (wv, bv)))
    e = (a @ w_e.t()).view(B, N, N, H, C)                              # per entry, on purpose
    s = torch.einsum("bihc,bjhc->bijh", q, k) / math.sqrt(C) + torch.einsum("bihc,bijhc->bijh", q, e) / math.sqrt(C)
    smax = s.masked_fill(~on, float("-inf")).amax(2, keepdim=True).detach()
    smax = torch.where(torch.isinf(smax), torch.zeros_like(smax), smax)
    p = torch.exp(s - smax) * on
    l = p.sum(2, keepdim=True)
    alpha = p / torch.where(l > 0, l, torch.ones_like(l))
    o = torch.einsum("bijh,bjhc->bihc", alpha, v) + torch.einsum("bijh,bijhc->bihc", alpha, e)
    r = None if w_skip is None else _lin(x, w_skip, b_skip)
    return _finish(o, r, w_beta, concat, mask)


class _Base(torch.nn.Module):
    """Parameter layout of gcm.transformer's layers (lin_key, lin_query, lin_value, lin_edge, lin_skip, lin_beta) and
    their constructor arguments."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None,
                 bias=True, root_weight=True):
        super().__init__()
        self.heads, self.concat, self.edge_dim = heads, concat, edge_dim
        width = heads * out_channels if concat else out_channels
        self.lin_key = torch.nn.Linear(in_channels, heads * out_channels)
        self.lin_query = torch.nn.Linear(in_channels, heads * out_channels)
        self.lin_value = torch.nn.Linear(in_channels, heads * out_channels)
        self.lin_edge = torch.nn.Linear(edge_dim, heads * out_channels, bias=False) if edge_dim is not None else None
        self.lin_skip = torch.nn.Linear(in_channels, width, bias=bias) if root_weight else None
        self.lin_beta = torch.nn.Linear(3 * width, 1, bias=False) if beta and root_weight else None

    def operands(self):
        skip, beta = self.lin_skip, self.lin_beta
        return dict(wq=self.lin_query.weight, bq=self.lin_query.bias, wk=self.lin_key.weight, bk=self.lin_key.bias,
                    wv=self.lin_value.weight, bv=self.lin_value.bias, w_e=self.lin_edge.weight,
                    w_skip=None if skip is None else skip.weight, b_skip=None if skip is None else skip.bias,
                    w_beta=None if beta is None else beta.weight, heads=self.heads, concat=self.concat)


class TransformerEdgeRef(_Base):
    def forward(self, x, edge_index, edge_attr):
        return transformer_edge(x, edge_index, edge_attr, **self.operands())


class DenseTransformerEdgeRef(_Base):
    def forward(self, x, adj, edge_attr, mask=None, add_loop=False):
        return dense_transformer_edge(x, adj, edge_attr, mask=mask, add_loop=add_loop, **self.operands())


# ---------------------------------------------------------------------------
# the factored form, forward and hand-written backward (no autograd)
# ---------------------------------------------------------------------------
def factored(x, edge_index, a, g, wq, bq, wk, bk, wv, bv, w_e, w_skip=None, b_skip=None, w_beta=None, heads=1,
             concat=True):
    """-> (out, gradients) with the gradients of sum(out * g) by hand, keyed x, edge_attr, wq, bq, wk, bk, wv, bv, w_e,
    w_skip, b_skip, w_beta.  Nothing per edge is wider than D = a.shape[1]."""
    with torch.no_grad():
        M, H = x.shape[0], heads
        C = wq.shape[0] // H
        D = a.shape[1]
        src, dst = edge_index[0], edge_index[1]
        sc = 1.0 / math.sqrt(C)
        We = w_e.view(H, C, D)
        q, k, v = (_lin(x, w, b).view(M, H, C) for w, b in ((wq, bq), (wk, bk), (wv, bv)))
        zeros = lambda *shape: torch.zeros(*shape, dtype=x.dtype)
        ax = a.unsqueeze(1)                                               # [E, 1, D]
        # forward
        u = sc * torch.einsum("mhc,hcd->mhd", q, We)
        s = sc * (q[dst] * k[src]).sum(-1) + (u[dst] * ax).sum(-1)
        idx = dst.unsqueeze(-1).expand(-1, H)
        smax = torch.full((M, H), float("-inf"), dtype=x.dtype).scatter_reduce(0, idx, s, "amax")
        smax = torch.where(torch.isinf(smax), torch.zeros_like(smax), smax)
        p = torch.exp(s - smax[dst])
        alpha = p / zeros(M, H).index_add(0, dst, p)[dst]
        abar = zeros(M, H, D).index_add(0, dst, alpha.unsqueeze(-1) * ax)
        o = zeros(M, H, C).index_add(0, dst, alpha.unsqueeze(-1) * v[src]) + torch.einsum("hcd,mhd->mhc", We, abar)
        om = o.flatten(-2) if concat else o.mean(-2)
        Do = om.shape[-1]
        r = None if w_skip is None else _lin(x, w_skip, b_skip)
        grads = {}
        # heads, skip and gate
        if r is None:
            out, g_om, g_r = om, g, None
        elif w_beta is None:
            out, g_om, g_r = om + r, g, g
        else:
            wb = w_beta.reshape(-1)
            t = torch.cat([om, r, om - r], -1)
            gate = torch.sigmoid(t @ wb).unsqueeze(-1)
            out = gate * r + (1 - gate) * om
            gl = (g * (r - om)).sum(-1, keepdim=True) * gate * (1 - gate)
            g_om = g * (1 - gate) + gl * (wb[:Do] + wb[2 * Do:])
            g_r = g * gate + gl * (wb[Do:2 * Do] - wb[2 * Do:])
            grads["w_beta"] = (gl * t).sum(0).view_as(w_beta)
        dO = g_om.view(M, H, C) if concat else (g_om / H).unsqueeze(1).expand(M, H, C)
        # attention
        w = torch.einsum("mhc,hcd->mhd", dO, We)
        dP = (dO[dst] * v[src]).sum(-1) + (w[dst] * ax).sum(-1)
        delta = zeros(M, H).index_add(0, dst, alpha * dP)
        dS = alpha * (dP - delta[dst])
        b = sc * zeros(M, H, D).index_add(0, dst, dS.unsqueeze(-1) * ax)
        dq = sc * zeros(M, H, C).index_add(0, dst, dS.unsqueeze(-1) * k[src]) + torch.einsum("hcd,mhd->mhc", We, b)
        dk = sc * zeros(M, H, C).index_add(0, src, dS.unsqueeze(-1) * q[dst])
        dv = zeros(M, H, C).index_add(0, src, alpha.unsqueeze(-1) * dO[dst])
        grads["edge_attr"] = (dS.unsqueeze(-1) * u[dst]).sum(1) + (alpha.unsqueeze(-1) * w[dst]).sum(1)
        grads["w_e"] = (torch.einsum("mhc,mhd->hcd", dO, abar) + torch.einsum("mhc,mhd->hcd", q, b)).reshape(H * C, D)
        # projections
        g_x = zeros(*x.shape)
        for name, wt, d in (("q", wq, dq), ("k", wk, dk), ("v", wv, dv)):
            d = d.reshape(M, H * C)
            g_x = g_x + d @ wt
            grads["w" + name], grads["b" + name] = d.t() @ x, d.sum(0)
        if g_r is not None:
            g_x = g_x + g_r @ w_skip
            grads["w_skip"] = g_r.t() @ x
            if b_skip is not None:
                grads["b_skip"] = g_r.sum(0)
        grads["x"] = g_x
        return out, grads


# ---------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------
# (M, E, Fi, H, C, D, options).  Every C that takes another lane-group width; the sixth: two channels per lane and both
# limits
SPARSE_CASES = [(40, 90, 8, 2, 8, 3, {}), (40, 90, 5, 1, 4, 1, {}), (33, 200, 16, 1, 16, 16, {}),
                (33, 200, 32, 1, 32, 4, {}), (20, 120, 64, 1, 64, 3, {}), (20, 120, 128, 1, 128, 32, {}),
                (20, 120, 32, 3, 8, 3, {"concat": False})]

# (B, N, Fi, H, C, D, options): a partial 32-tile; across the 128-row block; both limits
DENSE_CASES = [(3, 40, 8, 2, 8, 3, {}), (2, 130, 16, 4, 4, 4, {}), (2, 33, 32, 1, 128, 32, {})]


def case_id(case):
    return "-".join(str(c) for c in case[:6]) + "".join("-" + k for k in case[6])


def sparse_case(M, E, Fi, H, C, D, opts=None, seed=0):
    """-> (x [M,Fi], edge_index [2,E] in no particular order, edge_attr [E,D]) in float64.  Node 0 is a hub with at
    least 70 in-edges, the last three nodes have no in-edge (M - 2 is a source), there are a loop and a duplicated
    edge."""
    gen = torch.Generator().manual_seed(5000 + seed + 7 * M + E + Fi)
    assert E >= 80 and M >= 10
    x = torch.randn(M, Fi, generator=gen, dtype=torch.float64)
    src = torch.randint(0, M - 1, (E,), generator=gen)
    dst = torch.randint(0, M - 3, (E,), generator=gen)
    dst[:70] = 0
    src[70], dst[70] = 5, 5                                           # a loop
    src[72], dst[72] = src[71], dst[71]                               # a duplicate
    src[73] = M - 2
    ei = torch.stack([src, dst])[:, torch.randperm(E, generator=gen)]
    ea = torch.randn(E, D, generator=gen, dtype=torch.float64)
    return x, ei, ea


def dense_pattern(B, N, pattern):
    """band: TemporalBackedge([1,2,4])'s (i attends to i - 1, i - 2, i - 4); lower: the lower triangle with the
    diagonal.  Both with row 2 emptied and the last row full; odd graphs also have (3, 3) set."""
    i = torch.arange(N)
    adj = torch.zeros(B, N, N, dtype=torch.float64)
    if pattern == "band":
        for h in (1, 2, 4):
            adj[:, i[h:], i[h:] - h] = 1
    else:
        adj[:] = torch.tril(torch.ones(N, N, dtype=torch.float64))
    adj[:, 2] = 0
    adj[:, N - 1] = 1
    adj[1::2, 3, 3] = 1
    return adj


def dense_case(B, N, Fi, H, C, D, opts=None, pattern="band", seed=0):
    """-> (x [B,N,Fi], adj [B,N,N], edge_attr [B,N,N,D]) in float64."""
    gen = torch.Generator().manual_seed(6000 + seed + 7 * B + N + Fi)
    x = torch.randn(B, N, Fi, generator=gen, dtype=torch.float64)
    ea = torch.randn(B, N, N, D, generator=gen, dtype=torch.float64)
    return x, dense_pattern(B, N, pattern), ea


def layer_kwargs(case):
    """The constructor arguments of the case's layer (gcm.transformer's classes and the Ref ones take them)."""
    _, _, Fi, H, C, D, opts = case
    kw = dict(in_channels=Fi, out_channels=C, heads=H, edge_dim=D)
    kw.update({k: v for k, v in opts.items() if k in ("concat", "beta", "bias", "root_weight", "dropout")})
    return kw


# ---------------------------------------------------------------------------
# the same layer as a user would write it on a MessagePassing base class (PyG's message body): the unfused form, which
# forms lin_edge(edge_attr), the keys and the messages per edge
# ---------------------------------------------------------------------------
def mp_layer(base, softmax):
    """The class, on `base` (tests/_mp_restate.RefMessagePassing or gcm.nn.MessagePassing) and its segment softmax."""

    class TransformerEdgeMP(base):
        def __init__(self, in_channels, out_channels, heads=1, concat=True, edge_dim=None, root_weight=True):
            super().__init__(aggr="add", node_dim=0)
            self.heads, self.out_channels, self.concat = heads, out_channels, concat
            width = heads * out_channels if concat else out_channels
            self.lin_key = torch.nn.Linear(in_channels, heads * out_channels)
            self.lin_query = torch.nn.Linear(in_channels, heads * out_channels)
            self.lin_value = torch.nn.Linear(in_channels, heads * out_channels)
            self.lin_edge = torch.nn.Linear(edge_dim, heads * out_channels, bias=False)
            self.lin_skip = torch.nn.Linear(in_channels, width) if root_weight else None

        def forward(self, x, edge_index, edge_attr):
            H, C = self.heads, self.out_channels
            q, k, v = (lin(x).view(-1, H, C) for lin in (self.lin_query, self.lin_key, self.lin_value))
            out = self.propagate(edge_index, query=q, key=k, value=v, e=self.lin_edge(edge_attr).view(-1, H, C))
            out = out.reshape(-1, H * C) if self.concat else out.mean(1)
            return out if self.lin_skip is None else out + self.lin_skip(x)

        def message(self, query_i, key_j, value_j, e, index, size_i):
            alpha = (query_i * (key_j + e)).sum(-1) / math.sqrt(self.out_channels)
            alpha = softmax(alpha, index, None, size_i)
            return (value_j + e) * alpha.unsqueeze(-1)

    return TransformerEdgeMP
