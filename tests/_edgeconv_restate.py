"""Eager restatement of EdgeConv (Wang et al., Dynamic Graph CNN; PyG's EdgeConv, aggr="max") - the contract gcm.nn's
EdgeConv and DenseEdgeConv implement - in plain torch and dtype generic, in the LITERAL form: gather [x_i, x_j - x_i]
for every edge, run `nn` on it, take the per-channel maximum over a node's in-edges (0 for a node without any; of
equal messages the first wins: the lowest source index / the first edge of the node in the list's order).  The dense
and the sparse form are written independently of each other and of gcm.  Also the margins the GPU cases are chosen
by: how close the two best messages of a (sink, channel) are, and how close a pre-activation is to the kink."""
import torch


def make_nn(F, H, C, act="relu", bias=True):
    """Linear(2F -> H), ReLU | LeakyReLU(0.2), Linear(H -> C) with W1 ~ N(0, 1/2F), W2 ~ N(0, 1/H), biases 0.1 N(0,1)."""
    a = torch.nn.ReLU() if act == "relu" else torch.nn.LeakyReLU(0.2)
    nn = torch.nn.Sequential(torch.nn.Linear(2 * F, H, bias=bias), a, torch.nn.Linear(H, C, bias=bias))
    with torch.no_grad():
        nn[0].weight.copy_(torch.randn(H, 2 * F) * (2 * F) ** -0.5)
        nn[2].weight.copy_(torch.randn(C, H) * H ** -0.5)
        if bias:
            nn[0].bias.copy_(0.1 * torch.randn(H))
            nn[2].bias.copy_(0.1 * torch.randn(C))
    return nn


def dense_messages(x, nn):
    """m[b,i,j,:] = nn([x_i, x_j - x_i]) for every pair: [B,N,N,C]."""
    B, N, F = x.shape
    xi = x.unsqueeze(2).expand(B, N, N, F)
    xj = x.unsqueeze(1).expand(B, N, N, F)
    return nn(torch.cat([xi, xj - xi], -1))


def _act2(nn, pre):
    return nn[2](nn[1](pre))


def dense_messages_decomposed(x, nn):
    """The same messages through the split of the first Linear the kernels use: nn[2](act(P_i + Q_j))."""
    P, Q = decomposed_pre(x, nn)
    return _act2(nn, P.unsqueeze(2) + Q.unsqueeze(1))


def dense_edgeconv(x, adj, nn, with_winner=False, decomposed=False):
    """x [B,N,F], adj [B,N,N] (adj[b,i,j] != 0: i receives from j; the values do not matter)."""
    B, N, _ = x.shape
    m = dense_messages_decomposed(x, nn) if decomposed else dense_messages(x, nn)
    pat = (adj != 0).expand(B, N, N).unsqueeze(-1)
    idx = m.detach().masked_fill(~pat, float("-inf")).argmax(dim=2, keepdim=True)    # the first of equal maxima
    out = torch.gather(m, 2, idx).squeeze(2)
    has = pat.any(dim=2)
    out = torch.where(has, out, torch.zeros_like(out))
    if with_winner:
        return out, torch.where(has, idx.squeeze(2), torch.full_like(idx.squeeze(2), -1))
    return out


def edge_messages(x, edge_index, nn):
    src, dst = edge_index[0], edge_index[1]
    return nn(torch.cat([x[dst], x[src] - x[dst]], -1))                               # [E,C]


def edge_messages_decomposed(x, edge_index, nn):
    P, Q = decomposed_pre(x, nn)
    return _act2(nn, P[edge_index[1]] + Q[edge_index[0]])


def edgeconv(x, edge_index, nn, with_winner=False, decomposed=False):
    """x [M,F], edge_index [2,E] = (source, sink), used as given.  The winner is a position in edge_index."""
    M = x.shape[0]
    E = edge_index.shape[1]
    dst = edge_index[1]
    m = edge_messages_decomposed(x, edge_index, nn) if decomposed else edge_messages(x, edge_index, nn)
    C = m.shape[1]
    d2 = dst.unsqueeze(-1).expand(E, C)
    top = torch.full((M, C), float("-inf"), dtype=m.dtype).scatter_reduce(0, d2, m.detach(), reduce="amax")
    pos = torch.arange(E).unsqueeze(-1).expand(E, C)
    cand = torch.where(m.detach() == top[dst], pos, torch.full_like(pos, E))
    win = torch.full((M, C), E, dtype=torch.long).scatter_reduce(0, d2, cand, reduce="amin")
    has = win < E
    out = torch.gather(torch.cat([m, m.new_zeros(1, C)]), 0, win)
    out = torch.where(has, out, torch.zeros_like(out))
    if with_winner:
        return out, torch.where(has, win, torch.full_like(win, -1))
    return out


class DenseEdgeConvRef(torch.nn.Module):
    """Parameter layout of gcm.nn.DenseEdgeConv: nn.0.*, nn.2.*.  decomposed: the messages through P_i + Q_j."""

    def __init__(self, nn, decomposed=False):
        super().__init__()
        self.nn, self.decomposed = nn, decomposed

    def forward(self, x, adj, mask=None):
        x = x.unsqueeze(0) if x.dim() == 2 else x
        adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
        B, N, _ = x.shape
        out = dense_edgeconv(x, adj, self.nn, decomposed=self.decomposed)
        return out if mask is None else out * mask.view(B, N, 1).to(out.dtype)


class EdgeConvRef(torch.nn.Module):
    def __init__(self, nn, decomposed=False):
        super().__init__()
        self.nn, self.decomposed = nn, decomposed

    def forward(self, x, edge_index):
        return edgeconv(x, edge_index, self.nn, decomposed=self.decomposed)


# ---- margins (float64) ----
def decomposed_pre(x, nn):
    """(P, Q) with W1 [x_i, x_j - x_i] + b1 = P_i + Q_j: P = x (A - Bm)^T + b1, Q = x Bm^T, W1 = [A | Bm]."""
    F = x.shape[-1]
    w1, b1 = nn[0].weight, nn[0].bias
    A, Bm = w1[:, :F], w1[:, F:]
    return torch.nn.functional.linear(x, A - Bm, b1), torch.nn.functional.linear(x, Bm)


def dense_margins(x, adj, nn):
    """(smallest gap between the best and the second-best message of a (sink, channel) with two entries or more,
    smallest |pre-activation| over the set entries), both in float64; inf where there is nothing to compare."""
    x, nn = x.double(), _double(nn)
    B, N, _ = x.shape
    with torch.no_grad():
        pat = (adj != 0).expand(B, N, N)
        m = dense_messages(x, nn).masked_fill(~pat.unsqueeze(-1), float("-inf"))
        gap = torch.tensor(float("inf"), dtype=torch.float64)
        if N > 1:
            top = m.topk(2, dim=2).values
            two = (pat.sum(2) >= 2).unsqueeze(-1).expand_as(top[:, :, 0])
            if two.any():
                gap = (top[:, :, 0] - top[:, :, 1])[two].min()
        P, Q = decomposed_pre(x, nn)
        pre = (P.unsqueeze(2) + Q.unsqueeze(1))[pat]
        kink = pre.abs().min() if pre.numel() else torch.tensor(float("inf"), dtype=torch.float64)
    return float(gap), float(kink)


def csr_margins(x, edge_index, nn):
    """The same over an edge list.  Edges that repeat a (source, sink) pair carry the same message in every precision
    - an exact tie, settled by the first-entry rule - and count once here."""
    x, nn = x.double(), _double(nn)
    with torch.no_grad():
        ei = torch.unique(edge_index, dim=1)
        m = edge_messages(x, ei, nn)
        gap = float("inf")
        for i in torch.unique(ei[1]).tolist():
            mi = m[ei[1] == i]
            if mi.shape[0] >= 2:
                top = mi.topk(2, dim=0).values
                gap = min(gap, float((top[0] - top[1]).min()))
        P, Q = decomposed_pre(x, nn)
        pre = P[ei[1]] + Q[ei[0]]
        kink = float(pre.abs().min()) if pre.numel() else float("inf")
    return gap, kink


def _double(nn):
    import copy
    return copy.deepcopy(nn).double()
