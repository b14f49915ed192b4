"""Eager restatement of GENConv with softmax aggregation (DeeperGCN; PyG's GENConv) - the contract gcm.nn's GENConv
and DenseGENConv implement - in plain torch and dtype generic, so the tests can evaluate it in float64 to bound the
kernels' fp32 error.  The dense and the sparse form are written independently of each other and of gcm."""
import torch


def _t(t, like):
    return t if torch.is_tensor(t) else torch.tensor(float(t), dtype=like.dtype)


def dense_softmax_agg(xs, adj, t, eps=1e-7):
    """xs [B,N,C], adj [B,N,N] (adj[b,i,j] != 0: i aggregates from j; the values do not matter).  Per channel the
    softmax over the set entries of row i of t * m, m = relu(xs) + eps; an empty row aggregates 0."""
    B, N, C = xs.shape
    m = torch.relu(xs) + eps                                            # [B,N,C]
    pat = (adj != 0).expand(B, N, N).unsqueeze(-1)                      # [B,i,j,1]
    logit = (_t(t, xs) * m).unsqueeze(1).expand(B, N, N, C)             # [B,i,j,C]: depends on (j, c) alone
    logit = logit.masked_fill(~pat, float("-inf"))
    top = logit.max(dim=2, keepdim=True).values
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top).detach()   # an empty row: nothing to shift by
    p = torch.exp(logit - top) * pat
    s = p.sum(2)
    w = (p * m.unsqueeze(1)).sum(2)
    return torch.where(s > 0, w / s.clamp(min=1e-30), torch.zeros_like(w))


def softmax_agg(xs, edge_index, t, eps=1e-7):
    """xs [M,C], edge_index [2,E] = (source, sink), used as given: no loop added or removed, duplicates count once
    each.  A node without in-edges aggregates 0."""
    M, C = xs.shape
    src, dst = edge_index[0], edge_index[1]
    m = torch.relu(xs) + eps
    mj = m[src]                                                         # [E,C]
    logit = _t(t, xs) * mj
    top = torch.full((M, C), float("-inf"), dtype=xs.dtype).scatter_reduce(
        0, dst.unsqueeze(-1).expand(-1, C), logit.detach(), reduce="amax", include_self=True)
    p = torch.exp(logit - top[dst])
    s = torch.zeros(M, C, dtype=xs.dtype).index_add(0, dst, p)
    w = torch.zeros(M, C, dtype=xs.dtype).index_add(0, dst, p * mj)
    return torch.where(s > 0, w / s.clamp(min=1e-30), torch.zeros_like(w))


def message_norm(x, agg, scale):
    return agg / agg.norm(p=2, dim=-1, keepdim=True).clamp(min=1e-12) * x.norm(p=2, dim=-1, keepdim=True) * scale


class _GENRefBase(torch.nn.Module):
    """Parameter layout of gcm.nn.GENConv / DenseGENConv: lin_src.*, lin_dst.* (widths differ), aggr_module.t [1],
    msg_norm.scale [1], mlp.*."""

    def __init__(self, in_channels, out_channels, t=1.0, learn_t=False, msg_norm=False, learn_msg_scale=False,
                 norm="batch", num_layers=2, expansion=2, eps=1e-7, bias=False):
        super().__init__()
        self.in_channels, self.out_channels, self.eps, self.initial_t = in_channels, out_channels, eps, float(t)
        if in_channels != out_channels:
            self.lin_src = torch.nn.Linear(in_channels, out_channels, bias=bias)
            self.lin_dst = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.aggr_module = torch.nn.Module()
        if learn_t:
            self.aggr_module.t = torch.nn.Parameter(torch.full((1,), float(t)))
        else:
            self.aggr_module.register_buffer("t", torch.full((1,), float(t)))
        if msg_norm:
            self.msg_norm = torch.nn.Module()
            self.msg_norm.scale = torch.nn.Parameter(torch.ones(1), requires_grad=learn_msg_scale)
        widths = [out_channels] + [out_channels * expansion] * (num_layers - 1) + [out_channels]
        layers = []
        for i in range(1, len(widths)):
            layers.append(torch.nn.Linear(widths[i - 1], widths[i], bias=bias))
            if i < len(widths) - 1:
                if norm == "batch":
                    layers.append(torch.nn.BatchNorm1d(widths[i]))
                elif norm == "layer":
                    layers.append(torch.nn.LayerNorm(widths[i]))
                else:
                    assert norm is None
                layers += [torch.nn.ReLU(), torch.nn.Dropout(0.0)]
        self.mlp = torch.nn.Sequential(*layers)

    def _source(self, x):
        return self.lin_src(x) if self.in_channels != self.out_channels else x

    def _tail(self, x, agg):
        if hasattr(self, "msg_norm"):
            agg = message_norm(x, agg, self.msg_norm.scale)
        out = agg + (self.lin_dst(x) if self.in_channels != self.out_channels else x)
        return self.mlp(out.reshape(-1, self.out_channels)).view(*out.shape[:-1], self.out_channels)


class DenseGENRef(_GENRefBase):
    def forward(self, x, adj, mask=None):
        x = x.unsqueeze(0) if x.dim() == 2 else x
        adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
        B, N, _ = x.shape
        out = self._tail(x, dense_softmax_agg(self._source(x), adj, self.aggr_module.t, self.eps))
        return out if mask is None else out * mask.view(B, N, 1).to(out.dtype)


class GENRef(_GENRefBase):
    def forward(self, x, edge_index):
        return self._tail(x, softmax_agg(self._source(x), edge_index, self.aggr_module.t, self.eps))
