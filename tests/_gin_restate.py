"""Eager restatement of PyG's DenseGINConv and GINConv (the contract gcm.nn's layers implement), dtype generic so
the tests can evaluate it in float64 to bound the kernels' fp32 error."""
import torch


def dense_gin(x, adj, eps, nn, mask=None, add_loop=True):
    """adj[b, i, j]: i aggregates from j.  The values of adj are weights; its diagonal is an ordinary entry (kept and
    counted), the self term (1 + eps) x comes on top of it when add_loop."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    B, N, _ = x.shape
    out = torch.matmul(adj, x)
    if add_loop:
        out = (1 + eps) * x + out
    out = nn(out)
    if mask is not None:
        out = out * mask.view(B, N, 1).to(out.dtype)
    return out


def gin(x, edge_index, eps, nn):
    """edge_index [2, E] = (source, sink), used as given: no loop added or removed, duplicates count once each."""
    src, dst = edge_index[0], edge_index[1]
    agg = torch.zeros_like(x).index_add(0, dst, x[src])
    return nn((1 + eps) * x + agg)


class _GINRefBase(torch.nn.Module):
    """Parameter layout of gcm.nn.DenseGINConv / GINConv (eps [1], nn.*)."""

    def __init__(self, nn, eps=0.0, train_eps=False):
        super().__init__()
        self.nn, self.initial_eps = nn, float(eps)
        if train_eps:
            self.eps = torch.nn.Parameter(torch.full((1,), float(eps)))
        else:
            self.register_buffer("eps", torch.full((1,), float(eps)))


class DenseGINRef(_GINRefBase):
    def forward(self, x, adj, mask=None, add_loop=True):
        return dense_gin(x, adj, self.eps, self.nn, mask, add_loop)


class GINRef(_GINRefBase):
    def forward(self, x, edge_index):
        return gin(x, edge_index, self.eps, self.nn)
