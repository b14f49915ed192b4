"""Eager restatement of PyG's ResGatedGraphConv (without edge features) and of its dense form (the contract
gcm.nn's layers implement), dtype generic so the tests can evaluate it in float64 to bound the kernels' fp32 error.
    out_i = W_skip x_i + sum_{j -> i} sigmoid(W_key x_i + b_key + W_query x_j + b_query) * (W_value x_j + b_value) + bias
The gate is per edge and per channel and is not normalised over the neighbourhood."""
import torch
import torch.nn.functional as F


def dense_resgated(x, adj, w_key, b_key, w_query, b_query, w_value, b_value, w_skip=None, bias=None, mask=None,
                   add_loop=False):
    """adj[b, i, j]: the weight of the edge j -> i (0: no edge); add_loop overwrites the diagonal with 1.
    Materialises the gates [B, N, N, C]."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    B, N, _ = x.shape
    A = adj.expand(B, N, N)
    if add_loop:
        eye = torch.eye(N, dtype=torch.bool)
        A = torch.where(eye, torch.ones_like(A), A)
    k, q, v = F.linear(x, w_key, b_key), F.linear(x, w_query, b_query), F.linear(x, w_value, b_value)
    gate = torch.sigmoid(k.unsqueeze(2) + q.unsqueeze(1))                       # [B, i, j, C]
    out = (A.unsqueeze(-1) * gate * v.unsqueeze(1)).sum(2)
    if w_skip is not None:
        out = out + F.linear(x, w_skip)
    if bias is not None:
        out = out + bias
    if mask is not None:
        out = out * mask.view(B, N, 1).to(out.dtype)
    return out


def dense_resgated_adj_grad(x, g_out, w_key, b_key, w_query, b_query, w_value, b_value, add_loop=False):
    """The stated gradient of the adjacency: g_adj[b,i,j] = sum_c g_out[b,i,c] sigmoid(k[b,i] + q[b,j])_c v[b,j,c],
    the diagonal zeroed when add_loop."""
    k, q, v = F.linear(x, w_key, b_key), F.linear(x, w_query, b_query), F.linear(x, w_value, b_value)
    gate = torch.sigmoid(k.unsqueeze(2) + q.unsqueeze(1))
    g = torch.einsum("bic,bijc,bjc->bij", g_out, gate, v)
    if add_loop:
        g = g * (1 - torch.eye(x.shape[1], dtype=g.dtype))
    return g


def resgated(x, edge_index, w_key, b_key, w_query, b_query, w_value, b_value, w_skip=None, bias=None):
    """edge_index [2, E] = (source, sink), used as given: no loop is added or removed, duplicates count once each."""
    src, dst = edge_index[0], edge_index[1]
    k, q, v = F.linear(x, w_key, b_key), F.linear(x, w_query, b_query), F.linear(x, w_value, b_value)
    msg = torch.sigmoid(k[dst] + q[src]) * v[src]
    out = torch.zeros(x.shape[0], w_key.shape[0], dtype=x.dtype).index_add(0, dst, msg)
    if w_skip is not None:
        out = out + F.linear(x, w_skip)
    return out if bias is None else out + bias


class _ResGatedRefBase(torch.nn.Module):
    """Parameter layout of the gcm.nn layers: lin_key / lin_query / lin_value (with bias), lin_skip.weight, bias."""

    def __init__(self, cin, cout, root_weight=True, bias=True):
        super().__init__()
        self.root_weight = root_weight
        self.lin_key = torch.nn.Linear(cin, cout)
        self.lin_query = torch.nn.Linear(cin, cout)
        self.lin_value = torch.nn.Linear(cin, cout)
        self.lin_skip = torch.nn.Linear(cin, cout, bias=False) if root_weight else None
        self.bias = torch.nn.Parameter(torch.zeros(cout)) if bias else None

    def _operands(self):
        return (self.lin_key.weight, self.lin_key.bias, self.lin_query.weight, self.lin_query.bias,
                self.lin_value.weight, self.lin_value.bias, self.lin_skip.weight if self.root_weight else None,
                self.bias)


class DenseResGatedRef(_ResGatedRefBase):
    def forward(self, x, adj, mask=None, add_loop=False):
        return dense_resgated(x, adj, *self._operands(), mask=mask, add_loop=add_loop)


class ResGatedRef(_ResGatedRefBase):
    def forward(self, x, edge_index, edge_attr=None):
        return resgated(x, edge_index, *self._operands())
