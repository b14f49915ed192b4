"""Eager restatement of PyG's TAGConv (Du et al., Topology Adaptive Graph Convolutional Networks) and of its dense
form (the contract gcm.nn's layers implement), dtype generic so the tests can evaluate it in float64 to bound the
kernels' fp32 error.  Written from the formulas:
    h_0 = x;  h_k = A^ h_{k-1};  out = sum_{k=0..K} h_k W_k^T + bias
    normalize: gcn_norm(add_self_loops=False): deg_i = the sum of the weights INTO i, d_i = deg_i^-1/2 and 0 where
    deg_i == 0, A^_ij = d_i A_ij d_j (dense), c_e = d_src w_e d_dst (sparse); otherwise A^ = A, c_e = w_e.
Autograd through these functions is the stated gradient: every entry of adj gets one, also where adj is 0, the degree
term of its row included; an overwritten diagonal gets 0; the degree term of a row with deg == 0 is exactly 0."""
import torch


def inv_sqrt_degree(deg):
    """deg^-1/2, 0 where deg == 0; the power is taken of a positive stand-in so that autograd gives 0 there, not
    NaN."""
    pos = deg > 0
    return torch.where(pos, torch.where(pos, deg, torch.ones_like(deg)) ** -0.5, torch.zeros_like(deg))


def dense_adjacency(adj, B, N, add_loop):
    """adj broadcast to [B, N, N], the diagonal overwritten with 1 when add_loop."""
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    A = adj.expand(B, N, N)
    if add_loop:
        A = torch.where(torch.eye(N, dtype=torch.bool), torch.ones_like(A), A)
    return A


def _polynomial(hop, x, weights, bias):
    h = x
    out = h @ weights[0].t()
    for w in weights[1:]:
        h = hop(h)
        out = out + h @ w.t()
    return out if bias is None else out + bias


def dense_tag(x, adj, weights, bias=None, mask=None, add_loop=False, normalize=True):
    """adj[b, i, j]: the weight of the edge j -> i; weights: the K + 1 matrices [Fo, Fi]."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    B, N, _ = x.shape
    A = dense_adjacency(adj, B, N, add_loop)
    if normalize:
        d = inv_sqrt_degree(A.sum(-1))
        A = d.unsqueeze(-1) * A * d.unsqueeze(-2)
    out = _polynomial(lambda h: A @ h, x, weights, bias)
    if mask is not None:
        out = out * mask.view(B, N, 1).to(out.dtype)
    return out


def tag(x, edge_index, weights, bias=None, edge_weight=None, normalize=True):
    """edge_index [2, E] = (source, sink), used as given: no loop is added or removed, duplicates are separate terms.
    A weight vector of the wrong length is ignored (GraphConv's rule)."""
    src, dst = edge_index[0], edge_index[1]
    M = x.shape[0]
    if edge_weight is not None and edge_weight.numel() != src.numel():
        edge_weight = None
    w = torch.ones(src.numel(), dtype=x.dtype) if edge_weight is None else edge_weight.to(x.dtype)
    if normalize:
        d = inv_sqrt_degree(torch.zeros(M, dtype=x.dtype).index_add(0, dst, w))
        coef = d[src] * w * d[dst]
    else:
        coef = w

    def hop(h):
        return torch.zeros_like(h).index_add(0, dst, coef.unsqueeze(-1) * h[src])
    return _polynomial(hop, x, weights, bias)


class _TagRefBase(torch.nn.Module):
    """Parameter layout of the gcm.nn layers and of PyG: lins.k.weight [Fo, Fi] for k = 0..K, bias [Fo]."""

    def __init__(self, in_channels, out_channels, K=3, bias=True, normalize=True):
        super().__init__()
        self.K, self.normalize = K, normalize
        self.lins = torch.nn.ModuleList(torch.nn.Linear(in_channels, out_channels, bias=False) for _ in range(K + 1))
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)

    def _weights(self):
        return [lin.weight for lin in self.lins]


class DenseTagRef(_TagRefBase):
    def forward(self, x, adj, mask=None, add_loop=False):
        return dense_tag(x, adj, self._weights(), self.bias, mask, add_loop, self.normalize)


class TagRef(_TagRefBase):
    def forward(self, x, edge_index, edge_weight=None):
        return tag(x, edge_index, self._weights(), self.bias, edge_weight, self.normalize)


def lively(conv):
    """The bias off its zero init: drawn from U(-0.5, 0.5)."""
    with torch.no_grad():
        if conv.bias is not None:
            conv.bias.uniform_(-0.5, 0.5)
    return conv
