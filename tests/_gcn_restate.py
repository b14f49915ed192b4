"""Eager restatement of PyG's DenseGCNConv and GCNConv (the contract gcm.nn's layers implement),
dtype generic so the tests can evaluate it in float64 to bound the kernels' fp32 error."""
import torch


def dense_gcn(x, adj, weight, bias=None, mask=None, add_loop=True, improved=False):
    """adj[b, i, j]: edge j -> i.  The diagonal is overwritten (not added) when add_loop."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    B, N, _ = x.shape
    A = adj.expand(B, N, N).clone()
    if add_loop:
        idx = torch.arange(N)
        A[:, idx, idx] = 2.0 if improved else 1.0
    d = A.sum(-1).clamp(min=1) ** -0.5
    out = d.unsqueeze(-1) * (A @ (d.unsqueeze(-1) * (x @ weight.t())))
    if bias is not None:
        out = out + bias
    if mask is not None:
        out = out * mask.view(B, N, 1).to(out.dtype)
    return out


def gcn(x, edge_index, weight, bias=None, edge_weight=None, improved=False, add_self_loops=True,
        normalize=True):
    """edge_index [2, E] = (source, sink); gcn_norm with add_remaining_self_loops (the last existing
    i -> i edge of a node gives its loop weight, every i -> i edge is removed)."""
    M, E = x.shape[0], edge_index.shape[1]
    src, dst = edge_index[0], edge_index[1]
    w = torch.ones(E, dtype=x.dtype) if edge_weight is None else edge_weight
    if normalize:
        if add_self_loops:
            fill = torch.full((M,), 2.0 if improved else 1.0, dtype=x.dtype)
            is_loop = src == dst
            pos = torch.arange(E)
            last = torch.full((M,), -1, dtype=torch.long).scatter_reduce(
                0, src[is_loop], pos[is_loop], reduce="amax")
            lw = torch.where(last >= 0, w[last.clamp(min=0)], fill) if E else fill
            keep = ~is_loop
            loops = torch.arange(M)
            src, dst = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
            w = torch.cat([w[keep], lw])
        deg = torch.zeros(M, dtype=x.dtype).index_add(0, dst, w)
        dinv = deg ** -0.5
        dinv = dinv.masked_fill(dinv == float("inf"), 0.0)
        coef = dinv[src] * w * dinv[dst]
    else:
        coef = w
    y = x @ weight.t()
    out = torch.zeros(M, weight.shape[0], dtype=x.dtype).index_add(0, dst, coef.unsqueeze(-1) * y[src])
    return out if bias is None else out + bias


class DenseGCNRef(torch.nn.Module):
    """Parameter layout of gcm.nn.DenseGCNConv (lin.weight, bias)."""

    def __init__(self, cin, cout, improved=False, bias=True):
        super().__init__()
        self.improved = improved
        self.lin = torch.nn.Linear(cin, cout, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(cout)) if bias else None

    def forward(self, x, adj, mask=None, add_loop=True):
        return dense_gcn(x, adj, self.lin.weight, self.bias, mask, add_loop, self.improved)


class GCNRef(torch.nn.Module):
    """Parameter layout of gcm.nn.GCNConv (lin.weight, bias)."""

    def __init__(self, cin, cout, improved=False, add_self_loops=True, normalize=True, bias=True):
        super().__init__()
        self.improved, self.add_self_loops, self.normalize = improved, add_self_loops, normalize
        self.lin = torch.nn.Linear(cin, cout, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(cout)) if bias else None

    def forward(self, x, edge_index, edge_weight=None):
        return gcn(x, edge_index, self.lin.weight, self.bias, edge_weight, self.improved, self.add_self_loops,
                   self.normalize)


def bound(f64, f32_ref, floor=2e-6, relative=False):
    """atol: 3x the restatement's own fp32 distance from its float64 evaluation, with tests/_golden.py's
    floors: 2e-6 absolute for outputs, 5e-7 of the gradient's scale for gradients (relative=True)."""
    f64 = f64.detach().double()
    if f64.numel() == 0:
        return floor
    scale = float(f64.abs().max()) if relative else 1.0
    own = float((f32_ref.detach().double() - f64).abs().max())
    return max(3.0 * own, floor * scale)


def assert_bounded(got, f64, f32_ref, what="", floor=2e-6, relative=False):
    atol = bound(f64, f32_ref, floor, relative)
    if f64.numel() == 0:
        return
    err = float((got.detach().cpu().double() - f64.detach().double()).abs().max())
    assert err <= atol, f"{what}: max error {err:.3e} > bound {atol:.3e}"
