"""Eager restatement of PyG's GATv2Conv (with edge_dim) and of its dense twin - the contract gcm.gatv2's classes
implement - dtype generic so the tests can evaluate it in float64 to bound the kernels' fp32 error; and the quantised
test inputs that make every LeakyReLU argument exact in fp32, so the side of the kink (and the convention at 0: the
derivative there is negative_slope, torch's) cannot differ between the kernels and the float64 reference."""
import torch

from _gine_restate import quant


def _loop_attr(edge_attr, dst, M, fill_value):
    """[M, D]: the loop's edge feature: the mean over the in-edges given (zero for none), or the number."""
    D = edge_attr.shape[-1]
    if fill_value == "mean":
        cnt = torch.zeros(M, dtype=edge_attr.dtype).index_add(0, dst, torch.ones(dst.numel(), dtype=edge_attr.dtype))
        return torch.zeros(M, D, dtype=edge_attr.dtype).index_add(0, dst, edge_attr) / cnt.clamp(min=1).unsqueeze(-1)
    return torch.full((M, D), float(fill_value), dtype=edge_attr.dtype)


def terms(x, edge_index, lin_l, lin_r, lin_edge=None, edge_attr=None, heads=1, add_self_loops=True,
          fill_value="mean"):
    """The terms of the softmaxes -> (src, dst, x_l [M,H,C], x_r, e [T,H,C] | None, z [T,H,C]); the loops come last."""
    M, H = x.shape[0], heads
    src, dst = edge_index[0], edge_index[1]
    ea = edge_attr if lin_edge is not None else None
    if add_self_loops:
        keep = src != dst
        src, dst = src[keep], dst[keep]
        n = torch.arange(M)
        if ea is not None:
            ea = ea[keep]
            ea = torch.cat([ea, _loop_attr(ea, dst, M, fill_value)])
        src, dst = torch.cat([src, n]), torch.cat([dst, n])
    x_l, x_r = lin_l(x).view(M, H, -1), lin_r(x).view(M, H, -1)
    z = x_l[src] + x_r[dst]
    e = None
    if ea is not None:
        e = lin_edge(ea).view(-1, H, x_l.shape[-1])
        z = z + e
    return src, dst, x_l, x_r, e, z


def gatv2(x, edge_index, lin_l, lin_r, att, lin_edge=None, bias=None, edge_attr=None, heads=1, concat=True,
          negative_slope=0.2, add_self_loops=True, fill_value="mean"):
    """edge_index [2, E] = (source, sink); edge_attr [E, D] in edge_index order (ignored without lin_edge)."""
    M, H = x.shape[0], heads
    src, dst, x_l, _, _, z = terms(x, edge_index, lin_l, lin_r, lin_edge, edge_attr, heads, add_self_loops, fill_value)
    s = (torch.nn.functional.leaky_relu(z, negative_slope) * att.view(1, H, -1)).sum(-1)         # [T, H]
    idx = dst.view(-1, 1).expand(-1, H)
    top = torch.full((M, H), float("-inf"), dtype=x.dtype).scatter_reduce(0, idx, s.detach(), "amax")
    p = torch.exp(s - top[dst])
    alpha = p / torch.zeros(M, H, dtype=x.dtype).index_add(0, dst, p)[dst]
    out = torch.zeros_like(x_l).index_add(0, dst, alpha.unsqueeze(-1) * x_l[src])
    out = out.reshape(M, -1) if concat else out.mean(1)
    return out if bias is None else out + bias


def dense_gatv2(x, adj, lin_l, lin_r, att, lin_edge=None, bias=None, edge_attr=None, mask=None, heads=1, concat=True,
                negative_slope=0.2, add_loop=True, fill_value="mean"):
    """adj[b, i, j] != 0: i attends to j (only the pattern is read); edge_attr [B, N, N, D], read at the set entries
    only.  The broadcast form: every [B, N, N, H, C] tensor is written out."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    B, N, _ = x.shape
    H = heads
    pat = (adj != 0).expand(B, N, N)
    eye = torch.eye(N, dtype=torch.bool).expand(B, N, N)
    off = pat & ~eye if add_loop else pat
    x_l, x_r = lin_l(x).view(B, N, H, -1), lin_r(x).view(B, N, H, -1)
    z = x_l.unsqueeze(1) + x_r.unsqueeze(2)                               # [b, i, j] = x_l[b, j] + x_r[b, i]
    if lin_edge is not None:
        ea = edge_attr.unsqueeze(0) if edge_attr.dim() == 3 else edge_attr
        ea = torch.where(off.unsqueeze(-1), ea.expand(B, N, N, -1), torch.zeros((), dtype=x.dtype))
        if add_loop:
            if fill_value == "mean":
                loop = ea.sum(2) / off.sum(2).clamp(min=1).unsqueeze(-1).to(x.dtype)
            else:
                loop = torch.full((B, N, ea.shape[-1]), float(fill_value), dtype=x.dtype)
            ea = ea + eye.unsqueeze(-1).to(x.dtype) * loop.unsqueeze(2)
        z = z + lin_edge(ea).view(B, N, N, H, -1)
    pat = off | eye if add_loop else off
    s = (torch.nn.functional.leaky_relu(z, negative_slope) * att.view(1, 1, 1, H, -1)).sum(-1)   # [B, N, N, H]
    s = s.masked_fill(~pat.unsqueeze(-1), float("-inf"))
    live = pat.any(2).view(B, N, 1, 1)
    alpha = torch.softmax(torch.where(live, s, torch.zeros((), dtype=x.dtype)), dim=2)
    alpha = torch.where(live, alpha, torch.zeros((), dtype=x.dtype))
    out = torch.einsum("bijh,bjhc->bihc", alpha, x_l)
    out = out.reshape(B, N, -1) if concat else out.mean(2)
    if bias is not None:
        out = out + bias
    if mask is not None:
        out = out * mask.reshape(B, N, 1).to(out.dtype)
    return out


class _GATv2RefBase(torch.nn.Module):
    """Parameter layout of gcm.gatv2.GATv2Conv / DenseGATv2Conv: lin_l, lin_r (lin_l itself with share_weights), att
    [1,H,C], lin_edge (no bias; with edge_dim), bias."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, edge_dim=None,
                 fill_value="mean", bias=True, share_weights=False, add_self_loops=True):
        super().__init__()
        self.heads, self.concat, self.negative_slope = heads, concat, negative_slope
        self.fill_value, self.add_self_loops, self.edge_dim = fill_value, add_self_loops, edge_dim
        self.lin_l = torch.nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.lin_r = self.lin_l if share_weights else torch.nn.Linear(in_channels, heads * out_channels, bias=bias)
        self.att = torch.nn.Parameter(torch.randn(1, heads, out_channels) * 0.5)
        self.lin_edge = torch.nn.Linear(edge_dim, heads * out_channels, bias=False) if edge_dim is not None else None
        self.bias = torch.nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels)) if bias else None


class GATv2Ref(_GATv2RefBase):
    def forward(self, x, edge_index, edge_attr=None):
        return gatv2(x, edge_index, self.lin_l, self.lin_r, self.att, self.lin_edge, self.bias, edge_attr, self.heads,
                     self.concat, self.negative_slope, self.add_self_loops, self.fill_value)


class DenseGATv2Ref(_GATv2RefBase):
    def forward(self, x, adj, edge_attr=None, mask=None, add_loop=True):
        return dense_gatv2(x, adj, self.lin_l, self.lin_r, self.att, self.lin_edge, self.bias, edge_attr, mask,
                           self.heads, self.concat, self.negative_slope, add_loop, self.fill_value)


# ---------------------------------------------------------------------------
# quantised inputs: x and edge_attr in eighths, every Linear weight and bias in quarters (pose-offset columns of
# lin_edge in halves: those features are differences of eighths scaled by a power of two).  Then x_l, x_r, lin_edge(a)
# and z are small multiples of 2^-6, exact in fp32 in every summation order.  Where a "mean" loop averages edge
# features, the in-degrees are 0, 1, 2 or 4 and the features multiples of 1/2, so the mean is in eighths again.
# att and the output bias are not quantised: they sit behind the kink.
# ---------------------------------------------------------------------------
def quant_layer(conv, gen, half_cols=()):
    """conv's Linear parameters overwritten in place with quantised ones."""
    with torch.no_grad():
        for lin in [conv.lin_l] + ([] if conv.lin_r is conv.lin_l else [conv.lin_r]):
            lin.weight.copy_(quant(tuple(lin.weight.shape), 4, 4, gen))
            if lin.bias is not None:
                lin.bias.copy_(quant(tuple(lin.bias.shape), 4, 4, gen))
        if conv.lin_edge is not None:
            w = quant(tuple(conv.lin_edge.weight.shape), 4, 4, gen)
            for c in half_cols:
                w[:, c] = quant((w.shape[0],), 2, 2, gen)
            conv.lin_edge.weight.copy_(w)
        conv.att.copy_(torch.randn(conv.att.shape, generator=gen) * 0.5)
        if conv.bias is not None:
            conv.bias.copy_(torch.randn(conv.bias.shape, generator=gen) * 0.5)


def _pow2_degrees(n, E, gen):
    """n in-degrees from {0, 1, 2, 4} that sum to E."""
    assert 4 * n >= E
    deg, left = [0] * n, E
    while left:
        for i in torch.randperm(n, generator=gen).tolist():
            cost = {0: 1, 1: 1, 2: 2}.get(deg[i])
            if cost is not None and cost <= left:
                deg[i] += cost
                left -= cost
            if not left:
                break
    return deg


# (M, E, Fi, H, C, D, options).  fill_value: the layer's (default "mean"); mixed: duplicates and self edges
SPARSE_CASES = [(1, 0, 3, 1, 2, None, {}), (7, 15, 3, 2, 5, None, {"mixed": True}), (40, 90, 8, 3, 7, 5, {}),
                (33, 200, 32, 4, 8, 3, {"fill_value": 0.5, "mixed": True}), (20, 60, 65, 1, 128, 32, {}),
                (20, 60, 128, 4, 32, None, {"concat": False, "mixed": True})]


def case_id(case):
    return "-".join(str(c) for c in case[:6])


def sparse_case(M, E, Fi, H, C, D, opts, seed=0):
    """-> (x [M,Fi], edge_index [2,E] in no particular order, edge_attr [E,D] | None) in float64; the last nodes stay
    isolated.  mixed: duplicates and self edges; otherwise in-degrees from {0, 1, 2, 4} and no self edge."""
    gen = torch.Generator().manual_seed(3000 + seed + 7 * M + E + Fi)
    x = quant((M, Fi), 8, 16, gen)
    hi = max(M - 3, 1)
    if opts.get("mixed"):
        ei = torch.randint(0, hi, (2, E), generator=gen)
        if E >= 8:
            ei[:, 1] = ei[:, 0]                                   # a duplicate
            ei[1, 2] = ei[0, 2]                                   # a self edge
            ei[:, 3] = ei[:, 2]                                   # twice
    else:
        dst = torch.tensor([i for i, d in enumerate(_pow2_degrees(hi, E, gen)) for _ in range(d)], dtype=torch.long)
        src = (dst + 1 + torch.randint(0, max(hi - 1, 1), (E,), generator=gen)) % hi if E else dst.clone()
        ei = torch.stack([src, dst])[:, torch.randperm(E, generator=gen)]
    ea = None
    if D is not None:
        ea = quant((E, D), 8, 8, gen) if opts.get("mixed") else quant((E, D), 2, 2, gen)
    return x, ei, ea


# (B, N, Fi, H, C, D, options)
DENSE_CASES = [(3, 7, 3, 1, 5, None, {}), (5, 1, 4, 2, 3, 1, {}), (3, 33, 8, 2, 8, 3, {"mask": True}),
               (2, 40, 16, 4, 12, 4, {"add_loop": False, "concat": False}), (2, 130, 64, 4, 32, 4, {}),
               (2, 20, 128, 1, 128, 32, {})]


def dense_case(B, N, Fi, H, C, D, opts, seed=0):
    """-> (x, adj, edge_attr | None, mask | None) in float64.  With add_loop the rows have 0, 1, 2 or 4 set off-diagonal
    entries (and some set diagonal ones, which the loop replaces); with add_loop=False a random pattern with empty rows
    and diagonal entries.  broadcast: one adjacency / edge_attr for the batch; two_d: [N,Fi], [N,N], [N,N,D]."""
    gen = torch.Generator().manual_seed(4000 + seed + 7 * B + N + Fi)
    Ba = 1 if opts.get("broadcast") or opts.get("two_d") else B
    x = quant((B, N, Fi), 8, 16, gen)
    if opts.get("add_loop", True):
        adj = torch.zeros(Ba, N, N, dtype=torch.float64)
        for b in range(Ba):
            for i in range(N):
                d = [0, 1, 2, 4][int(torch.randint(0, 4, (1,), generator=gen))]
                others = [j for j in range(N) if j != i]
                if d > len(others):
                    d = {0: 0, 1: 1, 2: 2, 3: 2}.get(len(others), 4)
                for t in torch.randperm(len(others), generator=gen)[:d].tolist():
                    adj[b, i, others[t]] = 1
        if N > 1:
            adj[:, 1, 1] = 1                                      # a set diagonal entry
        ea = quant((Ba, N, N, D), 2, 2, gen) if D is not None else None
    else:
        adj = (torch.rand(Ba, N, N, generator=gen) < 0.3).double()
        adj[:, 2] = 0                                             # an empty row
        adj[:, 1, 1] = 1
        ea = quant((Ba, N, N, D), 8, 8, gen) if D is not None else None
    mask = (torch.rand(B, N, generator=gen) < 0.7) if opts.get("mask") else None
    if opts.get("two_d"):
        x, adj, ea = x[0], adj[0], None if ea is None else ea[0]
    return x, adj, ea, mask


def layer_kwargs(case):
    """The constructor arguments of the case's layer (both the gcm.gatv2 classes and the Ref ones take them)."""
    _, _, Fi, H, C, D, opts = case
    kw = dict(in_channels=Fi, out_channels=C, heads=H, concat=opts.get("concat", True), edge_dim=D)
    for k in ("fill_value", "bias", "share_weights", "negative_slope"):
        if k in opts:
            kw[k] = opts[k]
    return kw


def exactness(values):
    """(every entry an integer multiple of 2^-6, the largest magnitude) over the given tensors."""
    ok, top = True, 0.0
    for v in values:
        if v is None or v.numel() == 0:
            continue
        v = v.detach().double()
        ok = ok and bool(((v * 64) == (v * 64).round()).all())
        top = max(top, float(v.abs().max()))
    return ok, top
