"""DenseGINConv / GINConv kernels against the eager restatement (tests/_gin_restate.py), evaluated in float64 for the
bound and in float32 for the restatement's own error (tests/_gcn_restate.py's rule).  Needs an MI355X."""
import copy

import pytest
import torch

from _gcn_restate import assert_bounded
from _gin_restate import DenseGINRef, GINRef, dense_gin, gin
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _nn(kind, cin, cout):
    """identity: the aggregation alone; mlp: the whole layer (Tanh: no kink for an fp32 sign flip to sit on)."""
    if kind == "identity":
        return torch.nn.Identity()
    if kind == "skinny":                                      # the same MLP on gcm.nn.SkinnyLinear (HIP, many rows)
        from gcm import nn as G
        return torch.nn.Sequential(G.SkinnyLinear(cin, 2 * cout), torch.nn.Tanh(), G.SkinnyLinear(2 * cout, cout))
    return torch.nn.Sequential(torch.nn.Linear(cin, 2 * cout), torch.nn.Tanh(), torch.nn.Linear(2 * cout, cout))


def _ref_eval(fn, nn, inputs, g, dtype):
    """fn(nn, *inputs) in dtype -> (out, {name: gradient}) over the floating inputs and nn's parameters."""
    nn_ = copy.deepcopy(nn).to(dtype)
    ts = {k: None if t is None else t.detach().to(dtype).requires_grad_() for k, t in inputs.items()}
    out = fn(nn_, **ts)
    out.backward(g.to(dtype))
    grads = {k: None if t is None else t.grad for k, t in ts.items()}
    grads.update({"nn." + k: p.grad for k, p in nn_.named_parameters()})
    return out, grads


def _check(got, grads_got, fn, nn, inputs, g):
    o64, g64 = _ref_eval(fn, nn, inputs, g, torch.float64)
    o32, g32 = _ref_eval(fn, nn, inputs, g, torch.float32)
    assert got.shape == o64.shape
    assert_bounded(got, o64, o32, "out")
    for name, b64 in g64.items():
        if b64 is None:
            continue
        assert grads_got[name] is not None, name
        assert_bounded(grads_got[name], b64, g32[name], name, floor=GRAD_FLOOR, relative=True)


# ---------------------------------------------------------------------------
# DenseGINConv
# ---------------------------------------------------------------------------
_DENSE = [
    (3, 7, 3, {"eps": 0.3}),                                  # sub-tile
    (5, 1, 4, {}),                                            # a single node
    (3, 33, 8, {"mask": True}),                               # one past a tile
    (2, 40, 16, {"add_loop": False}),                         # no self term
    (2, 40, 16, {"eps": -1.0}),                               # the self term vanishes
    (4, 300, 64, {"weighted": True, "diag": True}),           # several row blocks
    (2, 20, 128, {}),                                         # the widest F
    (1, 20, 6, {"two_d": True}),
    (4, 20, 6, {"bcast": True}),
]


def _run_dense(B, N, F, opts, kind):
    from gcm import nn as G
    torch.manual_seed(B * 1000 + N + F)
    add_loop, eps = opts.get("add_loop", True), opts.get("eps", 0.0)
    Fo = F if kind == "identity" else max(3, F // 2)
    conv = G.DenseGINConv(_nn(kind, F, Fo), eps=eps, train_eps=True)
    x = torch.randn(B, N, F)
    nb = 1 if opts.get("bcast") else B
    adj = (torch.rand(nb, N, N) < 0.3).float()
    if opts.get("weighted"):
        adj = adj * torch.rand(nb, N, N) * 2
    eye = torch.eye(N).expand(nb, N, N)
    adj = adj * (1 - eye) + (eye * torch.rand(nb, N, 1) * 3 if opts.get("diag") else 0)
    mask = (torch.rand(B, N) < 0.7) if opts.get("mask") else None
    if opts.get("two_d"):
        x, adj = x[0], adj[0]
    g = torch.randn(B, N, Fo)

    dconv = copy.deepcopy(conv).to(DEV)
    xd, ad = x.to(DEV).requires_grad_(), adj.to(DEV).requires_grad_()
    out = dconv(xd, ad, None if mask is None else mask.to(DEV), add_loop=add_loop)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    got = {"x": xd.grad, "adj": ad.grad, "eps": dconv.eps.grad}
    got.update({"nn." + k: p.grad for k, p in dconv.nn.named_parameters()})
    if not add_loop:                                          # eps is not used: its gradient is exactly zero
        assert got["eps"] is None or float(got["eps"].abs().max()) == 0.0

    def fn(nn_, x, adj, eps):
        return dense_gin(x, adj, eps, nn_, mask, add_loop)

    _check(out, got, fn, conv.nn, {"x": x, "adj": adj, "eps": conv.eps}, g)


@pytest.mark.parametrize("kind", ["identity", "mlp"])
@pytest.mark.parametrize("B,N,F,opts", _DENSE)
def test_dense_ginconv(B, N, F, opts, kind):
    _run_dense(B, N, F, opts, kind)


def test_dense_ginconv_cfg2_size():
    """cfg2's shape, the whole layer with no library GEMM: `nn` is built from gcm.nn.SkinnyLinear, whose weight
    gradient sums the 32768 rows as row-split slabs.  (A torch.nn.Linear here would hand its weight gradient to the
    library GEMM, one fp32 chain over all 32768 rows: about 9e-6 of the gradient's scale away from float64, beyond 3x
    the restatement's own distance - an error of that GEMM, not of the aggregation under test.)"""
    _run_dense(256, 128, 32, {"eps": 0.1}, "skinny")


def test_dense_ginconv_rejects_wide_layers():
    from gcm import nn as G
    conv = G.DenseGINConv(torch.nn.Identity()).to(DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        conv(torch.randn(2, 5, 130, device=DEV), torch.ones(2, 5, 5, device=DEV))


# ---------------------------------------------------------------------------
# GINConv
# ---------------------------------------------------------------------------
def _edges(M, E, seed, loops=True):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, M - 3), (2, E), generator=gen)     # the last 3 nodes stay isolated
    if E and loops:
        extra = torch.tensor([[0, 1, 0, 2, 1], [0, 2, 0, 2, 2]])     # duplicate loops (0, 0), duplicate edge 1 -> 2
        ei = torch.cat([ei[:, : E // 2], extra, ei[:, E // 2:]], 1)
    return ei


def _with_index(ei, M, mask=None):
    """The edge list in CSR order on the device with a ready index attached, as SparseGCM hands it over."""
    from gcm import _ops
    dst, perm = torch.sort(ei[1], stable=True)
    es = ei[:, perm].contiguous().to(DEV)
    es.gcm_graph = _ops.GraphIndex(es, _ops.ptr_from_sorted(es[1].contiguous(), M), M, mask=mask)
    return es


def _run_sparse(M, E, F, opts, kind, indexed):
    from gcm import nn as G
    torch.manual_seed(M + E + F)
    Fo = F if kind == "identity" else max(3, F // 2)
    conv = G.GINConv(_nn(kind, F, Fo), eps=opts.get("eps", 0.0), train_eps=True)
    ei = _edges(M, E, seed=M + E)
    x = torch.randn(M, F)
    g = torch.randn(M, Fo)

    dconv = copy.deepcopy(conv).to(DEV)
    xd = x.to(DEV).requires_grad_()
    out = dconv(xd, _with_index(ei, M) if indexed else ei.to(DEV))
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    got = {"x": xd.grad, "eps": dconv.eps.grad}
    got.update({"nn." + k: p.grad for k, p in dconv.nn.named_parameters()})

    def fn(nn_, x, eps):
        return gin(x, ei, eps, nn_)

    _check(out, got, fn, conv.nn, {"x": x, "eps": conv.eps}, g)


@pytest.mark.parametrize("kind", ["identity", "mlp"])
@pytest.mark.parametrize("M,E,F,opts", [
    (6, 0, 3, {}),                                            # no edges
    (40, 90, 8, {"eps": 0.2}),                                # the eps gradient
    (300, 1500, 33, {}),                                      # odd F
    (129, 700, 128, {"eps": -0.4}),                           # the widest F
])
def test_ginconv(M, E, F, opts, kind):
    _run_sparse(M, E, F, opts, kind, indexed=True)


@pytest.mark.parametrize("M,E,F", [(6, 0, 3), (40, 90, 8)])
def test_ginconv_builds_its_own_index(M, E, F):
    _run_sparse(M, E, F, {"eps": 0.2}, "mlp", indexed=False)


def test_ginconv_rejects_a_masked_index():
    from gcm import nn as G
    M = 10
    es = _with_index(_edges(M, 20, seed=3), M, mask=torch.ones(M, dtype=torch.bool, device=DEV))
    conv = G.GINConv(torch.nn.Identity()).to(DEV)
    with pytest.raises(ValueError, match="masked GraphIndex"):
        conv(torch.randn(M, 4, device=DEV), es)


def test_ginconv_rejects_wide_layers():
    from gcm import nn as G
    conv = G.GINConv(torch.nn.Identity()).to(DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        conv(torch.randn(5, 130, device=DEV), torch.tensor([[0, 1], [1, 2]], device=DEV))


def test_dense_equals_sparse():
    """The same graph through both layers with shared weights, each against the same float64 restatement."""
    from gcm import nn as G
    torch.manual_seed(7)
    B, N, F, Fo = 3, 20, 8, 12
    adj = (torch.rand(B, N, N) < 0.25).float()                # 0/1, loops on the diagonal here and there
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])              # adj[b, i, j]: edge j -> i
    conv = G.DenseGINConv(_nn("mlp", F, Fo), eps=0.3, train_eps=True)
    dconv = copy.deepcopy(conv).to(DEV)
    sconv = G.GINConv(_nn("mlp", F, Fo), train_eps=True).to(DEV)
    sconv.load_state_dict(dconv.state_dict())
    x, g = torch.randn(B, N, F), torch.randn(B, N, Fo)
    xa, xb = x.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
    out_d = dconv(xa, adj.to(DEV))
    out_s = sconv(xb.view(B * N, F), ei.to(DEV)).view(B, N, Fo)
    out_d.backward(g.to(DEV))
    out_s.backward(g.to(DEV))
    torch.cuda.synchronize()

    def fn(nn_, x, eps):
        return dense_gin(x, adj.to(x.dtype), eps, nn_)

    for out, xg, c in ((out_d, xa.grad, dconv), (out_s, xb.grad, sconv)):
        got = {"x": xg, "eps": c.eps.grad}
        got.update({"nn." + k: p.grad for k, p in c.nn.named_parameters()})
        _check(out, got, fn, conv.nn, {"x": x, "eps": conv.eps}, g)


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
def _layers(cls, F, H):
    torch.manual_seed(5)
    return (cls(_nn("mlp", F, H), eps=0.1, train_eps=True), cls(_nn("mlp", H, H), eps=-0.2, train_eps=True))


def _dense_pair(F, H):
    from gcm import nn as G
    r1, r2 = _layers(DenseGINRef, F, H)
    ref = pyg.Sequential("x, adj, weights, B, N", [(r1, "x, adj -> x"), torch.nn.Tanh(),
                                                   (r2, "x, adj -> x"), torch.nn.Tanh()])
    d1, d2 = _layers(G.DenseGINConv, F, H)
    dev = G.Sequential("x, adj, weights, B, N", [(d1, "x, adj -> x"), torch.nn.Tanh(),
                                                 (d2, "x, adj -> x"), torch.nn.Tanh()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _sparse_pair(F, H):
    from gcm import nn as G
    r1, r2 = _layers(GINRef, F, H)
    ref = pyg.Sequential("x, edges, weights", [(r1, "x, edges -> x"), torch.nn.Tanh(), (r2, "x, edges -> x")])
    d1, d2 = _layers(G.GINConv, F, H)
    dev = G.Sequential("x, edges, weights", [(d1, "x, edges -> x"), torch.nn.Tanh(), (d2, "x, edges -> x")])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def test_dense_gcm_with_gin_stack():
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    torch.manual_seed(11)
    B, F, H, N, T = 4, 6, 16, 8, 12               # T > N: the overflow wrap
    ref, dev = _dense_pair(F, H)
    assert any(k.endswith(".eps") for k, _ in dev.named_parameters())
    obs = torch.randn(T, B, F)
    gw = torch.randn(T, B, H)

    res = {}
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(ref).to(dt)
        want, h = od.dense_rollout(obs.to(dt), None, r, graph_size=N, edge_selectors=od.TemporalBackedge([1, 2]))
        (want * gw.to(dt)).sum().backward()
        res[dt] = (want, h, {k: p.grad for k, p in r.named_parameters()})

    def compare(got, hidden):
        assert_bounded(got, res[torch.float64][0], res[torch.float32][0], "mx")
        assert_bounded(hidden[0], res[torch.float64][1][0], res[torch.float32][1][0], "nodes")
        assert torch.equal(hidden[1].cpu(), res[torch.float32][1][1])
        for k, p in dev.named_parameters():
            assert_bounded(p.grad, res[torch.float64][2][k], res[torch.float32][2][k], k, floor=GRAD_FLOOR,
                           relative=True)

    mem = DenseGCM(dev, edge_selectors=TemporalBackedge([1, 2]), graph_size=N)
    assert mem._structure() is None
    hidden, outs = None, []
    for t in range(T):
        mx, hidden = mem(obs[t].to(DEV), hidden)
        outs.append(mx)
    got = torch.stack(outs)
    (got * gw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    compare(got, hidden)

    dev.zero_grad(set_to_none=True)
    got, hidden = mem.rollout(obs.to(DEV))
    (got * gw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    compare(got, hidden)


@pytest.mark.parametrize("max_hops", [None, 2])
def test_sparse_gcm_with_gin_stack(max_hops):
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    torch.manual_seed(12)
    B, F, H, N = 3, 5, 16, 24
    ref, dev = _sparse_pair(F, H)
    calls = [(torch.randn(B, 6, F), torch.tensor([6, 4, 5])), (torch.randn(B, 6, F), torch.tensor([3, 6, 1]))]
    gws = [torch.randn(B, 6, H) for _ in calls]

    mem = SparseGCM(dev, edge_selectors=TemporalEdge([1]), graph_size=N, max_hops=max_hops)
    assert mem._canonical() is None and not mem._native_gnn()
    hidden, loss, got = None, 0, []
    for (x, taus), gw in zip(calls, gws):
        mx, hidden = mem(x.to(DEV), taus.to(DEV), hidden)
        got.append(mx)
        loss = loss + (mx * gw.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()

    res = {}
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(ref).to(dt)
        h0 = osp.initial_hidden(calls[0][0], N)
        h = (h0[0].to(dt), torch.zeros((B, N, N), dtype=dt, layout=torch.sparse_coo), h0[2])
        loss_r, outs = 0, []
        for (x, taus), gw in zip(calls, gws):
            mx, h = osp.sparse_step(x.to(dt), taus, h, r, graph_size=N, edge_selectors=osp.TemporalEdge([1]),
                                    max_hops=max_hops)
            outs.append(mx)
            loss_r = loss_r + (mx * gw.to(dt)).sum()
        loss_r.backward()
        res[dt] = (outs, h, {k: p.grad for k, p in r.named_parameters()})
    for i, mx in enumerate(got):
        assert_bounded(mx, res[torch.float64][0][i], res[torch.float32][0][i], f"mx[{i}]")
    assert_bounded(hidden[0], res[torch.float64][1][0], res[torch.float32][1][0], "nodes")
    assert torch.equal(hidden[2].cpu(), res[torch.float32][1][2])
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][k], res[torch.float32][2][k], k, floor=GRAD_FLOOR, relative=True)


# ---------------------------------------------------------------------------
# HIP-graph capture, determinism
# ---------------------------------------------------------------------------
def test_cuda_graph_capture_two_layers():
    """Forward + backward of two layers with a trainable eps, captured and replayed: eps is read on the device, so
    the replays equal the eager run - also after eps was changed in place between two replays."""
    from gcm import nn as G
    torch.manual_seed(14)
    c1 = G.DenseGINConv(_nn("mlp", 8, 16), eps=0.2, train_eps=True).to(DEV)
    c2 = G.DenseGINConv(_nn("mlp", 16, 16), eps=-0.1, train_eps=True).to(DEV)
    params = list(c1.parameters()) + list(c2.parameters())
    x = torch.randn(4, 20, 8, device=DEV)
    adj = ((torch.rand(4, 20, 20, device=DEV) < 0.3).float() * torch.rand(4, 20, 20, device=DEV))
    adj.requires_grad_()
    gout = torch.randn(4, 20, 16, device=DEV)

    def step():
        out = c2(torch.tanh(c1(x, adj)), adj)
        out.backward(gout)
        return out

    def eager():
        for p in params + [adj]:
            p.grad = None
        out = step().detach().clone()
        return out, [p.grad.clone() for p in params + [adj]]

    want, want_g = eager()
    with torch.no_grad():
        c1.eps.fill_(0.7)
    want2, want2_g = eager()
    assert not torch.equal(want, want2)
    with torch.no_grad():
        c1.eps.fill_(0.2)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for p in params + [adj]:
                p.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    for p in params + [adj]:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(static_out, want, rtol=0, atol=0)
    for a, b in zip([p.grad for p in params + [adj]], want_g):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    with torch.no_grad():
        c1.eps.fill_(0.7)
    graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(static_out, want2, rtol=0, atol=0)
    for a, b in zip([p.grad for p in params + [adj]], want2_g):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_backward_is_deterministic():
    from gcm import _ops
    torch.manual_seed(15)
    B, N, F = 8, 150, 40
    x = torch.randn(B, N, F, device=DEV)
    adj = torch.rand(B, N, N, device=DEV)
    g = torch.randn(B, N, F, device=DEV)
    runs = []
    for _ in range(2):
        xs, as_, eps = x.clone().requires_grad_(), adj.clone().requires_grad_(), torch.full((1,), 0.3, device=DEV)
        eps.requires_grad_()
        _ops.dense_gin_aggregate(xs, as_, eps, True).backward(g)
        runs.append((xs.grad, as_.grad, eps.grad))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    ei = _with_index(_edges(B * N, 4000, seed=16), B * N)
    runs = []
    for _ in range(2):
        xs, eps = x.view(B * N, F).clone().requires_grad_(), torch.full((1,), 0.3, device=DEV).requires_grad_()
        _ops.csr_gin_aggregate(xs, eps, ei.gcm_graph).backward(g.view(B * N, F))
        runs.append((xs.grad, eps.grad))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)
