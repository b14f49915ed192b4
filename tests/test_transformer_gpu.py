"""DenseTransformerConv / TransformerConv kernels against the eager restatement (tests/_transformer_restate.py),
evaluated in float64 for the bound and in float32 for the restatement's own error.  Needs an MI355X."""
import copy

import pytest
import torch

from _gcn_restate import assert_bounded
from _transformer_restate import DenseTransformerRef, TransformerRef
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _lively(conv):
    """Parameters away from their init: query and key weights x3 and non-zero biases, so the softmax is far from
    uniform."""
    with torch.no_grad():
        conv.lin_query.weight.mul_(3)
        conv.lin_key.weight.mul_(3)
        for lin in (conv.lin_query, conv.lin_key, conv.lin_value, conv.lin_skip):
            if lin is not None and lin.bias is not None:
                lin.bias.uniform_(-0.5, 0.5)
    return conv


def _check(dconv, out, x_grad, ref, run, x, g):
    """`run(module, x)` on the restatement `ref` (the layer's parameters) in float64 and float32 bounds the layer's
    output and every gradient: x and all parameters."""
    res = {}
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(ref).to(dt)
        xr = x.detach().to(dt).requires_grad_()
        o = run(r, xr)
        o.backward(g.to(dt))
        res[dt] = (o, xr.grad, {k: p.grad for k, p in r.named_parameters()})
    o64, x64, p64 = res[torch.float64]
    o32, x32, p32 = res[torch.float32]
    assert out.shape == o64.shape
    assert torch.isfinite(out).all()
    assert_bounded(out, o64, o32, "out")
    assert_bounded(x_grad.reshape(x64.shape), x64, x32, "x", floor=GRAD_FLOOR, relative=True)
    got = dict(dconv.named_parameters())
    assert set(got) == set(p64)
    for k in p64:
        assert got[k].grad is not None, k
        assert_bounded(got[k].grad, p64[k], p32[k], k, floor=GRAD_FLOOR, relative=True)


def _ref_of(conv, cls, Fi, C, H, kw):
    ref = cls(Fi, C, heads=H, **kw)
    ref.load_state_dict(conv.state_dict())
    return ref


# ---------------------------------------------------------------------------
# DenseTransformerConv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,Fi,C,H,opts", [
    (3, 7, 3, 5, 1, {}),
    (3, 7, 3, 5, 2, {"concat": False}),
    (5, 1, 4, 3, 2, {}),                                    # N = 1
    (2, 33, 8, 8, 2, {}),                                   # one past a 32-wide tile
    (2, 130, 16, 8, 4, {}),                                 # past a 128-row block
    (2, 40, 16, 12, 4, {"concat": False}),
    (1, 64, 128, 128, 1, {}),                               # the widest supported layer
    (2, 40, 16, 24, 2, {"empty_rows": True}),
    (3, 33, 8, 8, 2, {"mask": True}),
    (3, 33, 8, 8, 2, {"bias": False}),
    (3, 33, 8, 8, 2, {"root_weight": False}),
    (3, 33, 8, 8, 2, {"beta": True}),
    (3, 33, 8, 6, 3, {"beta": True, "concat": False}),
    (3, 33, 8, 8, 2, {"add_loop": True}),
    (1, 20, 6, 9, 1, {"two_d": True}),
    (4, 20, 6, 9, 2, {"bcast": True}),
    (3, 50, 10, 7, 3, {"weighted": True, "adj_grad": True}),
    (3, 50, 10, 7, 2, {"eval_dropout": True}),
])
def test_dense_transformerconv(B, N, Fi, C, H, opts):
    from gcm import nn as G
    torch.manual_seed(B * 1000 + N + Fi + H)
    concat, add_loop = opts.get("concat", True), opts.get("add_loop", False)
    kw = {"concat": concat, "beta": opts.get("beta", False), "bias": opts.get("bias", True),
          "root_weight": opts.get("root_weight", True)}
    conv = _lively(G.DenseTransformerConv(Fi, C, heads=H, dropout=0.6 if opts.get("eval_dropout") else 0.0, **kw))
    x = torch.randn(B, N, Fi)
    nb = 1 if opts.get("bcast") else B
    adj = (torch.rand(nb, N, N) < 0.3).float()
    if opts.get("weighted"):
        adj = adj * (torch.rand(nb, N, N) * 4 - 2)          # values (negative ones too) are not weights
    if opts.get("empty_rows"):
        adj[:, : N // 4] = 0                                # rows with nothing to attend to
    mask = (torch.rand(B, N) < 0.7) if opts.get("mask") else None
    if opts.get("two_d"):
        x, adj = x[0], adj[0]
    g = torch.randn(B, N, H * C if concat else C)

    dconv = copy.deepcopy(conv).to(DEV)
    if opts.get("eval_dropout"):
        dconv.eval()
    xd, ad = x.to(DEV).requires_grad_(), adj.to(DEV)
    if opts.get("adj_grad"):
        ad.requires_grad_()
    out = dconv(xd, ad, None if mask is None else mask.to(DEV), add_loop=add_loop)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    if opts.get("adj_grad"):
        assert ad.grad is None

    _check(dconv, out, xd.grad, _ref_of(conv, DenseTransformerRef, Fi, C, H, kw),
           lambda r, x_: r(x_, adj.to(x_.dtype), mask, add_loop), x, g)


def test_dense_transformerconv_only_the_pattern_matters():
    from gcm import nn as G
    torch.manual_seed(3)
    conv = _lively(G.DenseTransformerConv(8, 8, heads=2)).to(DEV)
    x = torch.randn(2, 30, 8, device=DEV)
    pat = (torch.rand(2, 30, 30, device=DEV) < 0.3).float()
    weighted = pat * (torch.rand(2, 30, 30, device=DEV) * 5 + 0.1) * torch.where(torch.rand_like(pat) < 0.5, -1, 1)
    torch.testing.assert_close(conv(x, weighted), conv(x, pat), rtol=0, atol=0)


def test_dense_transformerconv_deterministic():
    from gcm import nn as G
    torch.manual_seed(4)
    conv = _lively(G.DenseTransformerConv(32, 8, heads=4, beta=True)).to(DEV)
    x = torch.randn(16, 128, 32, device=DEV, requires_grad=True)
    adj = (torch.rand(16, 128, 128, device=DEV) < 0.2).float()
    g = torch.randn(16, 128, 32, device=DEV)
    runs = []
    for _ in range(2):
        for p in list(conv.parameters()) + [x]:
            p.grad = None
        out = conv(x, adj)
        out.backward(g)
        runs.append([out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in conv.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_transformer_rejects_wide_layers():
    from gcm import nn as G
    with pytest.raises(RuntimeError, match="code -2"):
        G.DenseTransformerConv(129, 8).to(DEV)(torch.randn(2, 5, 129, device=DEV), torch.ones(2, 5, 5, device=DEV))
    with pytest.raises(RuntimeError, match="code -2"):
        G.DenseTransformerConv(8, 43, heads=3).to(DEV)(torch.randn(2, 5, 8, device=DEV),
                                                       torch.ones(2, 5, 5, device=DEV))
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        G.TransformerConv(129, 8).to(DEV)(torch.randn(3, 129, device=DEV), ei)
    with pytest.raises(RuntimeError, match="code -2"):
        G.TransformerConv(8, 129).to(DEV)(torch.randn(3, 8, device=DEV), ei)


# ---------------------------------------------------------------------------
# TransformerConv
# ---------------------------------------------------------------------------
def _edges(M, E, seed):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, M - 3), (2, E), generator=gen)     # the last 3 nodes stay isolated
    if E:
        extra = torch.tensor([[0, 1, 0, 2, 1], [0, 2, 0, 2, 2]])     # duplicate loops (0, 0), duplicate edge 1 -> 2
        ei = torch.cat([ei[:, : E // 2], extra, ei[:, E // 2:]], 1)
    return ei


@pytest.mark.parametrize("M,E,Fi,C,H,opts", [
    (6, 0, 3, 5, 1, {}),                                    # no edges
    (40, 90, 8, 16, 2, {}),
    (40, 90, 8, 6, 3, {"concat": False}),
    (300, 1500, 32, 8, 4, {"edge_attr": True}),
    (129, 700, 128, 128, 1, {}),
    (50, 120, 8, 8, 2, {"beta": True}),
    (50, 120, 8, 8, 2, {"root_weight": False}),
    (50, 120, 8, 8, 2, {"bias": False}),
])
def test_transformerconv(M, E, Fi, C, H, opts):
    from gcm import nn as G
    torch.manual_seed(M + E + Fi + H)
    concat = opts.get("concat", True)
    kw = {"concat": concat, "beta": opts.get("beta", False), "bias": opts.get("bias", True),
          "root_weight": opts.get("root_weight", True)}
    conv = _lively(G.TransformerConv(Fi, C, heads=H, **kw))
    ei = _edges(M, E, seed=M + E)
    x = torch.randn(M, Fi)
    g = torch.randn(M, H * C if concat else C)
    dconv = copy.deepcopy(conv).to(DEV)
    xd = x.to(DEV).requires_grad_()
    attr = torch.randn(ei.shape[1], 3, device=DEV) if opts.get("edge_attr") else None
    out = dconv(xd, ei.to(DEV), attr)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    _check(dconv, out, xd.grad, _ref_of(conv, TransformerRef, Fi, C, H, kw), lambda r, x_: r(x_, ei), x, g)


def test_masked_graph_index_raises():
    from gcm import nn as G, _ops
    M = 5
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]], device=DEV)
    ei.gcm_graph = _ops.GraphIndex(ei, _ops.ptr_from_sorted(ei[1], M), M, mask=torch.ones(M, dtype=torch.bool,
                                                                                          device=DEV))
    with pytest.raises(ValueError, match="masked GraphIndex"):
        G.TransformerConv(4, 4).to(DEV)(torch.randn(M, 4, device=DEV), ei)


def test_dense_equals_sparse():
    from gcm import nn as G
    torch.manual_seed(7)
    B, N, Fi, C, H = 3, 20, 8, 6, 2
    adj = (torch.rand(B, N, N) < 0.25).float()
    adj[:, 3] = 0                                           # a node without in-edges
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])            # adj[b, i, j]: i attends to j, edge j -> i
    dconv = _lively(G.DenseTransformerConv(Fi, C, heads=H, beta=True)).to(DEV)
    sconv = G.TransformerConv(Fi, C, heads=H, beta=True).to(DEV)
    sconv.load_state_dict(dconv.state_dict())
    x = torch.randn(B, N, Fi, device=DEV)
    g = torch.randn(B, N, H * C, device=DEV)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    out_d = dconv(xa, adj.to(DEV))
    out_s = sconv(xb.view(B * N, Fi), ei.to(DEV)).view(B, N, H * C)
    out_d.backward(g)
    out_s.backward(g)
    torch.testing.assert_close(out_d, out_s, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-5)
    sparse = dict(sconv.named_parameters())
    for k, p in dconv.named_parameters():
        torch.testing.assert_close(p.grad, sparse[k].grad, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
def _lively_ref(ref):
    for m in ref.modules():
        if isinstance(m, (DenseTransformerRef, TransformerRef)):
            _lively(m)
    return ref


def _dense_pair(F, H):
    from gcm import nn as G
    ref = _lively_ref(pyg.Sequential("x, adj, weights, B, N", [
        (DenseTransformerRef(F, H // 2, heads=2, beta=True), "x, adj -> x"), torch.nn.ReLU(),
        (DenseTransformerRef(H, H, heads=2, concat=False), "x, adj -> x"), torch.nn.ReLU()]))
    dev = G.Sequential("x, adj, weights, B, N", [
        (G.DenseTransformerConv(F, H // 2, heads=2, beta=True), "x, adj -> x"), torch.nn.ReLU(),
        (G.DenseTransformerConv(H, H, heads=2, concat=False), "x, adj -> x"), torch.nn.ReLU()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _sparse_pair(F, H):
    from gcm import nn as G
    ref = _lively_ref(pyg.Sequential("x, edges, weights", [
        (TransformerRef(F, H // 2, heads=2), "x, edges, weights -> x"), torch.nn.Tanh(),
        (TransformerRef(H, H, beta=True), "x, edges, weights -> x")]))
    dev = G.Sequential("x, edges, weights", [
        (G.TransformerConv(F, H // 2, heads=2), "x, edges, weights -> x"), torch.nn.Tanh(),
        (G.TransformerConv(H, H, beta=True), "x, edges, weights -> x")])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def test_dense_gcm_with_transformer_stack():
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    torch.manual_seed(11)
    B, F, H, N, T = 4, 6, 16, 8, 12               # T > N: the overflow wrap; step 0 is a row with no neighbour
    ref, dev = _dense_pair(F, H)
    obs = torch.randn(T, B, F)
    gw = torch.randn(T, B, H)

    mem = DenseGCM(dev, edge_selectors=TemporalBackedge([1, 2]), graph_size=N)
    assert mem._structure() is None
    hidden, outs = None, []
    for t in range(T):
        mx, hidden = mem(obs[t].to(DEV), hidden)
        outs.append(mx)
    got = torch.stack(outs)
    (got * gw.to(DEV)).sum().backward()
    torch.cuda.synchronize()

    res = {}
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(ref).to(dt)
        want, h = od.dense_rollout(obs.to(dt), None, r, graph_size=N, edge_selectors=od.TemporalBackedge([1, 2]))
        (want * gw.to(dt)).sum().backward()
        res[dt] = (want, h, {k: p.grad for k, p in r.named_parameters()})
    assert_bounded(got, res[torch.float64][0], res[torch.float32][0], "mx")
    assert_bounded(hidden[0], res[torch.float64][1][0], res[torch.float32][1][0], "nodes")
    assert torch.equal(hidden[1].cpu(), res[torch.float32][1][1])
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][k], res[torch.float32][2][k], k, floor=GRAD_FLOOR, relative=True)


@pytest.mark.parametrize("max_hops", [None, 2])
def test_sparse_gcm_with_transformer_stack(max_hops):
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


def test_training_loss_falls():
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    torch.manual_seed(13)
    F, H, B = 4, 16, 8
    _, dg = _dense_pair(F, H)
    _, sg = _sparse_pair(F, H)
    obs = torch.randn(6, B, F, device=DEV)
    target = torch.randn(6, B, H, device=DEV)

    def dense_loss():
        m, hidden, outs = DenseGCM(dg, edge_selectors=TemporalBackedge([1]), graph_size=8), None, []
        for t in range(obs.shape[0]):
            mx, hidden = m(obs[t], hidden)
            outs.append(mx)
        return ((torch.stack(outs) - target) ** 2).mean()

    def sparse_loss():
        m = SparseGCM(sg, edge_selectors=TemporalEdge([1]), graph_size=8)
        mx, _ = m(obs.transpose(0, 1), torch.full((B,), obs.shape[0], device=DEV), None)
        return ((mx - target.transpose(0, 1)) ** 2).mean()

    for net, loss_fn in ((dg, dense_loss), (sg, sparse_loss)):
        opt = torch.optim.Adam(net.parameters(), lr=0.01)
        losses = []
        for _ in range(8):
            opt.zero_grad()
            loss = loss_fn()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert losses[-1] < losses[0], losses


def test_cuda_graph_capture_two_layers():
    from gcm import nn as G
    torch.manual_seed(14)
    c1 = _lively(G.DenseTransformerConv(8, 8, heads=2, beta=True)).to(DEV)
    c2 = _lively(G.DenseTransformerConv(16, 16, heads=2, concat=False)).to(DEV)
    params = list(c1.parameters()) + list(c2.parameters())
    x = torch.randn(4, 20, 8, device=DEV, requires_grad=True)
    adj = (torch.rand(4, 20, 20, device=DEV) < 0.3).float()
    gout = torch.randn(4, 20, 16, device=DEV)

    def step():
        out = c2(torch.relu(c1(x, adj)), adj)
        out.backward(gout)
        return out

    want = step().detach().clone()
    want_g = [p.grad.clone() for p in params] + [x.grad.clone()]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for p in params + [x]:
                p.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    for p in params + [x]:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(static_out, want, rtol=0, atol=0)
    for a, b in zip([p.grad for p in params] + [x.grad], want_g):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
