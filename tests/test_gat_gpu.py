"""DenseGATConv / GATConv kernels against the eager restatement (tests/_gat_restate.py), evaluated in
float64 for the bound and in float32 for the restatement's own error.  Needs an MI355X."""
import copy

import pytest
import torch

from _gat_restate import DenseGATRef, GATRef, dense_gat, gat
from _gcn_restate import assert_bounded
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _ref_eval(fn, inputs, g, dtype):
    ts = [None if t is None else t.detach().to(dtype).requires_grad_() for t in inputs]
    out = fn(*ts)
    out.backward(g.to(dtype))
    return out, [None if t is None else t.grad for t in ts]


def _check(got, grads_got, fn, inputs, g, names):
    o64, g64 = _ref_eval(fn, inputs, g, torch.float64)
    o32, g32 = _ref_eval(fn, inputs, g, torch.float32)
    assert got.shape == o64.shape
    assert torch.isfinite(got).all()
    assert_bounded(got, o64, o32, "out")
    for name, a, b64, b32 in zip(names, grads_got, g64, g32):
        if b64 is None:
            continue
        assert a is not None, name
        assert_bounded(a.reshape(b64.shape), b64, b32, name, floor=GRAD_FLOOR, relative=True)


def _lively(conv):
    """Attention vectors and bias away from their init, so the softmax is far from uniform."""
    with torch.no_grad():
        conv.att_src.normal_(0, 0.7)
        conv.att_dst.normal_(0, 0.7)
        if conv.bias is not None:
            conv.bias.uniform_(-0.5, 0.5)
    return conv


def _params(conv):
    b = None if conv.bias is None else conv.bias.detach()
    return [conv.lin.weight.detach(), conv.att_src.detach(), conv.att_dst.detach(), b]


def _grads(conv):
    return [conv.lin.weight.grad, conv.att_src.grad, conv.att_dst.grad, None if conv.bias is None else conv.bias.grad]


# ---------------------------------------------------------------------------
# DenseGATConv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,Fi,C,H,opts", [
    (3, 7, 3, 5, 1, {}),
    (3, 7, 3, 5, 2, {"concat": False}),
    (5, 1, 4, 3, 2, {}),
    (256, 128, 32, 32, 1, {}),
    (256, 128, 32, 8, 4, {}),
    (4, 300, 64, 32, 4, {}),
    (4, 300, 64, 128, 1, {"concat": False}),
    (2, 40, 16, 12, 4, {"concat": False, "slope": 0.05}),
    (2, 40, 16, 24, 2, {"add_loop": False, "empty_rows": True}),
    (3, 33, 8, 8, 2, {"mask": True}),
    (3, 33, 8, 8, 2, {"bias": False, "slope": 0.5}),
    (1, 20, 6, 9, 1, {"two_d": True}),
    (4, 20, 6, 9, 2, {"bcast": True}),
    (3, 50, 10, 7, 3, {"weighted": True, "adj_grad": True}),
    (3, 50, 10, 7, 2, {"eval_dropout": True}),
])
def test_dense_gatconv(B, N, Fi, C, H, opts):
    from gcm import nn as G
    torch.manual_seed(B * 1000 + N + Fi + H)
    concat, add_loop, slope = opts.get("concat", True), opts.get("add_loop", True), opts.get("slope", 0.2)
    conv = _lively(G.DenseGATConv(Fi, C, heads=H, concat=concat, negative_slope=slope, bias=opts.get("bias", True),
                                  dropout=0.6 if opts.get("eval_dropout") else 0.0))
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

    def fn(x_, W_, as_, ad_, b_):
        return dense_gat(x_, adj, W_, as_, ad_, b_, H, concat, slope, mask, add_loop)

    _check(out, [xd.grad] + _grads(dconv), fn, [x] + _params(conv), g,
           ["x", "weight", "att_src", "att_dst", "bias"])


def test_dense_gatconv_only_the_pattern_matters():
    from gcm import nn as G
    torch.manual_seed(3)
    conv = _lively(G.DenseGATConv(8, 8, heads=2)).to(DEV)
    x = torch.randn(2, 30, 8, device=DEV)
    pat = (torch.rand(2, 30, 30, device=DEV) < 0.3).float()
    weighted = pat * (torch.rand(2, 30, 30, device=DEV) * 5 + 0.1) * torch.where(torch.rand_like(pat) < 0.5, -1, 1)
    torch.testing.assert_close(conv(x, weighted), conv(x, pat), rtol=0, atol=0)


def test_dense_gatconv_deterministic():
    from gcm import nn as G
    torch.manual_seed(4)
    conv = _lively(G.DenseGATConv(32, 8, heads=4)).to(DEV)
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


def test_gat_rejects_wide_layers():
    from gcm import nn as G
    with pytest.raises(RuntimeError, match="code -2"):
        G.DenseGATConv(129, 8).to(DEV)(torch.randn(2, 5, 129, device=DEV), torch.ones(2, 5, 5, device=DEV))
    with pytest.raises(RuntimeError, match="code -2"):
        G.DenseGATConv(8, 43, heads=3).to(DEV)(torch.randn(2, 5, 8, device=DEV), torch.ones(2, 5, 5, device=DEV))
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        G.GATConv(8, 129).to(DEV)(torch.randn(3, 8, device=DEV), ei)


# ---------------------------------------------------------------------------
# GATConv
# ---------------------------------------------------------------------------
def _edges(M, E, seed, loops=True):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, M - 3), (2, E), generator=gen)     # the last 3 nodes stay isolated
    if E and loops:
        extra = torch.tensor([[0, 1, 0, 2, 1], [0, 2, 0, 2, 2]])     # duplicate loops (0, 0), duplicate edge 1 -> 2
        ei = torch.cat([ei[:, : E // 2], extra, ei[:, E // 2:]], 1)
    return ei


@pytest.mark.parametrize("M,E,Fi,C,H,opts", [
    (6, 0, 3, 5, 1, {}),
    (6, 0, 3, 5, 2, {"add_self_loops": False}),
    (40, 90, 8, 16, 2, {}),
    (40, 90, 8, 6, 3, {"add_self_loops": False}),
    (40, 90, 8, 6, 4, {"concat": False, "slope": 0.01}),
    (300, 1500, 32, 32, 1, {}),
    (300, 1500, 32, 8, 4, {"edge_attr": True}),
    (129, 700, 128, 128, 1, {}),
    (129, 700, 64, 32, 4, {"concat": False}),
    (50, 120, 8, 8, 2, {"bias": False}),
])
def test_gatconv(M, E, Fi, C, H, opts):
    from gcm import nn as G
    torch.manual_seed(M + E + Fi + H)
    concat, loops, slope = opts.get("concat", True), opts.get("add_self_loops", True), opts.get("slope", 0.2)
    conv = _lively(G.GATConv(Fi, C, heads=H, concat=concat, negative_slope=slope, add_self_loops=loops,
                             bias=opts.get("bias", True)))
    ei = _edges(M, E, seed=M + E)
    x = torch.randn(M, Fi)
    g = torch.randn(M, H * C if concat else C)
    dconv = copy.deepcopy(conv).to(DEV)
    xd = x.to(DEV).requires_grad_()
    attr = torch.randn(ei.shape[1], 3, device=DEV) if opts.get("edge_attr") else None
    out = dconv(xd, ei.to(DEV), attr)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()

    def fn(x_, W_, as_, ad_, b_):
        return gat(x_, ei, W_, as_, ad_, b_, H, concat, slope, loops)

    _check(out, [xd.grad] + _grads(dconv), fn, [x] + _params(conv), g, ["x", "weight", "att_src", "att_dst", "bias"])


def test_dense_equals_sparse():
    from gcm import nn as G
    torch.manual_seed(7)
    B, N, Fi, C, H = 3, 20, 8, 6, 2
    adj = (torch.rand(B, N, N) < 0.25).float()
    adj[:, 3] = 0                                           # nodes without in-edges besides their loop
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])            # adj[b, i, j]: i attends to j, edge j -> i
    dconv = _lively(G.DenseGATConv(Fi, C, heads=H)).to(DEV)
    sconv = G.GATConv(Fi, C, heads=H).to(DEV)
    sd = dconv.state_dict()
    sd["att_src"], sd["att_dst"] = sd["att_src"].view(1, H, C), sd["att_dst"].view(1, H, C)
    sconv.load_state_dict(sd)
    x = torch.randn(B, N, Fi, device=DEV)
    g = torch.randn(B, N, H * C, device=DEV)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    out_d = dconv(xa, adj.to(DEV))
    out_s = sconv(xb.view(B * N, Fi), ei.to(DEV)).view(B, N, H * C)
    out_d.backward(g)
    out_s.backward(g)
    torch.testing.assert_close(out_d, out_s, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-5)
    for k in ("lin.weight", "att_src", "att_dst", "bias"):
        a = dict(dconv.named_parameters())[k].grad
        b = dict(sconv.named_parameters())[k].grad
        torch.testing.assert_close(a.reshape(b.shape), b, rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
def _lively_ref(ref):
    for m in ref.modules():
        if isinstance(m, (DenseGATRef, GATRef)):
            torch.nn.init.uniform_(m.bias, -0.3, 0.3)
    return ref


def _dense_pair(F, H):
    from gcm import nn as G
    ref = _lively_ref(pyg.Sequential("x, adj, weights, B, N", [
        (DenseGATRef(F, H // 2, heads=2), "x, adj -> x"), torch.nn.ReLU(),
        (DenseGATRef(H, H, heads=2, concat=False), "x, adj -> x"), torch.nn.ReLU()]))
    dev = G.Sequential("x, adj, weights, B, N", [
        (G.DenseGATConv(F, H // 2, heads=2), "x, adj -> x"), torch.nn.ReLU(),
        (G.DenseGATConv(H, H, heads=2, concat=False), "x, adj -> x"), torch.nn.ReLU()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _sparse_pair(F, H):
    from gcm import nn as G
    ref = _lively_ref(pyg.Sequential("x, edges, weights", [
        (GATRef(F, H // 2, heads=2), "x, edges, weights -> x"), torch.nn.Tanh(),
        (GATRef(H, H), "x, edges, weights -> x")]))
    dev = G.Sequential("x, edges, weights", [
        (G.GATConv(F, H // 2, heads=2), "x, edges, weights -> x"), torch.nn.Tanh(),
        (G.GATConv(H, H), "x, edges, weights -> x")])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def test_dense_gcm_with_gat_stack():
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    torch.manual_seed(11)
    B, F, H, N, T = 4, 6, 16, 8, 12               # T > N: the overflow wrap
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
def test_sparse_gcm_with_gat_stack(max_hops):
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
    c1 = _lively(G.DenseGATConv(8, 8, heads=2)).to(DEV)
    c2 = _lively(G.DenseGATConv(16, 16, heads=2, concat=False)).to(DEV)
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
