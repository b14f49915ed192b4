"""DenseGCNConv / GCNConv kernels against the eager restatement (tests/_gcn_restate.py), evaluated in
float64 for the bound and in float32 for the restatement's own error.  Needs an MI355X."""
import copy

import pytest
import torch

from _gcn_restate import DenseGCNRef, GCNRef, assert_bounded, dense_gcn, gcn
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _ref_eval(fn, inputs, g, dtype):
    """fn(*inputs) in dtype with gradients of every floating input -> (out, [grads])."""
    ts = [None if t is None else t.detach().to(dtype).requires_grad_() for t in inputs]
    out = fn(*ts)
    out.backward(g.to(dtype))
    return out, [None if t is None else t.grad for t in ts]


def _check(got, grads_got, fn, inputs, g, names):
    o64, g64 = _ref_eval(fn, inputs, g, torch.float64)
    o32, g32 = _ref_eval(fn, inputs, g, torch.float32)
    assert got.shape == o64.shape
    assert_bounded(got, o64, o32, "out")
    for name, a, b64, b32 in zip(names, grads_got, g64, g32):
        if b64 is None:
            continue
        assert a is not None, name
        assert_bounded(a, b64, b32, name, floor=GRAD_FLOOR, relative=True)


# ---------------------------------------------------------------------------
# DenseGCNConv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,Fi,Fo,weighted,diag,opts", [
    (3, 7, 3, 5, False, False, {}),
    (3, 7, 3, 5, True, True, {}),
    (256, 128, 32, 32, False, False, {}),
    (4, 300, 64, 128, True, True, {}),
    (5, 1, 4, 3, False, True, {}),
    (2, 40, 16, 24, True, True, {"improved": True}),
    (2, 40, 16, 24, True, True, {"add_loop": False}),
    (2, 40, 16, 24, False, False, {"add_loop": False}),
    (3, 33, 8, 8, True, False, {"mask": True}),
    (3, 33, 8, 8, True, False, {"bias": False}),
    (1, 20, 6, 9, True, True, {"two_d": True}),
    (4, 20, 6, 9, True, True, {"bcast": True}),
])
def test_dense_gcnconv(B, N, Fi, Fo, weighted, diag, opts):
    from gcm import nn as G
    torch.manual_seed(B * 1000 + N + Fi)
    improved, add_loop, bias = opts.get("improved", False), opts.get("add_loop", True), opts.get("bias", True)
    conv = G.DenseGCNConv(Fi, Fo, improved=improved, bias=bias)
    if bias:
        torch.nn.init.uniform_(conv.bias, -0.5, 0.5)
    x = torch.randn(B, N, Fi)
    nb = 1 if opts.get("bcast") else B
    adj = (torch.rand(nb, N, N) < 0.3).float()
    if weighted:
        adj = adj * torch.rand(nb, N, N) * 2
    eye = torch.eye(N).expand(nb, N, N)
    adj = adj * (1 - eye) + (eye * torch.rand(nb, N, 1) * 3 if diag else 0)
    mask = (torch.rand(B, N) < 0.7) if opts.get("mask") else None
    if opts.get("two_d"):
        x, adj = x[0], adj[0]
    W, b = conv.lin.weight.detach(), None if conv.bias is None else conv.bias.detach()
    g = torch.randn(B, N, Fo)

    dconv = copy.deepcopy(conv).to(DEV)
    xd, ad = x.to(DEV).requires_grad_(), adj.to(DEV).requires_grad_()
    out = dconv(xd, ad, None if mask is None else mask.to(DEV), add_loop=add_loop)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()

    def fn(x_, a_, W_, b_):
        return dense_gcn(x_, a_, W_, b_, mask, add_loop, improved)

    _check(out, [xd.grad, ad.grad, dconv.lin.weight.grad, None if b is None else dconv.bias.grad],
           fn, [x, adj, W, b], g, ["x", "adj", "weight", "bias"])


def test_dense_gcnconv_rejects_wide_layers():
    from gcm import nn as G
    conv = G.DenseGCNConv(130, 8).to(DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        conv(torch.randn(2, 5, 130, device=DEV), torch.ones(2, 5, 5, device=DEV))


# ---------------------------------------------------------------------------
# GCNConv
# ---------------------------------------------------------------------------
def _edges(M, E, seed, loops=True):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, M - 3), (2, E), generator=gen)     # the last 3 nodes stay isolated
    if E and loops:
        extra = torch.tensor([[0, 1, 0, 2, 1], [0, 2, 0, 2, 2]])     # duplicate loops (0, 0), duplicate edge 1 -> 2
        ei = torch.cat([ei[:, : E // 2], extra, ei[:, E // 2:]], 1)
    return ei


@pytest.mark.parametrize("M,E,Fi,Fo,weighted,opts", [
    (6, 0, 3, 5, False, {}),
    (6, 0, 3, 5, True, {"add_self_loops": False}),
    (40, 90, 8, 16, True, {}),
    (40, 90, 8, 16, False, {}),
    (300, 1500, 32, 32, True, {"improved": True}),
    (300, 1500, 32, 32, True, {"add_self_loops": False}),
    (300, 1500, 33, 70, True, {"normalize": False}),
    (129, 700, 128, 128, True, {}),
    (50, 120, 8, 8, True, {"bias": False}),
])
def test_gcnconv(M, E, Fi, Fo, weighted, opts):
    from gcm import nn as G
    torch.manual_seed(M + E + Fi)
    kw = {k: opts[k] for k in ("improved", "add_self_loops", "normalize", "bias") if k in opts}
    conv = G.GCNConv(Fi, Fo, **kw)
    if conv.bias is not None:
        torch.nn.init.uniform_(conv.bias, -0.5, 0.5)
    ei = _edges(M, E, seed=M + E)
    Et = ei.shape[1]
    w = torch.rand(Et) + 0.5 if weighted else None
    x = torch.randn(M, Fi)
    g = torch.randn(M, Fo)
    W, b = conv.lin.weight.detach(), None if conv.bias is None else conv.bias.detach()

    dconv = copy.deepcopy(conv).to(DEV)
    xd = x.to(DEV).requires_grad_()
    wd = None if w is None else w.to(DEV).requires_grad_()
    out = dconv(xd, ei.to(DEV), wd)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()

    def fn(x_, w_, W_, b_):
        return gcn(x_, ei, W_, b_, w_, kw.get("improved", False), kw.get("add_self_loops", True),
                   kw.get("normalize", True))

    _check(out, [xd.grad, None if wd is None else wd.grad, dconv.lin.weight.grad,
                 None if b is None else dconv.bias.grad], fn, [x, w, W, b], g,
           ["x", "edge_weight", "weight", "bias"])


def test_gcnconv_cfg4_size():
    """512 graphs x 512 nodes, TemporalEdge([1]) edges, weights with a gradient."""
    from gcm import nn as G
    torch.manual_seed(4)
    Bg, N, F = 512, 512, 32
    M = Bg * N
    t = torch.arange(M)
    keep = t % N != 0
    ei = torch.stack([t[keep] - 1, t[keep]])
    w = torch.rand(ei.shape[1]) + 0.5
    conv = G.GCNConv(F, F)
    torch.nn.init.uniform_(conv.bias, -0.5, 0.5)
    x, g = torch.randn(M, F), torch.randn(M, F)
    dconv = copy.deepcopy(conv).to(DEV)
    xd, wd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    out = dconv(xd, ei.to(DEV), wd)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    W, b = conv.lin.weight.detach(), conv.bias.detach()
    _check(out, [xd.grad, wd.grad, dconv.lin.weight.grad, dconv.bias.grad],
           lambda x_, w_, W_, b_: gcn(x_, ei, W_, b_, w_), [x, w, W, b], g, ["x", "edge_weight", "weight", "bias"])


def test_dense_equals_sparse():
    from gcm import nn as G
    torch.manual_seed(7)
    B, N, Fi, Fo = 3, 20, 8, 12
    adj = (torch.rand(B, N, N) < 0.25).float() * (torch.rand(B, N, N) + 0.5)
    adj = adj * (1 - torch.eye(N))
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])        # adj[b, i, j]: edge j -> i
    w = adj[bb, ii, jj]
    dconv = G.DenseGCNConv(Fi, Fo).to(DEV)
    torch.nn.init.uniform_(dconv.bias, -0.5, 0.5)
    sconv = G.GCNConv(Fi, Fo).to(DEV)
    sconv.load_state_dict(dconv.state_dict())
    x = torch.randn(B, N, Fi, device=DEV)
    g = torch.randn(B, N, Fo, device=DEV)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    out_d = dconv(xa, adj.to(DEV))
    out_s = sconv(xb.view(B * N, Fi), ei.to(DEV), w.to(DEV)).view(B, N, Fo)
    out_d.backward(g)
    out_s.backward(g)
    torch.testing.assert_close(out_d, out_s, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
def _dense_pair(F, H):
    from gcm import nn as G
    ref = pyg.Sequential("x, adj, weights, B, N", [(DenseGCNRef(F, H), "x, adj -> x"), torch.nn.ReLU(),
                                                   (DenseGCNRef(H, H), "x, adj -> x"), torch.nn.ReLU()])
    for m in ref.modules():
        if isinstance(m, DenseGCNRef):
            torch.nn.init.uniform_(m.bias, -0.3, 0.3)
    dev = G.Sequential("x, adj, weights, B, N", [(G.DenseGCNConv(F, H), "x, adj -> x"), torch.nn.ReLU(),
                                                 (G.DenseGCNConv(H, H), "x, adj -> x"), torch.nn.ReLU()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _ref_params(ref, dtype):
    r = copy.deepcopy(ref).to(dtype)
    return r


def test_dense_gcm_with_gcn_stack():
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
        r = _ref_params(ref, dt)
        want, h = od.dense_rollout(obs.to(dt), None, r, graph_size=N,
                                   edge_selectors=od.TemporalBackedge([1, 2]))
        (want * gw.to(dt)).sum().backward()
        res[dt] = (want, h, {k: p.grad for k, p in r.named_parameters()})
    assert_bounded(got, res[torch.float64][0], res[torch.float32][0], "mx")
    assert_bounded(hidden[0], res[torch.float64][1][0], res[torch.float32][1][0], "nodes")
    assert torch.equal(hidden[1].cpu(), res[torch.float32][1][1])
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][k], res[torch.float32][2][k], k, floor=GRAD_FLOOR, relative=True)


def test_dense_gcm_with_gcn_stack_learned_edge():
    """LearnedEdge hands the GNN an adjacency with a gradient: the edge network learns only through
    DenseGCNConv's g_adj, degree term included.  Gumbel draws injected into both sides."""
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.learned import LearnedEdge
    torch.manual_seed(21)
    B, F, H, N, T, k = 4, 6, 16, 8, 12, 3          # T > N: the overflow wrap
    ref, dev = _dense_pair(F, H)
    net = od.build_edge_network(F)
    with torch.no_grad():                           # livelier than the default init: the sampled rows vary
        for p in net.parameters():
            p.mul_(2.0)
    sel = LearnedEdge(F, num_edge_samples=k)
    sel.edge_network.load_state_dict(net.state_dict())
    sel = sel.to(DEV)
    gen = torch.Generator().manual_seed(22)
    obs = torch.randn(T, B, F, generator=gen)
    noise = -torch.empty(T, B, N).exponential_(generator=gen).log()
    gw = torch.randn(T, B, H, generator=gen)
    step = {"t": 0}
    sel.noise_fn = lambda like: noise[step["t"]].to(DEV)

    mem = DenseGCM(dev, edge_selectors=sel, graph_size=N)
    assert mem._structure() is None
    hidden, outs = None, []
    for t in range(T):
        step["t"] = t
        mx, hidden = mem(obs[t].to(DEV), hidden)
        outs.append(mx)
    got = torch.stack(outs)
    (got * gw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert hidden[1].requires_grad

    res = {}
    for dt in (torch.float64, torch.float32):
        r, n_ = _ref_params(ref, dt), copy.deepcopy(net).to(dt)
        osel = od.LearnedEdge(n_, num_edge_samples=k, noise_fn=lambda shape: noise[step["t"]][:, : shape[1]].to(dt))
        h, o = None, []
        for t in range(T):
            step["t"] = t
            mx, h = od.dense_step(obs[t].to(dt), h, r, graph_size=N, edge_selectors=osel)
            o.append(mx)
        want = torch.stack(o)
        (want * gw.to(dt)).sum().backward()
        grads = {kk: p.grad for kk, p in r.named_parameters()}
        grads.update({"net." + kk: p.grad for kk, p in n_.named_parameters()})
        res[dt] = (want, h, grads)
    r64, r32 = res[torch.float64], res[torch.float32]
    assert torch.equal(r64[1][1].detach().float(), r32[1][1].detach()), "the oracle's two precisions sampled different edges"
    assert torch.equal(hidden[1].detach().cpu(), r32[1][1].detach())           # sampled edges: bit exact
    assert_bounded(got, r64[0], r32[0], "mx")
    assert_bounded(hidden[0], r64[1][0], r32[1][0], "nodes")
    for kk, p in dev.named_parameters():
        assert_bounded(p.grad, r64[2][kk], r32[2][kk], kk, floor=GRAD_FLOOR, relative=True)
    net_scale = max(float(v.abs().max()) for kk, v in r64[2].items() if kk.startswith("net."))
    assert net_scale > 0
    for kk, p in sel.edge_network.named_parameters():
        g64, g32 = r64[2]["net." + kk], r32[2]["net." + kk]
        err = float((p.grad.cpu().double() - g64).abs().max())
        own = float((g32.double() - g64).abs().max())
        # (floor on the edge network's common scale, as tests/test_learned_fused_gpu.py: biases after the
        #  softmax get sum_j g_logit[j] = 0 analytically)
        assert err <= max(3.0 * own, 2e-6 * net_scale), (kk, err, own, net_scale)


def _sparse_pair(F, H):
    from gcm import nn as G
    ref = pyg.Sequential("x, edges, weights", [(GCNRef(F, H), "x, edges, weights -> x"), torch.nn.Tanh(),
                                               (GCNRef(H, H), "x, edges, weights -> x")])
    for m in ref.modules():
        if isinstance(m, GCNRef):
            torch.nn.init.uniform_(m.bias, -0.3, 0.3)
    dev = G.Sequential("x, edges, weights", [(G.GCNConv(F, H), "x, edges, weights -> x"), torch.nn.Tanh(),
                                             (G.GCNConv(H, H), "x, edges, weights -> x")])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


@pytest.mark.parametrize("max_hops", [None, 2])
def test_sparse_gcm_with_gcn_stack(max_hops):
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
        r = _ref_params(ref, dt)
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
    """A few Adam steps in the reference test's style (tests/test_gcm.py:442-550) on both memories."""
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
    c1, c2 = G.DenseGCNConv(8, 16).to(DEV), G.DenseGCNConv(16, 16).to(DEV)
    torch.nn.init.uniform_(c1.bias, -0.3, 0.3)
    params = list(c1.parameters()) + list(c2.parameters())
    x = torch.randn(4, 20, 8, device=DEV)
    adj = ((torch.rand(4, 20, 20, device=DEV) < 0.3).float() * torch.rand(4, 20, 20, device=DEV))
    adj.requires_grad_()
    gout = torch.randn(4, 20, 16, device=DEV)

    def step():
        out = c2(torch.relu(c1(x, adj)), adj)
        out.backward(gout)
        return out

    want = step().detach().clone()
    want_g = [p.grad.clone() for p in params] + [adj.grad.clone()]

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
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(static_out, want, rtol=0, atol=0)
    for a, b in zip([p.grad for p in params] + [adj.grad], want_g):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
