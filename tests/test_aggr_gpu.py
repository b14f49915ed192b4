"""Mean / max aggregation kernels (GraphConv(aggr=...), DenseGraphConv(aggr=...), SAGEConv, DenseSAGEConv) against the
eager restatement (tests/_aggr_restate.py), evaluated in float64 for the bound and in float32 for the restatement's
own error.  Needs an MI355X."""
import copy

import pytest
import torch

from _aggr_restate import (DenseGraphConvRef, DenseSAGERef, GraphConvRef, SAGERef, dense_aggr_conv, random_edges,
                           sparse_aggr_conv, sparse_max_margin, weighted_max_case)
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
    with torch.no_grad():
        for n, p in conv.named_parameters():
            if n.endswith("bias"):
                p.uniform_(-0.5, 0.5)
    return conv


def _grad(p):
    return None if p is None else p.grad


# ---------------------------------------------------------------------------
# dense layers
# ---------------------------------------------------------------------------
def _dense_layer(kind, Fi, Fo, bias=True):
    """(module, the state-dict names of [w_rel, w_root, bias] (None: absent), aggr)"""
    from gcm import nn as G
    if kind == "sage":
        return _lively(G.DenseSAGEConv(Fi, Fo, bias=bias)), \
            ["lin_rel.weight", "lin_root.weight", "lin_root.bias" if bias else None], "mean"
    return _lively(G.DenseGraphConv(Fi, Fo, aggr=kind, bias=bias)), \
        ["lin_rel.weight", "lin_root.weight", "lin_rel.bias" if bias else None], kind


def _adjacency(nb, N, weighted, empty_rows=True):
    adj = (torch.rand(nb, N, N) < 0.3).float()
    if weighted:                                        # weights of both signs, some rows summing below 1
        adj = adj * (torch.rand(nb, N, N) * 2 - 0.5)
    if empty_rows and N > 2:
        adj[:, 1] = 0
    return adj


@pytest.mark.parametrize("kind", ["mean", "max", "sage"])
@pytest.mark.parametrize("B,N,Fi,Fo,weighted,opts", [
    (3, 7, 3, 5, False, {}),
    (3, 7, 3, 5, True, {}),
    (256, 128, 32, 32, False, {}),
    (4, 300, 64, 128, True, {}),
    (2, 70, 128, 33, True, {}),
    (5, 1, 4, 3, False, {}),
    (5, 1, 4, 3, True, {"self": True}),
    (3, 33, 8, 8, True, {"mask": True}),
    (3, 33, 8, 8, True, {"bias": False}),
    (1, 20, 6, 9, True, {"two_d": True}),
    (4, 20, 6, 9, True, {"bcast": True}),
])
def test_dense_layers(kind, B, N, Fi, Fo, weighted, opts):
    torch.manual_seed(B * 1000 + N + Fi)
    conv, names, aggr = _dense_layer(kind, Fi, Fo, opts.get("bias", True))
    x = torch.randn(B, N, Fi)
    nb = 1 if opts.get("bcast") else B
    adj = _adjacency(nb, N, weighted)
    if opts.get("self"):
        adj = torch.full((nb, N, N), 0.4)
    mask = (torch.rand(B, N) < 0.7) if opts.get("mask") else None
    if opts.get("two_d"):
        x, adj = x[0], adj[0]
    g = torch.randn(B, N, Fo)
    sd = {k: v.detach().clone() for k, v in conv.state_dict().items()}
    wr, wo, b = (None if n is None else sd[n] for n in names)

    dconv = copy.deepcopy(conv).to(DEV)
    xd, ad = x.to(DEV).requires_grad_(), adj.to(DEV).requires_grad_()
    out = dconv(xd, ad, None if mask is None else mask.to(DEV))
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    by_name = dict(dconv.named_parameters())
    grads = [None if n is None else by_name[n].grad for n in names]
    if aggr == "max":
        assert ad.grad is None                      # only the pattern is read: adj gets no gradient

    def fn(x_, a_, wr_, wo_, b_):
        return dense_aggr_conv(x_, adj if a_ is None else a_, wr_, wo_, b_, aggr, mask)

    _check(out, [xd.grad, ad.grad] + grads, fn, [x, adj if aggr == "mean" else None, wr, wo, b], g,
           ["x", "adj", "w_rel", "w_root", "bias"])


def test_dense_layers_reject_wide_layers():
    from gcm import nn as G
    for conv in (G.DenseGraphConv(130, 8, aggr="mean"), G.DenseGraphConv(8, 130, aggr="max"), G.DenseSAGEConv(130, 8)):
        conv = conv.to(DEV)
        with pytest.raises(RuntimeError, match="code -2"):
            conv(torch.randn(2, 5, conv.in_channels, device=DEV), torch.ones(2, 5, 5, device=DEV))
    with pytest.raises(RuntimeError, match="code -2"):
        G.GraphConv(130, 8, aggr="max").to(DEV)(torch.randn(4, 130, device=DEV), torch.tensor([[0, 1], [1, 2]], device=DEV))


# ---------------------------------------------------------------------------
# sparse layers
# ---------------------------------------------------------------------------
def _sparse_layer(kind, aggr, Fi, Fo, bias=True, root_weight=True):
    from gcm import nn as G
    if kind == "sage":
        conv = _lively(G.SAGEConv(Fi, Fo, aggr=aggr, root_weight=root_weight, bias=bias))
        return conv, ["lin_l.weight", "lin_r.weight" if root_weight else None, "lin_l.bias" if bias else None]
    conv = _lively(G.GraphConv(Fi, Fo, aggr=aggr, bias=bias))
    return conv, ["lin_rel.weight", "lin_root.weight", "lin_rel.bias" if bias else None]


def _run_sparse(conv, names, aggr, x, ei, w, g, graph=None):
    """The layer on the device against the restatement: outputs and every gradient."""
    sd = {k: v.detach().clone() for k, v in conv.state_dict().items()}
    dconv = copy.deepcopy(conv).to(DEV)
    xd = x.to(DEV).requires_grad_()
    wd = None if w is None else w.to(DEV).requires_grad_()
    eid = ei.to(DEV)
    if graph is not None:
        eid.gcm_graph = graph(eid)
    out = dconv(xd, eid) if w is None else dconv(xd, eid, wd)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    by_name = dict(dconv.named_parameters())
    wr, wo, b = (None if n is None else sd[n] for n in names)

    def fn(x_, w_, wr_, wo_, b_):
        return sparse_aggr_conv(x_, ei, wr_, wo_, b_, w_, aggr)

    _check(out, [xd.grad, _grad(wd)] + [None if n is None else by_name[n].grad for n in names],
           fn, [x, w, wr, wo, b], g, ["x", "edge_weight", "w_rel", "w_root", "bias"])
    return out, xd.grad, _grad(wd)


@pytest.mark.parametrize("aggr", ["mean", "max"])
@pytest.mark.parametrize("kind,M,E,Fi,Fo,weighted,opts", [
    ("graph", 6, 0, 3, 5, False, {}),                 # no edges at all
    ("graph", 6, 0, 3, 5, True, {}),
    ("sage", 6, 0, 3, 5, False, {}),
    ("graph", 1, 0, 4, 3, False, {}),
    ("graph", 40, 90, 8, 16, True, {}),
    ("graph", 40, 90, 8, 16, False, {}),              # duplicate unit-weight edges: g_x (there is no g_w)
    ("sage", 40, 90, 8, 16, False, {}),
    ("sage", 40, 90, 8, 16, False, {"root_weight": False}),
    ("sage", 50, 120, 8, 8, False, {"bias": False}),
    ("graph", 50, 120, 8, 8, True, {"bias": False}),
    ("graph", 300, 1500, 32, 32, True, {}),
    ("graph", 300, 1500, 33, 70, False, {}),
    ("graph", 129, 700, 128, 128, True, {}),
    ("sage", 129, 700, 128, 128, False, {}),
    ("graph", 64, 2000, 16, 16, True, {}),            # heavy fan-in: ~33 edges per node
])
def test_sparse_layers(kind, aggr, M, E, Fi, Fo, weighted, opts):
    seed = M + E * 10 + Fi * 100 + (1 if aggr == "max" else 0)
    torch.manual_seed(seed)
    conv, names = _sparse_layer(kind, aggr, Fi, Fo, opts.get("bias", True), opts.get("root_weight", True))
    if weighted:
        x, ei, w = weighted_max_case(M, E, Fi, {(40, 90): 130, (300, 1500): 1832, (129, 700): 957, (64, 2000): 77,
                                               (50, 120): 170, (6, 0): 6}[(M, E)])
        if aggr == "max":       # near ties of w_e x_src could go either way in fp32: these seeds have none
            near = sparse_max_margin(x, ei, w) < 1e-5
            assert int(near.sum()) <= 1e-3 * near.numel() and int(near.sum()) == 0
    else:
        x, ei, w = torch.randn(M, Fi), random_edges(M, E, seed), None
    _run_sparse(conv, names, aggr, x, ei, w, torch.randn(M, Fo))


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_sparse_wrong_length_and_unit_weights_are_ignored(aggr):
    from gcm import nn as G
    torch.manual_seed(3)
    M, Fi, Fo = 30, 6, 7
    ei = random_edges(M, 80, 5).to(DEV)
    conv = _lively(G.GraphConv(Fi, Fo, aggr=aggr)).to(DEV)
    x = torch.randn(M, Fi, device=DEV)
    want = conv(x, ei)
    assert torch.equal(conv(x, ei, torch.rand(7, device=DEV)), want)
    unit = torch.rand(ei.shape[1], device=DEV)
    unit.gcm_unit_weights = True
    assert torch.equal(conv(x, ei, unit), want)


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_sparse_attached_index_and_ragged_rows(aggr):
    """A ready CSR attached to the edge list (what SparseGCM hands over: no csr_perm) with ragged rows: in-degrees
    0 .. 40 in one graph."""
    from gcm import _ops
    torch.manual_seed(8)
    M, Fi, Fo = 41, 9, 6
    dst = torch.cat([torch.full((d,), d) for d in range(M)])               # node d has d in-edges
    src = torch.cat([torch.randperm(M)[:d] for d in range(M)])
    ei = torch.stack([src, dst])
    x, w = torch.randn(M, Fi), torch.rand(ei.shape[1]) + 0.5
    assert int((sparse_max_margin(x, ei, w) < 1e-5).sum()) == 0

    def attach(eid):
        graph = _ops.GraphIndex(eid, _ops.ptr_from_sorted(eid[1], M), M)
        assert graph.csr_perm is None
        return graph

    conv, names = _sparse_layer("graph", aggr, Fi, Fo)
    _run_sparse(conv, names, aggr, x, ei, w, torch.randn(M, Fo), graph=attach)
    shuffle = torch.randperm(ei.shape[1])               # the same edges in another order: indexed with a csr_perm
    _run_sparse(conv, names, aggr, x, ei[:, shuffle], w[shuffle], torch.randn(M, Fo))


def test_sparse_cfg4_size():
    """512 graphs x 512 nodes, TemporalEdge([1]) edges, weights with a gradient."""
    torch.manual_seed(4)
    Bg, N, F = 512, 512, 32
    M = Bg * N
    t = torch.arange(M)
    keep = t % N != 0
    ei = torch.stack([t[keep] - 1, t[keep]])
    w = torch.rand(ei.shape[1]) + 0.5
    x, g = torch.randn(M, F), torch.randn(M, F)
    for aggr in ("mean", "max"):
        conv, names = _sparse_layer("graph", aggr, F, F)
        _run_sparse(conv, names, aggr, x, ei, w, g)


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_dense_equals_sparse(aggr):
    from gcm import nn as G
    torch.manual_seed(7)
    B, N, Fi, Fo = 3, 20, 8, 12
    adj = (torch.rand(B, N, N) < 0.25).float()
    adj[:, 4] = 0
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])        # adj[b, i, j]: edge j -> i
    dconv = _lively(G.DenseGraphConv(Fi, Fo, aggr=aggr)).to(DEV)
    sconv = G.GraphConv(Fi, Fo, aggr=aggr).to(DEV)
    sconv.load_state_dict(dconv.state_dict())
    x = torch.randn(B, N, Fi, device=DEV)
    g = torch.randn(B, N, Fo, device=DEV)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    out_d = dconv(xa, adj.to(DEV))
    out_s = sconv(xb.view(B * N, Fi), ei.to(DEV)).view(B, N, Fo)
    out_d.backward(g)
    out_s.backward(g)
    torch.testing.assert_close(out_d, out_s, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------
# reproducibility and graph capture
# ---------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal():
    from gcm import nn as G
    torch.manual_seed(15)
    B, N, F = 8, 96, 48
    x = torch.randn(B, N, F, device=DEV)
    adj = _adjacency(B, N, True).to(DEV)
    g = torch.randn(B, N, F, device=DEV)
    ei = random_edges(B * N, 6000, 3).to(DEV)
    w = (torch.rand(ei.shape[1], device=DEV) + 0.5)

    def dense(conv):
        xa, aa = x.clone().requires_grad_(), adj.clone().requires_grad_()
        conv.zero_grad()
        out = conv(xa, aa)
        out.backward(g)
        return [out.detach(), xa.grad] + ([aa.grad] if aa.grad is not None else []) + [p.grad.clone() for p in conv.parameters()]

    def sparse(conv):
        xa, wa = x.view(B * N, F).clone().requires_grad_(), w.clone().requires_grad_()
        conv.zero_grad()
        out = conv(xa, ei, wa)
        out.backward(g.view(B * N, F))
        return [out.detach(), xa.grad, wa.grad] + [p.grad.clone() for p in conv.parameters()]

    for aggr in ("mean", "max"):
        for run, conv in ((dense, G.DenseGraphConv(F, F, aggr=aggr)), (sparse, G.GraphConv(F, F, aggr=aggr))):
            conv = conv.to(DEV)
            first, second = run(conv), run(conv)
            torch.cuda.synchronize()
            assert len(first) == len(second)
            for a, b in zip(first, second):
                assert torch.equal(a, b)


def test_cuda_graph_capture_mean_then_max():
    from gcm import nn as G
    torch.manual_seed(14)
    c1 = _lively(G.DenseGraphConv(8, 16, aggr="mean")).to(DEV)
    c2 = _lively(G.DenseGraphConv(16, 16, aggr="max")).to(DEV)
    params = list(c1.parameters()) + list(c2.parameters())
    x = torch.randn(4, 20, 8, device=DEV, requires_grad=True)
    adj = ((torch.rand(4, 20, 20, device=DEV) < 0.3).float() * torch.rand(4, 20, 20, device=DEV))
    adj.requires_grad_()
    gout = torch.randn(4, 20, 16, device=DEV)
    leaves = params + [x, adj]

    def step():
        out = c2(torch.relu(c1(x, adj)), adj)
        out.backward(gout)
        return out

    want = step().detach().clone()
    want_g = [p.grad.clone() for p in leaves]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for p in leaves:
                p.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    for p in leaves:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(static_out, want, rtol=0, atol=0)
    for a, b in zip([p.grad for p in leaves], want_g):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
def _dense_pair(kind, F, H):
    from gcm import nn as G
    ref_l = {"mean": lambda a, b: DenseGraphConvRef(a, b, "mean"), "sage": DenseSAGERef}[kind]
    dev_l = {"mean": lambda a, b: G.DenseGraphConv(a, b, aggr="mean"), "sage": G.DenseSAGEConv}[kind]
    ref = pyg.Sequential("x, adj, weights, B, N", [(ref_l(F, H), "x, adj -> x"), torch.nn.Tanh(),
                                                   (ref_l(H, H), "x, adj -> x"), torch.nn.Tanh()])
    _lively(ref)
    dev = G.Sequential("x, adj, weights, B, N", [(dev_l(F, H), "x, adj -> x"), torch.nn.Tanh(),
                                                 (dev_l(H, H), "x, adj -> x"), torch.nn.Tanh()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


@pytest.mark.parametrize("kind", ["mean", "sage"])
def test_dense_gcm_dense_edge(kind):
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.dense import DenseEdge
    torch.manual_seed(11)
    B, F, H, N, T = 4, 6, 16, 8, 12               # T > N: the overflow wrap
    ref, dev = _dense_pair(kind, F, H)
    obs = torch.randn(T, B, F)
    gw = torch.randn(T, B, H)

    mem = DenseGCM(dev, edge_selectors=DenseEdge(), graph_size=N)
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
        want, h = od.dense_rollout(obs.to(dt), None, r, graph_size=N, edge_selectors=od.DenseEdge())
        (want * gw.to(dt)).sum().backward()
        res[dt] = (want, h, {k: p.grad for k, p in r.named_parameters()})
    assert_bounded(got, res[torch.float64][0], res[torch.float32][0], "mx")
    assert_bounded(hidden[0], res[torch.float64][1][0], res[torch.float32][1][0], "nodes")
    assert torch.equal(hidden[1].cpu(), res[torch.float32][1][1])
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][k], res[torch.float32][2][k], k, floor=GRAD_FLOOR, relative=True)


def test_dense_gcm_learned_edge_mean_stack():
    """LearnedEdge hands the GNN an adjacency with a gradient: the edge network learns only through the mean
    layer's g_adj, degree term included.  Gumbel draws injected into both sides."""
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.learned import LearnedEdge
    torch.manual_seed(21)
    B, F, H, N, T, k = 4, 6, 16, 8, 12, 3          # T > N: the overflow wrap
    ref, dev = _dense_pair("mean", F, H)
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
        r, n_ = copy.deepcopy(ref).to(dt), copy.deepcopy(net).to(dt)
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
    assert net_scale > 0                                                        # g_adj reached the edge network
    for kk, p in sel.edge_network.named_parameters():
        g64, g32 = r64[2]["net." + kk], r32[2]["net." + kk]
        err = float((p.grad.cpu().double() - g64).abs().max())
        own = float((g32.double() - g64).abs().max())
        # (floor on the edge network's common scale, as tests/test_gcn_gpu.py: biases after the softmax get
        #  sum_j g_logit[j] = 0 analytically)
        assert err <= max(3.0 * own, 2e-6 * net_scale), (kk, err, own, net_scale)


def _sparse_pair(kind, F, H):
    from gcm import nn as G
    if kind == "sage":
        sig, ref_l, dev_l = "x, edges -> x", SAGERef, G.SAGEConv
    else:
        sig = "x, edges, weights -> x"
        ref_l, dev_l = (lambda a, b: GraphConvRef(a, b, "max")), (lambda a, b: G.GraphConv(a, b, aggr="max"))
    ref = pyg.Sequential("x, edges, weights", [(ref_l(F, H), sig), torch.nn.Tanh(), (ref_l(H, H), sig)])
    _lively(ref)
    dev = G.Sequential("x, edges, weights", [(dev_l(F, H), sig), torch.nn.Tanh(), (dev_l(H, H), sig)])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


@pytest.mark.parametrize("kind", ["max", "sage"])
@pytest.mark.parametrize("mode", ["one_shot", "stepwise", "two_hops"])
def test_sparse_gcm_temporal_edge(kind, mode):
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    torch.manual_seed(12)
    B, F, H, N = 3, 5, 16, 24
    ref, dev = _sparse_pair(kind, F, H)
    if mode == "one_shot":
        calls = [(torch.randn(B, 9, F), torch.tensor([9, 4, 7]))]
    elif mode == "stepwise":
        calls = [(torch.randn(B, 1, F), torch.tensor([1, 1, 1])) for _ in range(5)]
    else:
        calls = [(torch.randn(B, 6, F), torch.tensor([6, 4, 5])), (torch.randn(B, 6, F), torch.tensor([3, 6, 1]))]
    max_hops = 2 if mode == "two_hops" else None
    gws = [torch.randn(*x.shape[:2], H) for x, _ in calls]

    mem = SparseGCM(dev, edge_selectors=TemporalEdge([1, 2]), graph_size=N, max_hops=max_hops)
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
            mx, h = osp.sparse_step(x.to(dt), taus, h, r, graph_size=N, edge_selectors=osp.TemporalEdge([1, 2]),
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


def test_add_stack_keeps_its_fused_paths():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    dense = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(6, 16, aggr="add"), "x, adj -> x"), torch.nn.Tanh(),
                                                   (G.DenseGraphConv(16, 16, aggr="add"), "x, adj -> x"), torch.nn.Tanh()])
    assert DenseGCM(dense.to(DEV), edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is not None
    sig = "x, edges, weights -> x"
    sparse = G.Sequential("x, edges, weights", [(G.GraphConv(6, 16), sig), torch.nn.Tanh(), (G.GraphConv(16, 16), sig)])
    mem = SparseGCM(sparse.to(DEV), edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is not None and mem._native_gnn()
