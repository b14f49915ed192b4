"""DenseResGatedGraphConv / ResGatedGraphConv kernels against the eager restatement (tests/_resgated_restate.py),
evaluated in float64 for the bound and in float32 for the restatement's own error.  Needs an MI355X."""
import copy

import pytest
import torch

from _gcn_restate import assert_bounded
from _resgated_restate import DenseResGatedRef, ResGatedRef
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _lively(conv, scale=2.0):
    """Parameters away from their init: key and query weights scaled and a non-zero bias, so the gates spread over
    (0, 1) instead of sitting near 1/2."""
    with torch.no_grad():
        conv.lin_key.weight.mul_(scale)
        conv.lin_query.weight.mul_(scale)
        if conv.bias is not None:
            conv.bias.uniform_(-0.5, 0.5)
    return conv


def _check(dconv, out, x_grad, ref, run, x, g, adj=None, adj_grad=None):
    """`run(module, x[, adj])` on the restatement `ref` (the layer's parameters) in float64 and float32 bounds the
    layer's output and every gradient: x, all parameters and, when given, the adjacency."""
    res = {}
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(ref).to(dt)
        xr = x.detach().to(dt).requires_grad_()
        ar = None if adj_grad is None else adj.detach().to(dt).requires_grad_()
        o = run(r, xr) if ar is None else run(r, xr, ar)
        o.backward(g.to(dt))
        res[dt] = (o, xr.grad, {k: p.grad for k, p in r.named_parameters()}, None if ar is None else ar.grad)
    o64, x64, p64, a64 = res[torch.float64]
    o32, x32, p32, a32 = res[torch.float32]
    assert out.shape == o64.shape
    assert torch.isfinite(out).all() and torch.isfinite(x_grad).all()
    assert_bounded(out, o64, o32, "out")
    assert_bounded(x_grad.reshape(x64.shape), x64, x32, "x", floor=GRAD_FLOOR, relative=True)
    got = dict(dconv.named_parameters())
    assert set(got) == set(p64)
    for k in p64:
        assert got[k].grad is not None, k
        assert torch.isfinite(got[k].grad).all(), k
        assert_bounded(got[k].grad, p64[k], p32[k], k, floor=GRAD_FLOOR, relative=True)
    if adj_grad is not None:
        assert_bounded(adj_grad.reshape(a64.shape), a64, a32, "adj", floor=GRAD_FLOOR, relative=True)


def _ref_of(conv, cls, Fi, C, kw):
    ref = cls(Fi, C, **kw)
    ref.load_state_dict(conv.state_dict())
    return ref


# ---------------------------------------------------------------------------
# DenseResGatedGraphConv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,Fi,C,opts", [
    (3, 7, 3, 5, {}),                                       # below one tile, odd widths
    (5, 1, 4, 3, {}),                                       # a single node
    (2, 33, 8, 1, {}),                                      # one channel, image word boundary at 32
    (2, 65, 16, 33, {}),                                    # word boundary at 64, channels just past a half-wave
    (2, 130, 32, 32, {}),                                   # past a 128-row block
    (16, 128, 32, 32, {}),                                  # cfg2's per-graph shape
    (2, 40, 128, 128, {}),                                  # both width limits, two columns per lane
    (2, 40, 64, 65, {}),
    (2, 40, 16, 12, {"add_loop": True}),
    (2, 40, 16, 12, {"empty_rows": True}),
    (3, 33, 8, 8, {"mask": True}),
    (3, 33, 8, 8, {"root_weight": False}),
    (3, 33, 8, 8, {"bias": False}),
    (1, 20, 6, 9, {"two_d": True}),
    (4, 20, 6, 9, {"bcast": True}),
    (3, 50, 10, 7, {"weighted": True, "adj_grad": True}),
    (3, 50, 10, 7, {"weighted": True, "adj_grad": True, "add_loop": True}),
    (2, 20, 8, 8, {"saturated": True}),
])
def test_dense_resgatedconv(B, N, Fi, C, opts):
    from gcm import nn as G
    torch.manual_seed(B * 1000 + N + Fi + C)
    add_loop = opts.get("add_loop", False)
    kw = {"bias": opts.get("bias", True), "root_weight": opts.get("root_weight", True)}
    conv = _lively(G.DenseResGatedGraphConv(Fi, C, **kw), 300.0 if opts.get("saturated") else 2.0)
    x = torch.randn(B, N, Fi)
    nb = 1 if opts.get("bcast") else B
    adj = (torch.rand(nb, N, N) < 0.3).float()
    if opts.get("weighted"):
        adj = adj * (torch.rand(nb, N, N) * 4 - 2)          # weights in [-2, 2] at density 0.3
    if opts.get("empty_rows"):
        adj[:, : N // 4] = 0                                # rows without a neighbour
    mask = (torch.rand(B, N) < 0.7) if opts.get("mask") else None
    if opts.get("two_d"):
        x, adj = x[0], adj[0]
    g = torch.randn(B, N, C)

    dconv = copy.deepcopy(conv).to(DEV)
    xd, ad = x.to(DEV).requires_grad_(), adj.to(DEV)
    if opts.get("adj_grad"):
        ad.requires_grad_()
    out = dconv(xd, ad, None if mask is None else mask.to(DEV), add_loop=add_loop)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()

    ref = _ref_of(conv, DenseResGatedRef, Fi, C, kw)
    if opts.get("adj_grad"):
        assert torch.isfinite(ad.grad).all()
        if add_loop:
            assert float(ad.grad.diagonal(dim1=-2, dim2=-1).abs().max()) == 0.0
        _check(dconv, out, xd.grad, ref, lambda r, x_, a_: r(x_, a_, mask, add_loop), x, g, adj, ad.grad)
    else:
        assert ad.grad is None
        _check(dconv, out, xd.grad, ref, lambda r, x_: r(x_, adj.to(x_.dtype), mask, add_loop), x, g)
    if opts.get("empty_rows"):                              # a row without a neighbour: skip + bias
        want = {dt: torch.nn.functional.linear(x.to(dt), conv.lin_skip.weight.detach().to(dt),
                                               conv.bias.detach().to(dt))[:, : N // 4]
                for dt in (torch.float64, torch.float32)}
        assert_bounded(out[:, : N // 4], want[torch.float64], want[torch.float32], "empty rows")


def test_sigmoid_saturates_to_exact_zero_and_one():
    """Pre-activations of +-1000: the gates are exactly 1 and 0, their gradient exactly 0, nothing is NaN."""
    from gcm import nn as G
    conv = G.DenseResGatedGraphConv(1, 2, root_weight=False, bias=False).to(DEV)
    with torch.no_grad():
        conv.lin_key.weight.copy_(torch.tensor([[1000.0], [-1000.0]]))
        conv.lin_key.bias.zero_()
        conv.lin_query.weight.zero_()
        conv.lin_query.bias.zero_()
        conv.lin_value.weight.copy_(torch.tensor([[3.0], [3.0]]))
        conv.lin_value.bias.zero_()
    x = torch.ones(1, 2, 1, device=DEV, requires_grad=True)
    adj = torch.ones(1, 2, 2, device=DEV)
    out = conv(x, adj)
    out.sum().backward()
    assert torch.equal(out.detach().cpu(), torch.tensor([[[6.0, 0.0], [6.0, 0.0]]]))
    for p in (conv.lin_key.weight, conv.lin_key.bias, conv.lin_query.weight, conv.lin_query.bias):
        assert torch.equal(p.grad, torch.zeros_like(p))
    assert torch.isfinite(x.grad).all()
    s = G.ResGatedGraphConv(1, 2, root_weight=False, bias=False).to(DEV)
    s.load_state_dict(conv.state_dict())
    ei = torch.tensor([[0, 1, 0, 1], [0, 0, 1, 1]], device=DEV)
    xs = torch.ones(2, 1, device=DEV, requires_grad=True)
    out_s = s(xs, ei)
    out_s.sum().backward()
    assert torch.equal(out_s.detach().cpu(), torch.tensor([[6.0, 0.0], [6.0, 0.0]]))
    for p in (s.lin_key.weight, s.lin_key.bias, s.lin_query.weight, s.lin_query.bias):
        assert torch.equal(p.grad, torch.zeros_like(p))


def test_zero_entries_are_skipped():
    """An entry equal to 0 contributes nothing, whatever sits behind it: a non-finite v_j of a node nobody reads
    must not reach the other rows."""
    from gcm import nn as G
    torch.manual_seed(5)
    conv = _lively(G.DenseResGatedGraphConv(4, 8)).to(DEV)
    x = torch.randn(2, 12, 4, device=DEV)
    adj = (torch.rand(2, 12, 12, device=DEV) < 0.4).float()
    adj[:, :, 5] = 0                                        # nobody reads node 5
    want = conv(x, adj)
    x2 = x.clone()
    x2[:, 5] = float("inf")
    got = conv(x2, adj)
    keep = [i for i in range(12) if i != 5]
    assert torch.equal(got[:, keep], want[:, keep])


@pytest.mark.parametrize("cls", ["DenseResGatedGraphConv", "ResGatedGraphConv"])
def test_deterministic(cls):
    from gcm import nn as G
    torch.manual_seed(4)
    conv = _lively(getattr(G, cls)(32, 32)).to(DEV)
    if cls == "DenseResGatedGraphConv":
        x = torch.randn(16, 128, 32, device=DEV, requires_grad=True)
        other = ((torch.rand(16, 128, 128, device=DEV) < 0.2).float() * torch.rand(16, 128, 128, device=DEV))
        other.requires_grad_()
    else:
        x = torch.randn(300, 32, device=DEV, requires_grad=True)
        other = _edges(300, 1500, 9).to(DEV)
    g = torch.randn(*x.shape[:-1], 32, device=DEV)
    leaves = list(conv.parameters()) + [x] + ([other] if other.requires_grad else [])
    runs = []
    for _ in range(2):
        for p in leaves:
            p.grad = None
        out = conv(x, other)
        out.backward(g)
        runs.append([out.detach().clone()] + [p.grad.clone() for p in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_resgated_rejects_wide_layers():
    from gcm import nn as G
    with pytest.raises(RuntimeError, match="code -2"):
        G.DenseResGatedGraphConv(129, 8).to(DEV)(torch.randn(2, 5, 129, device=DEV), torch.ones(2, 5, 5, device=DEV))
    with pytest.raises(RuntimeError, match="code -2"):
        G.DenseResGatedGraphConv(8, 129).to(DEV)(torch.randn(2, 5, 8, device=DEV), torch.ones(2, 5, 5, device=DEV))
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        G.ResGatedGraphConv(129, 8).to(DEV)(torch.randn(3, 129, device=DEV), ei)
    with pytest.raises(RuntimeError, match="code -2"):
        G.ResGatedGraphConv(8, 129).to(DEV)(torch.randn(3, 8, device=DEV), ei)


# ---------------------------------------------------------------------------
# ResGatedGraphConv
# ---------------------------------------------------------------------------
def _edges(M, E, seed):
    """tests/test_gat_gpu.py's construction: duplicate loops, a duplicate edge, the last three nodes isolated."""
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, M - 3), (2, E), generator=gen)     # the last 3 nodes stay isolated
    if E:
        extra = torch.tensor([[0, 1, 0, 2, 1], [0, 2, 0, 2, 2]])     # duplicate loops (0, 0), duplicate edge 1 -> 2
        ei = torch.cat([ei[:, : E // 2], extra, ei[:, E // 2:]], 1)
    return ei


@pytest.mark.parametrize("M,E,Fi,C,opts", [
    (6, 0, 3, 5, {}),                                       # no edges
    (40, 90, 8, 1, {}),
    (40, 90, 8, 33, {}),
    (300, 1500, 32, 32, {}),
    (129, 700, 128, 128, {}),
    (50, 120, 8, 8, {"root_weight": False, "bias": False, "edge_attr": True}),
])
def test_resgatedconv(M, E, Fi, C, opts):
    from gcm import nn as G
    torch.manual_seed(M + E + Fi + C)
    kw = {"bias": opts.get("bias", True), "root_weight": opts.get("root_weight", True)}
    conv = _lively(G.ResGatedGraphConv(Fi, C, **kw))
    ei = _edges(M, E, seed=M + E)
    x = torch.randn(M, Fi)
    g = torch.randn(M, C)
    dconv = copy.deepcopy(conv).to(DEV)
    xd = x.to(DEV).requires_grad_()
    attr = torch.randn(ei.shape[1], 3, device=DEV) if opts.get("edge_attr") else None
    out = dconv(xd, ei.to(DEV), attr)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    _check(dconv, out, xd.grad, _ref_of(conv, ResGatedRef, Fi, C, kw), lambda r, x_: r(x_, ei), x, g)


def test_masked_graph_index_raises():
    from gcm import nn as G, _ops
    M = 5
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]], device=DEV)
    ei.gcm_graph = _ops.GraphIndex(ei, _ops.ptr_from_sorted(ei[1], M), M, mask=torch.ones(M, dtype=torch.bool,
                                                                                          device=DEV))
    with pytest.raises(ValueError, match="masked GraphIndex"):
        G.ResGatedGraphConv(4, 4).to(DEV)(torch.randn(M, 4, device=DEV), ei)


def test_dense_equals_sparse():
    """Both layers on one 0/1 pattern, each held to the same float64 restatement by the bound."""
    from gcm import nn as G
    torch.manual_seed(7)
    B, N, Fi, C = 3, 20, 8, 6
    adj = (torch.rand(B, N, N) < 0.25).float()
    adj[:, 3] = 0                                           # a node without in-edges
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])            # adj[b, i, j]: edge j -> i
    conv = _lively(G.DenseResGatedGraphConv(Fi, C))
    dconv = copy.deepcopy(conv).to(DEV)
    sconv = G.ResGatedGraphConv(Fi, C).to(DEV)
    sconv.load_state_dict(dconv.state_dict())
    x = torch.randn(B, N, Fi)
    g = torch.randn(B, N, C)
    xa, xb = x.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
    out_d = dconv(xa, adj.to(DEV))
    out_s = sconv(xb.view(B * N, Fi), ei.to(DEV)).view(B, N, C)
    out_d.backward(g.to(DEV))
    out_s.backward(g.to(DEV))
    torch.cuda.synchronize()
    ref = _ref_of(conv, DenseResGatedRef, Fi, C, {})
    run = lambda r, x_: r(x_, adj.to(x_.dtype))             # noqa: E731
    _check(dconv, out_d, xa.grad, ref, run, x, g)
    _check(sconv, out_s, xb.grad, ref, run, x, g)


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
def _lively_ref(ref):
    for m in ref.modules():
        if isinstance(m, (DenseResGatedRef, ResGatedRef)):
            _lively(m)
    return ref


def _dense_pair(F, H):
    from gcm import nn as G
    ref = _lively_ref(pyg.Sequential("x, adj, weights, B, N", [
        (DenseResGatedRef(F, H), "x, adj -> x"), torch.nn.ReLU(),
        (DenseResGatedRef(H, H), "x, adj -> x"), torch.nn.ReLU()]))
    dev = G.Sequential("x, adj, weights, B, N", [
        (G.DenseResGatedGraphConv(F, H), "x, adj -> x"), torch.nn.ReLU(),
        (G.DenseResGatedGraphConv(H, H), "x, adj -> x"), torch.nn.ReLU()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _sparse_pair(F, H):
    from gcm import nn as G
    ref = _lively_ref(pyg.Sequential("x, edges, weights", [
        (ResGatedRef(F, H), "x, edges, weights -> x"), torch.nn.Tanh(),
        (ResGatedRef(H, H), "x, edges, weights -> x")]))
    dev = G.Sequential("x, edges, weights", [
        (G.ResGatedGraphConv(F, H), "x, edges, weights -> x"), torch.nn.Tanh(),
        (G.ResGatedGraphConv(H, H), "x, edges, weights -> x")])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


@pytest.mark.parametrize("selector", ["backedge", "dense"])
def test_dense_gcm_with_resgated_stack(selector):
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.dense import DenseEdge
    from gcm.edge_selectors.temporal import TemporalBackedge
    torch.manual_seed(11)
    B, F, H, N, T = 4, 6, 16, 8, 12               # T > N: the overflow wrap; step 0 is a row with no neighbour
    ref, dev = _dense_pair(F, H)
    obs = torch.randn(T, B, F)
    gw = torch.randn(T, B, H)
    sel, osel = (TemporalBackedge([1, 2]), od.TemporalBackedge([1, 2])) if selector == "backedge" else \
        (DenseEdge(), od.DenseEdge())

    mem = DenseGCM(dev, edge_selectors=sel, graph_size=N)
    assert mem._structure() is None                # the layered path
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
        want, h = od.dense_rollout(obs.to(dt), None, r, graph_size=N, edge_selectors=osel)
        (want * gw.to(dt)).sum().backward()
        res[dt] = (want, h, {k: p.grad for k, p in r.named_parameters()})
    assert_bounded(got, res[torch.float64][0], res[torch.float32][0], "mx")
    assert_bounded(hidden[0], res[torch.float64][1][0], res[torch.float32][1][0], "nodes")
    assert torch.equal(hidden[1].cpu(), res[torch.float32][1][1])
    assert torch.equal(hidden[3].cpu(), res[torch.float32][1][3])          # num_nodes
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][k], res[torch.float32][2][k], k, floor=GRAD_FLOOR, relative=True)


@pytest.mark.parametrize("max_hops", [None, 2])
def test_sparse_gcm_with_resgated_stack(max_hops):
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    torch.manual_seed(12)
    B, F, H, N = 3, 5, 16, 24
    ref, dev = _sparse_pair(F, H)
    calls = [(torch.randn(B, 6, F), torch.tensor([6, 4, 5])), (torch.randn(B, 6, F), torch.tensor([3, 6, 1]))]
    gws = [torch.randn(B, 6, H) for _ in calls]

    mem = SparseGCM(dev, edge_selectors=TemporalEdge([1]), graph_size=N, max_hops=max_hops)
    assert mem._canonical() is None and not mem._native_gnn()       # the generic path
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
    assert torch.equal(hidden[2].cpu(), res[torch.float32][1][2])           # num_nodes
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][k], res[torch.float32][2][k], k, floor=GRAD_FLOOR, relative=True)


@pytest.mark.parametrize("memory", ["dense", "sparse"])
def test_training_loss_falls(memory):
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    torch.manual_seed(13)
    F, H, B = 4, 16, 8
    net = (_dense_pair if memory == "dense" else _sparse_pair)(F, H)[1]
    obs = torch.randn(6, B, F, device=DEV)
    target = torch.randn(6, B, H, device=DEV)

    def dense_loss():
        m, hidden, outs = DenseGCM(net, edge_selectors=TemporalBackedge([1]), graph_size=8), None, []
        for t in range(obs.shape[0]):
            mx, hidden = m(obs[t], hidden)
            outs.append(mx)
        return ((torch.stack(outs) - target) ** 2).mean()

    def sparse_loss():
        m = SparseGCM(net, edge_selectors=TemporalEdge([1]), graph_size=8)
        mx, _ = m(obs.transpose(0, 1), torch.full((B,), obs.shape[0], device=DEV), None)
        return ((mx - target.transpose(0, 1)) ** 2).mean()

    loss_fn = dense_loss if memory == "dense" else sparse_loss
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
    c1 = _lively(G.DenseResGatedGraphConv(8, 16)).to(DEV)
    c2 = _lively(G.DenseResGatedGraphConv(16, 16, root_weight=False)).to(DEV)
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
