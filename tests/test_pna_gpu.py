"""DensePNAConv / PNAConv kernels against the eager restatement (tests/_pna_restate.py), evaluated in float64 for the
bound and in float32 for the restatement's own error, on the case table there (whose input-family conditions
tests/test_pna_cpu.py asserts).  Needs an MI355X."""
import copy

import pytest
import torch

import _pna_restate as R
from _gcn_restate import assert_bounded, bound
from _pna_restate import DensePNARef, PNARef
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _layer(ref, name):
    """The gcm.nn layer `name` with the parameters and buffers of the restatement module `ref`, on the device."""
    from gcm import nn as G
    conv = getattr(G, name)(deg=[1], **ref.kwargs())
    conv.load_state_dict(ref.state_dict())
    return conv.to(DEV)


def _held(got, res, show=""):
    """Every tensor of `got` (name -> device tensor) within assert_bounded of the references `res`."""
    f64, f32 = res[torch.float64], res[torch.float32]
    assert set(got) == set(f64), (sorted(got), sorted(f64))
    for k, v in got.items():
        assert v is not None, k
        assert torch.isfinite(v).all(), k
        v = v.reshape(f64[k].shape)
        err = float((v.detach().cpu().double() - f64[k]).abs().max()) if v.numel() else 0.0
        if k == "out":
            print(show, k, f"err {err:.2e} bound {bound(f64[k], f32[k]):.2e}")
            assert_bounded(v, f64[k], f32[k], k)
        else:
            print(show, k, f"err {err:.2e} bound {bound(f64[k], f32[k], GRAD_FLOOR, True):.2e}")
            assert_bounded(v, f64[k], f32[k], k, floor=GRAD_FLOOR, relative=True)


def _grads(conv):
    return {k: p.grad for k, p in conv.named_parameters()}


# ---------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(R.DENSE_CASES)), ids=[R.case_id(c) for c in R.DENSE_CASES])
def test_dense_pnaconv(index):
    inp, res = R.dense_reference(index)
    conv = _layer(inp["ref"], "DensePNAConv")
    x = inp["x"].to(DEV).requires_grad_()
    adj = inp["adj"].to(DEV).requires_grad_()
    mask = None if inp["mask"] is None else inp["mask"].to(DEV)
    out = conv(x, adj, mask, add_loop=inp["add_loop"])
    assert out.shape == res[torch.float64]["out"].shape
    out.backward(inp["g"].to(DEV).view_as(out))
    torch.cuda.synchronize()
    assert adj.grad is None                                         # only the pattern is read
    _held({"out": out, "x": x.grad, **_grads(conv)}, res, R.case_id(R.DENSE_CASES[index]))


@pytest.mark.parametrize("index", range(len(R.SPARSE_CASES)), ids=[R.case_id(c) for c in R.SPARSE_CASES])
@pytest.mark.parametrize("attached", [False, True], ids=["bare", "attached"])
def test_pnaconv(index, attached):
    """attached: with the index SparseGCM attaches (`edge_index.gcm_graph`); else the plain list, indexed in the layer."""
    from gcm import _ops
    inp, res = R.sparse_reference(index)
    conv = _layer(inp["ref"], "PNAConv")
    x = inp["x"].to(DEV).requires_grad_()
    ei = inp["edge_index"].to(DEV)
    if attached:
        ei.gcm_graph = _ops.GraphIndex.from_edge_index(ei, x.shape[0])
    out = conv(x, ei)
    out.backward(inp["g"].to(DEV))
    torch.cuda.synchronize()
    _held({"out": out, "x": x.grad, **_grads(conv)}, res, R.case_id(R.SPARSE_CASES[index]))


def test_degree_histogram_from_device_tensors():
    """The histogram of a rollout's adjacency, taken on the device, is accepted as `deg`."""
    from gcm import nn as G
    adj = torch.ones(6, 6, device=DEV).tril(-1)
    deg = G.degree_histogram(adj)
    assert deg.tolist() == [1, 1, 1, 1, 1, 1]
    conv = G.DensePNAConv(4, 4, ["mean"], ["linear"], deg).to(DEV)
    assert abs(float(conv.aggr_module.avg_deg_lin) - 2.5) < 1e-6
    assert G.degree_histogram(torch.tensor([[0, 1], [1, 1]], device=DEV), 3).tolist() == [2, 0, 1]


def test_width_limits():
    from gcm import nn as G
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    for cin, cout in ((129, 8), (8, 129)):
        with pytest.raises(RuntimeError, match="code -2"):
            G.DensePNAConv(cin, cout, ["mean"], ["identity"], [1, 1]).to(DEV)(torch.randn(2, 5, cin, device=DEV),
                                                                               torch.ones(2, 5, 5, device=DEV))
        with pytest.raises(RuntimeError, match="code -2"):
            G.PNAConv(cin, cout, ["mean"], ["identity"], [1, 1]).to(DEV)(torch.randn(3, cin, device=DEV), ei)


def test_masked_graph_index_raises():
    from gcm import nn as G, _ops
    M = 5
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]], device=DEV)
    ei.gcm_graph = _ops.GraphIndex(ei, _ops.ptr_from_sorted(ei[1], M), M, mask=torch.ones(M, dtype=torch.bool,
                                                                                          device=DEV))
    with pytest.raises(ValueError, match="masked GraphIndex"):
        G.PNAConv(4, 4, ["mean"], ["identity"], [1, 1]).to(DEV)(torch.randn(M, 4, device=DEV), ei)


# ---------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------
def _identity_tail(ref):
    """Identity post and final linears: the output is x + the aggregate, and x.grad shows where a tie's gradient went."""
    with torch.no_grad():
        for seq in ref.post_nns:
            seq[0].weight.copy_(torch.cat([torch.eye(ref.F_out)] * 2, 1))
            seq[0].bias.zero_()
        ref.lin.weight.copy_(torch.eye(ref.out_channels))
        ref.lin.bias.zero_()
    return ref


@pytest.mark.parametrize("aggregator", ["min", "max"])
def test_ties_dense(aggregator):
    """Dyadic inputs with few distinct values: ties everywhere.  x.grad equals the restatement's exactly, so every
    tie's gradient landed on the lowest j."""
    B, N, Fc = 2, 40, 6
    ref = _identity_tail(R.lively(DensePNARef(Fc, Fc, [aggregator], ["identity"], [1, 1]), 41, True))
    x = R.features((B, N, Fc), 42, True).clamp(-1, 1)
    adj = R.pattern("random", B, N, 43)
    g = torch.randint(-2, 3, (B, N, Fc)).float()
    xr = x.clone().requires_grad_()
    ref(xr, adj).backward(g)
    conv = _layer(ref, "DensePNAConv")
    xd = x.to(DEV).requires_grad_()
    out = conv(xd, adj.to(DEV))
    out.backward(g.to(DEV))
    torch.testing.assert_close(out.cpu(), ref(x, adj).detach(), rtol=0, atol=0)
    torch.testing.assert_close(xd.grad.cpu(), xr.grad, rtol=0, atol=0)
    pre = ref.pre_nns[0][0]
    msg = R.dense_messages(x, pre.weight, pre.bias).reshape(B * N, N, Fc).detach()
    assert int((R.min_max_margin(msg, (adj != 0).reshape(B * N, N)) == 0).sum()) > 20      # there were ties


@pytest.mark.parametrize("aggregator", ["min", "max"])
def test_ties_sparse(aggregator):
    """The same over an edge list with duplicates: the first edge in CSR order takes the gradient."""
    M, Fc = 40, 6
    ref = _identity_tail(R.lively(PNARef(Fc, Fc, [aggregator], ["identity"], [1, 1]), 44, True))
    x = R.features((M, Fc), 45, True).clamp(-1, 1)
    ei = R.random_edges(M, 300, 46)
    g = torch.randint(-2, 3, (M, Fc)).float()
    xr = x.clone().requires_grad_()
    ref(xr, ei).backward(g)
    conv = _layer(ref, "PNAConv")
    xd = x.to(DEV).requires_grad_()
    out = conv(xd, ei.to(DEV))
    out.backward(g.to(DEV))
    torch.testing.assert_close(out.cpu(), ref(x, ei).detach(), rtol=0, atol=0)
    torch.testing.assert_close(xd.grad.cpu(), xr.grad, rtol=0, atol=0)


# ---------------------------------------------------------------------------
# dense against sparse
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("lists", [R.ALL, R.NOVAR], ids=["all-dyadic", "novar-generic"])
def test_dense_equals_sparse(lists):
    """The dense twin and the sparse layer on one graph with the same parameters: within rtol = atol = 1e-5, the bound
    tests/test_aggr_gpu.py uses for this comparison."""
    B, N, cin, cout, T = 3, 20, 6, 8, 2
    dyadic = R.is_dyadic(lists[0])
    adj = R.pattern("random", B, N, 51)
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])                    # adj[b, i, j]: edge j -> i
    deg = R.histogram((adj != 0).sum(-1))
    ref = R.lively(DensePNARef(cin, cout, lists[0], lists[1], deg, T), 52, dyadic)
    x = R.features((B, N, cin), 53, dyadic)
    assert R.family_violations(ref, x, adj) == 0
    g = torch.randn(B, N, cout)
    dconv, sconv = _layer(ref, "DensePNAConv"), _layer(ref, "PNAConv")
    xa, xb = x.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
    out_d = dconv(xa, adj.to(DEV))
    out_s = sconv(xb.view(B * N, cin), ei.to(DEV)).view(B, N, cout)
    out_d.backward(g.to(DEV))
    out_s.backward(g.to(DEV))
    torch.testing.assert_close(out_d, out_s, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-5, atol=1e-5)
    for (k, p), q in zip(dconv.named_parameters(), sconv.parameters()):
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-5, atol=1e-5, msg=k)


# ---------------------------------------------------------------------------
# reproducibility
# ---------------------------------------------------------------------------
def _twice(conv, args, leaves, g):
    runs = []
    for _ in range(2):
        for p in leaves:
            p.grad = None
        out = conv(*args)
        out.backward(g)
        runs.append([out.detach().clone()] + [p.grad.clone() for p in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _random_layer(name, cin, cout, seed, lists=R.ALL, **kw):
    from gcm import nn as G
    torch.manual_seed(seed)
    return getattr(G, name)(cin, cout, lists[0], lists[1], [1, 3, 4, 2, 1], **kw).to(DEV)


def test_deterministic_dense():
    conv = _random_layer("DensePNAConv", 32, 32, 4, towers=2)
    x = torch.randn(4, 130, 32, device=DEV, requires_grad=True)
    adj = (torch.rand(4, 130, 130, device=DEV) < 0.2).float()
    _twice(conv, (x, adj), list(conv.parameters()) + [x], torch.randn(4, 130, 32, device=DEV))


def test_deterministic_sparse():
    conv = _random_layer("PNAConv", 32, 32, 5, towers=2, divide_input=True)
    x = torch.randn(300, 32, device=DEV, requires_grad=True)
    ei = R.random_edges(300, 1500, 9).to(DEV)
    _twice(conv, (x, ei), list(conv.parameters()) + [x], torch.randn(300, 32, device=DEV))


def test_cuda_graph_capture_two_layers():
    c1 = _random_layer("DensePNAConv", 8, 16, 14)
    c2 = _random_layer("DensePNAConv", 16, 16, 15, lists=R.PAPER, towers=2)
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


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
_DEG = [1, 3, 3, 2, 1]
_FIRST = (("mean", "min", "max", "std"), ("identity", "amplification", "attenuation"))
_SECOND = (("sum", "mean", "min", "max"), ("identity", "attenuation", "inverse_linear"))


def _dense_pair(F, H):
    """Layer 1 lists std and gets dyadic pre linears (the observations are dyadic); layer 2 has no var / std: its
    inputs are no longer dyadic."""
    from gcm import nn as G
    first = R.lively(DensePNARef(F, H, *_FIRST, _DEG), 61, True)
    second = R.lively(DensePNARef(H, H, *_SECOND, _DEG, towers=2), 62, False)
    ref = pyg.Sequential("x, adj, weights, B, N", [(first, "x, adj -> x"), torch.nn.Tanh(), (second, "x, adj -> x")])
    dev = G.Sequential("x, adj, weights, B, N", [
        (G.DensePNAConv(F, H, *_FIRST, _DEG), "x, adj -> x"), torch.nn.Tanh(),
        (G.DensePNAConv(H, H, *_SECOND, _DEG, towers=2), "x, adj -> x")])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _sparse_pair(F, H):
    from gcm import nn as G
    first = R.lively(PNARef(F, H, *_FIRST, _DEG), 63, True)
    second = R.lively(PNARef(H, H, *_SECOND, _DEG, towers=2), 64, False)
    ref = pyg.Sequential("x, edges, weights", [(first, "x, edges, weights -> x"), torch.nn.Tanh(),
                                               (second, "x, edges, weights -> x")])
    dev = G.Sequential("x, edges, weights", [
        (G.PNAConv(F, H, *_FIRST, _DEG), "x, edges, weights -> x"), torch.nn.Tanh(),
        (G.PNAConv(H, H, *_SECOND, _DEG, towers=2), "x, edges, weights -> x")])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


@pytest.mark.parametrize("selector", ["backedge", "dense"])
def test_dense_gcm_with_pna_stack(selector):
    """The gradient of module_0.lin.weight, accumulated over the 10 steps, is the sensitive figure here: it is g^T h
    with h the saved output of the post linear, so it carries the forward's error (Precision)."""
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.edge_selectors.dense import DenseEdge
    B, F, N, T = 3, 4, 8, 10                       # T > N: the overflow wrap
    H = F
    ref, dev = _dense_pair(F, H)
    obs = R.features((T, B, F), 65, True)
    gw = torch.randn(T, B, H, generator=torch.Generator().manual_seed(66))
    sel, osel = (TemporalBackedge([1, 2, 4]), od.TemporalBackedge([1, 2, 4])) if selector == "backedge" else \
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
    assert torch.equal(hidden[3].cpu(), res[torch.float32][1][3])          # num_nodes
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][k], res[torch.float32][2][k], k, floor=GRAD_FLOOR, relative=True)

    with torch.no_grad():                          # rollout() is the per-step loop
        rolled, hid2 = mem.rollout(obs.to(DEV))
    assert torch.equal(rolled, got.detach()) and torch.equal(hid2[0], hidden[0].detach())


@pytest.mark.parametrize("stepwise", [False, True], ids=["oneshot", "stepwise"])
def test_sparse_gcm_with_pna_stack(stepwise):
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    B, F, N, L = 3, 4, 8, 6
    H = F
    ref, dev = _sparse_pair(F, H)
    xs = R.features((B, L, F), 67, True)
    if stepwise:                                   # tau = 1: one node per call
        calls = [(xs[:, t:t + 1], torch.ones(B, dtype=torch.long)) for t in range(L)]
    else:
        calls = [(xs, torch.tensor([6, 4, 5]))]
    gen = torch.Generator().manual_seed(68)
    gws = [torch.randn(B, x.shape[1], H, generator=gen) for x, _ in calls]

    mem = SparseGCM(dev, edge_selectors=TemporalEdge([1, 2]), graph_size=N)
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
            mx, h = osp.sparse_step(x.to(dt), taus, h, r, graph_size=N, edge_selectors=osp.TemporalEdge([1, 2]))
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
