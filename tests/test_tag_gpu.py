"""DenseTAGConv / TAGConv kernels against the eager restatement (tests/_tag_restate.py), evaluated in float64 for the
bound and in float32 for the restatement's own error, on the cases of tests/_tag_cases.py.  Needs an MI355X."""
import copy

import pytest
import torch

import _tag_cases as cases
from _gcn_restate import assert_bounded, bound
from _tag_restate import DenseTagRef, TagRef, lively
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _layer(ref, name):
    """The gcm.nn layer `name` with the parameters of the restatement module `ref`, on the device."""
    from gcm import nn as G
    lin = ref.lins[0]
    conv = getattr(G, name)(lin.in_features, lin.out_features, ref.K, bias=ref.bias is not None,
                            normalize=ref.normalize)
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
# DenseTAGConv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cases.DENSE_CASES)), ids=[cases.case_id(c) for c in cases.DENSE_CASES])
def test_dense_tagconv(index):
    inp, res = cases.dense_reference(index)
    conv = _layer(inp["ref"], "DenseTAGConv")
    x = inp["x"].to(DEV).requires_grad_()
    adj = inp["adj"].to(DEV).requires_grad_(inp["adj_grad"])
    mask = None if inp["mask"] is None else inp["mask"].to(DEV)
    out = conv(x, adj, mask, add_loop=inp["add_loop"])
    assert out.shape == res[torch.float64]["out"].shape
    out.backward(inp["g"].to(DEV).view_as(out))
    torch.cuda.synchronize()
    got = {"out": out, "x": x.grad, **_grads(conv)}
    if inp["adj_grad"]:
        got["adj"] = adj.grad
        if conv.K > 0:
            assert float(adj.grad[adj == 0].abs().max()) > 0        # the derivative exists where adj is 0 too
    else:
        assert adj.grad is None
    _held(got, res, cases.case_id(cases.DENSE_CASES[index]))


def test_dense_adjacency_gradient_diagonal_and_empty_rows():
    """add_loop: the overwritten diagonal gets 0.  normalize: every entry of a row with deg == 0 gets exactly 0."""
    from gcm import nn as G
    torch.manual_seed(21)
    conv = G.DenseTAGConv(4, 6, 2).to(DEV)
    x = torch.randn(2, 9, 4, device=DEV)
    adj = (torch.rand(2, 9, 9, device=DEV) < 0.4).float() * torch.rand(2, 9, 9, device=DEV)
    adj[:, 3] = 0
    a1 = adj.clone().requires_grad_()
    conv(x, a1, add_loop=True).square().sum().backward()
    assert float(a1.grad.diagonal(dim1=-2, dim2=-1).abs().max()) == 0.0
    assert float(a1.grad.abs().max()) > 0
    a2 = adj.clone().requires_grad_()
    conv(x, a2).square().sum().backward()
    assert torch.isfinite(a2.grad).all()
    assert float(a2.grad[:, 3].abs().max()) == 0.0
    assert float(a2.grad[:, 4].abs().max()) > 0


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


@pytest.mark.parametrize("N", [128, 130])
def test_deterministic(N):
    """Forward + backward twice, on the one-workgroup path and on the per-hop path: outputs and every gradient bitwise
    equal."""
    from gcm import nn as G
    torch.manual_seed(4)
    conv = lively(G.DenseTAGConv(32, 32, 3)).to(DEV)
    x = torch.randn(8, N, 32, device=DEV, requires_grad=True)
    adj = ((torch.rand(8, N, N, device=DEV) < 0.2).float() * torch.rand(8, N, N, device=DEV))
    adj.requires_grad_()
    _twice(conv, (x, adj), list(conv.parameters()) + [x, adj], torch.randn(8, N, 32, device=DEV))


def test_deterministic_sparse():
    from gcm import nn as G
    torch.manual_seed(4)
    conv = lively(G.TAGConv(32, 32, 3)).to(DEV)
    x = torch.randn(300, 32, device=DEV, requires_grad=True)
    ei = cases.edges(300, 1500, 9).to(DEV)
    ew = torch.rand(ei.shape[1], device=DEV, requires_grad=True)
    _twice(conv, (x, ei, ew), list(conv.parameters()) + [x, ew], torch.randn(300, 32, device=DEV))


def test_width_limits():
    from gcm import nn as G
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    for cin, cout in ((129, 8), (8, 129)):
        with pytest.raises(RuntimeError, match="code -2"):
            G.DenseTAGConv(cin, cout, 1).to(DEV)(torch.randn(2, 5, cin, device=DEV), torch.ones(2, 5, 5, device=DEV))
        with pytest.raises(RuntimeError, match="code -2"):
            G.TAGConv(cin, cout, 1).to(DEV)(torch.randn(3, cin, device=DEV), ei)


# ---------------------------------------------------------------------------
# TAGConv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cases.SPARSE_CASES)), ids=[cases.case_id(c) for c in cases.SPARSE_CASES])
def test_tagconv(index):
    inp, res = cases.sparse_reference(index)
    conv = _layer(inp["ref"], "TAGConv")
    x = inp["x"].to(DEV).requires_grad_()
    ew = None if inp["edge_weight"] is None else inp["edge_weight"].to(DEV).requires_grad_()
    out = conv(x, inp["edge_index"].to(DEV), ew)
    out.backward(inp["g"].to(DEV))
    torch.cuda.synchronize()
    got = {"out": out, "x": x.grad, **_grads(conv)}
    if ew is not None:
        got["edge_weight"] = ew.grad
    _held(got, res, cases.case_id(cases.SPARSE_CASES[index]))


def test_attached_graph_index_equals_a_bare_edge_list():
    """The index SparseGCM attaches (`edge_index.gcm_graph`) is used when it matches: the same results, bitwise, as the
    bare list indexed inside the layer."""
    from gcm import _ops
    inp, _ = cases.sparse_reference(1)
    conv = _layer(inp["ref"], "TAGConv")
    x, g = inp["x"].to(DEV), inp["g"].to(DEV)
    bare = inp["edge_index"].to(DEV)
    attached = bare.clone()
    attached.gcm_graph = _ops.GraphIndex.from_edge_index(attached, x.shape[0])
    runs = []
    for ei in (bare, attached):
        conv.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_()
        ew = inp["edge_weight"].to(DEV).requires_grad_()
        out = conv(xd, ei, ew)
        out.backward(g)
        runs.append([out.detach().clone(), xd.grad.clone(), ew.grad.clone()] + [p.grad.clone() for p in conv.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_wrong_length_edge_weight_is_ignored():
    """A weight vector of the wrong length: the unweighted call, bitwise, and no gradient for the vector."""
    inp, _ = cases.sparse_reference(1)
    conv = _layer(inp["ref"], "TAGConv")
    x, ei = inp["x"].to(DEV), inp["edge_index"].to(DEV)
    g = inp["g"].to(DEV)
    runs = []
    for ew in (None, torch.rand(ei.shape[1] + 1, device=DEV, requires_grad=True)):
        conv.zero_grad(set_to_none=True)
        xd = x.clone().requires_grad_()
        out = conv(xd, ei, ew)
        out.backward(g)
        assert ew is None or ew.grad is None
        runs.append([out.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in conv.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_masked_graph_index_raises():
    from gcm import nn as G, _ops
    M = 5
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]], device=DEV)
    ei.gcm_graph = _ops.GraphIndex(ei, _ops.ptr_from_sorted(ei[1], M), M, mask=torch.ones(M, dtype=torch.bool,
                                                                                          device=DEV))
    with pytest.raises(ValueError, match="masked GraphIndex"):
        G.TAGConv(4, 4, 1).to(DEV)(torch.randn(M, 4, device=DEV), ei)


@pytest.mark.parametrize("normalize", [True, False])
def test_dense_equals_sparse(normalize):
    """Both layers on one weighted edge set: each within its own bound of the float64 restatement, and the two
    within the sum of the two bounds of each other."""
    torch.manual_seed(7)
    B, N, Fi, Fo, K = 3, 20, 4, 6, 3
    adj = (torch.rand(B, N, N) < 0.25).float() * (torch.rand(B, N, N) * 1.5 + 0.1)
    adj[:, 3] = 0                                               # a node without in-edges
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])                # adj[b, i, j]: edge j -> i
    ew = adj[bb, ii, jj]
    ref = lively(DenseTagRef(Fi, Fo, K, normalize=normalize))
    x, g = torch.randn(B, N, Fi), torch.randn(B, N, Fo)
    inp = {"ref": ref, "x": x, "adj": adj, "mask": None, "g": g, "add_loop": False, "adj_grad": True}
    res = cases._evaluate(inp, True)
    dconv, sconv = _layer(ref, "DenseTAGConv"), _layer(ref, "TAGConv")
    xa, xb = x.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
    adj_d, ew_d = adj.to(DEV).requires_grad_(), ew.to(DEV).requires_grad_()
    out_d = dconv(xa, adj_d)
    out_s = sconv(xb.view(B * N, Fi), ei.to(DEV), ew_d).view(B, N, Fo)
    out_d.backward(g.to(DEV))
    out_s.backward(g.to(DEV))
    torch.cuda.synchronize()
    got_d = {"out": out_d, "x": xa.grad, "adj": adj_d.grad, **_grads(dconv)}
    got_s = {"out": out_s, "x": xb.grad, **_grads(sconv)}
    _held(got_d, res, "dense")
    f64, f32 = res[torch.float64], res[torch.float32]
    res_s = {dt: {k: v for k, v in r.items() if k != "adj"} for dt, r in res.items()}
    _held(got_s, res_s, "sparse")
    for k in got_s:
        each = bound(f64[k], f32[k]) if k == "out" else bound(f64[k], f32[k], GRAD_FLOOR, True)
        diff = float((got_d[k].double() - got_s[k].reshape(got_d[k].shape).double()).abs().max())
        assert diff <= 2 * each, (k, diff, each)
    # the gradient of an edge's weight is the gradient of its entry of adj
    bd, id_, jd = bb.to(DEV), ii.to(DEV), jj.to(DEV)
    want64, want32 = f64["adj"][bb, ii, jj], f32["adj"][bb, ii, jj]
    assert_bounded(ew_d.grad, want64, want32, "edge_weight", floor=GRAD_FLOOR, relative=True)
    assert_bounded(adj_d.grad[bd, id_, jd], want64, want32, "adj at the edges", floor=GRAD_FLOOR, relative=True)


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
def _lively_ref(ref):
    for m in ref.modules():
        if isinstance(m, (DenseTagRef, TagRef)):
            lively(m)
    return ref


def _dense_pair(F, H):
    from gcm import nn as G
    ref = _lively_ref(pyg.Sequential("x, adj, weights, B, N", [
        (DenseTagRef(F, H, 2), "x, adj -> x"), torch.nn.Tanh(), (DenseTagRef(H, H, 1, normalize=False), "x, adj -> x")]))
    dev = G.Sequential("x, adj, weights, B, N", [
        (G.DenseTAGConv(F, H, 2), "x, adj -> x"), torch.nn.Tanh(),
        (G.DenseTAGConv(H, H, 1, normalize=False), "x, adj -> x")])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _sparse_pair(F, H):
    from gcm import nn as G
    ref = _lively_ref(pyg.Sequential("x, edges, weights", [
        (TagRef(F, H, 2), "x, edges, weights -> x"), torch.nn.Tanh(),
        (TagRef(H, H, 1, normalize=False), "x, edges, weights -> x")]))
    dev = G.Sequential("x, edges, weights", [
        (G.TAGConv(F, H, 2), "x, edges, weights -> x"), torch.nn.Tanh(),
        (G.TAGConv(H, H, 1, normalize=False), "x, edges, weights -> x")])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def test_dense_gcm_with_tag_stack():
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    torch.manual_seed(11)
    B, F, H, N, T = 4, 6, 16, 8, 12               # T > N: the overflow wrap
    ref, dev = _dense_pair(F, H)
    obs = torch.randn(T, B, F)
    gw = torch.randn(T, B, H)

    mem = DenseGCM(dev, edge_selectors=TemporalBackedge([1, 2]), graph_size=N)
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
        want, h = od.dense_rollout(obs.to(dt), None, r, graph_size=N, edge_selectors=od.TemporalBackedge([1, 2]))
        (want * gw.to(dt)).sum().backward()
        res[dt] = (want, h, {k: p.grad for k, p in r.named_parameters()})
    assert_bounded(got, res[torch.float64][0], res[torch.float32][0], "mx")
    assert_bounded(hidden[0], res[torch.float64][1][0], res[torch.float32][1][0], "nodes")
    assert torch.equal(hidden[1].cpu(), res[torch.float32][1][1])
    assert torch.equal(hidden[3].cpu(), res[torch.float32][1][3])          # num_nodes
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][k], res[torch.float32][2][k], k, floor=GRAD_FLOOR, relative=True)


@pytest.mark.parametrize("max_hops", [None, 2])
def test_sparse_gcm_with_tag_stack(max_hops):
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
    target = torch.rand(6, B, H, device=DEV) - 0.5

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
    for _ in range(10):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses


def test_cuda_graph_capture_two_layers():
    from gcm import nn as G
    torch.manual_seed(14)
    c1 = lively(G.DenseTAGConv(8, 16, 2)).to(DEV)
    c2 = lively(G.DenseTAGConv(16, 16, 1, bias=False)).to(DEV)
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
