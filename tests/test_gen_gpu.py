"""GENConv / DenseGENConv kernels (csrc/genconv.hip) against the eager restatement (tests/_gen_restate.py), evaluated
in float64 for the bound and in float32 for the restatement's own error (tests/_gcn_restate.py's rule: within 3x the
restatement's fp32 distance from float64, floors as in tests/test_gin_gpu.py).  The cases come from tests/_gen_cases.py;
tests/test_gen_cpu.py checks on the same tensors that none has an entry on relu's kink.  Needs an MI355X."""
import copy

import pytest
import torch

import _gen_cases as cases
from _gcn_restate import assert_bounded
from _gen_restate import DenseGENRef, GENRef, dense_softmax_agg, softmax_agg
from _sparse_window_restate import drop_oldest_ref, wrap_k
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _eval(fn, module, inputs, g, dtype):
    """fn(module, **inputs) in dtype -> (out, {name: gradient}) over the floating inputs and the parameters."""
    m = None if module is None else copy.deepcopy(module).to(dtype)
    ts = {k: t.detach().to(dtype).requires_grad_() for k, t in inputs.items()}
    out = fn(m, **ts)
    out.backward(g.to(dtype))
    grads = {k: t.grad for k, t in ts.items()}
    if m is not None:
        grads.update({k: p.grad for k, p in m.named_parameters() if p.requires_grad})
    return out.detach(), grads


def _check(got, grads_got, fn, module, inputs, g):
    o64, g64 = _eval(fn, module, inputs, g, torch.float64)
    o32, g32 = _eval(fn, module, inputs, g, torch.float32)
    assert got.shape == o64.shape
    assert torch.isfinite(got).all()
    assert_bounded(got, o64, o32, "out")
    for name, b64 in g64.items():
        assert b64 is not None and grads_got.get(name) is not None, name
        assert torch.isfinite(grads_got[name]).all(), name
        assert_bounded(grads_got[name], b64, g32[name], name, floor=GRAD_FLOOR, relative=True)
    return o64, g64


def _layer(cls_name, ref):
    """gcm.nn's layer with the restatement's options and weights, on the device."""
    from gcm import nn as G
    conv = getattr(G, cls_name)(
        ref.in_channels, ref.out_channels, t=ref.initial_t, learn_t=isinstance(ref.aggr_module.t, torch.nn.Parameter),
        msg_norm=hasattr(ref, "msg_norm"), learn_msg_scale=hasattr(ref, "msg_norm") and ref.msg_norm.scale.requires_grad,
        norm={torch.nn.LayerNorm: "layer", torch.nn.ReLU: None}[type(ref.mlp[1])], bias=ref.mlp[0].bias is not None)
    conv.load_state_dict(ref.state_dict())
    return conv.to(DEV)


def _param_grads(conv):
    return {k: p.grad for k, p in conv.named_parameters() if p.requires_grad}


def _with_index(ei, M, mask=None):
    """The edge list in CSR order on the device with a ready index attached, as SparseGCM hands it over."""
    from gcm import _ops
    dst, perm = torch.sort(ei[1], stable=True)
    es = ei[:, perm].contiguous().to(DEV)
    es.gcm_graph = _ops.GraphIndex(es, _ops.ptr_from_sorted(es[1].contiguous(), M), M, mask=mask)
    return es


# ---------------------------------------------------------------------------
# DenseGENConv
# ---------------------------------------------------------------------------
def _run_dense(B, N, C, opts, kind):
    from gcm import _ops
    c = cases.dense_case(B, N, C, opts)
    ref, adj, mask = c["ref"], c["adj"], c["mask"]
    if kind == "aggregation alone":
        xs, t = c["xs"].to(DEV).requires_grad_(), ref.aggr_module.t.detach().to(DEV).requires_grad_()
        a3 = adj.unsqueeze(0) if adj.dim() == 2 else adj
        out = _ops.dense_genagg(xs, a3.expand(B, N, N).to(DEV), t)
        out.backward(c["ga"].to(DEV))
        torch.cuda.synchronize()

        def fn(_, xs, t):
            return dense_softmax_agg(xs, a3.to(xs.dtype), t)

        return _check(out, {"xs": xs.grad, "t": t.grad}, fn, None, {"xs": c["xs"], "t": ref.aggr_module.t}, c["ga"])
    conv = _layer("DenseGENConv", ref)
    xd = c["x"].to(DEV).requires_grad_()
    ad = adj.to(DEV).requires_grad_()
    out = conv(xd, ad, None if mask is None else mask.to(DEV))
    out.backward(c["g"].to(DEV))
    torch.cuda.synchronize()
    assert ad.grad is None                                    # the pattern alone is read

    def fn(m, x):
        return m(x, adj.to(x.dtype), mask)

    return _check(out, {"x": xd.grad, **_param_grads(conv)}, fn, ref, {"x": c["x"]}, c["g"])


@pytest.mark.parametrize("B,N,C,opts,kind", [(*c, kind) for c in cases.DENSE for kind in ("aggregation alone", "mlp")
                                             if kind != "mlp" or c[3].get("mlp", True)])
def test_dense_genconv(B, N, C, opts, kind):
    _run_dense(B, N, C, opts, kind)


def test_dense_t_zero_is_the_mean_of_m():
    """t = 0 against aggr="mean" over m, written out: the masked mean of relu(xs) + eps."""
    from gcm import _ops
    c = cases.dense_case(3, 12, 8, {"t": 0.0})
    got = _ops.dense_genagg(c["xs"].to(DEV), c["adj"].to(DEV), torch.zeros(1, device=DEV))

    def mean(xs):
        m = torch.relu(xs) + 1e-7
        a = c["adj"].to(xs.dtype)
        return a @ m / a.sum(-1, keepdim=True).clamp(min=1)

    assert_bounded(got, mean(c["xs"].double()), mean(c["xs"]), "mean")


def test_dense_genconv_rejects_wide_layers():
    from gcm import nn as G
    conv = G.DenseGENConv(130, 130, norm=None).to(DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        conv(torch.randn(2, 5, 130, device=DEV), torch.ones(2, 5, 5, device=DEV))


# ---------------------------------------------------------------------------
# GENConv
# ---------------------------------------------------------------------------
def _run_sparse(M, E, C, opts, kind, indexed=True):
    from gcm import _ops
    c = cases.csr_case(M, E, C, opts)
    ref, ei = c["ref"], c["ei"]
    es = _with_index(ei, M) if indexed else ei.to(DEV)
    if kind == "aggregation alone":
        xs, t = c["xs"].to(DEV).requires_grad_(), ref.aggr_module.t.detach().to(DEV).requires_grad_()
        out = _ops.csr_genagg(xs, t, _with_index(ei, M).gcm_graph)
        out.backward(c["ga"].to(DEV))
        torch.cuda.synchronize()

        def fn(_, xs, t):
            return softmax_agg(xs, ei, t)

        return _check(out, {"xs": xs.grad, "t": t.grad}, fn, None, {"xs": c["xs"], "t": ref.aggr_module.t}, c["ga"])
    conv = _layer("GENConv", ref)
    xd = c["x"].to(DEV).requires_grad_()
    out = conv(xd, es)
    out.backward(c["g"].to(DEV))
    torch.cuda.synchronize()

    def fn(m, x):
        return m(x, ei)

    return _check(out, {"x": xd.grad, **_param_grads(conv)}, fn, ref, {"x": c["x"]}, c["g"])


@pytest.mark.parametrize("kind", ["aggregation alone", "mlp"])
@pytest.mark.parametrize("M,E,C,opts", cases.CSR)
def test_genconv(M, E, C, opts, kind):
    _run_sparse(M, E, C, opts, kind)


@pytest.mark.parametrize("M,E,C", [(5, 0, 4), (40, 90, 8)])
def test_genconv_builds_its_own_index(M, E, C):
    _run_sparse(M, E, C, {}, "mlp", indexed=False)


def test_genconv_rejects_a_masked_index():
    from gcm import nn as G
    M = 10
    es = _with_index(cases.edges(M, 20, seed=3), M, mask=torch.ones(M, dtype=torch.bool, device=DEV))
    conv = G.GENConv(4, 4, norm=None).to(DEV)
    with pytest.raises(ValueError, match="masked GraphIndex"):
        conv(torch.randn(M, 4, device=DEV), es)


def test_genconv_rejects_wide_layers():
    from gcm import nn as G
    conv = G.GENConv(130, 130, norm=None).to(DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        conv(torch.randn(5, 130, device=DEV), torch.tensor([[0, 1], [1, 2]], device=DEV))


def test_dense_equals_sparse():
    """The same 0/1 graph through both layers with shared weights, each against the same float64 restatement."""
    torch.manual_seed(7)
    B, N, F, C = 3, 20, 8, 8
    adj = (torch.rand(B, N, N) < 0.25).float()                # loops on the diagonal here and there
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])              # adj[b, i, j]: edge j -> i
    ref = DenseGENRef(F, C, t=1.3, learn_t=True, msg_norm=True, learn_msg_scale=True, norm="layer", bias=True)
    dconv, sconv = _layer("DenseGENConv", ref), _layer("GENConv", ref)
    x, g = torch.randn(B, N, F), torch.randn(B, N, C)
    xa, xb = x.to(DEV).requires_grad_(), x.to(DEV).requires_grad_()
    out_d = dconv(xa, adj.to(DEV))
    out_s = sconv(xb.view(B * N, F), ei.to(DEV)).view(B, N, C)
    out_d.backward(g.to(DEV))
    out_s.backward(g.to(DEV))
    torch.cuda.synchronize()

    def fn(m, x):
        return m(x, adj.to(x.dtype))

    for out, xg, conv in ((out_d, xa.grad, dconv), (out_s, xb.grad, sconv)):
        _check(out, {"x": xg, **_param_grads(conv)}, fn, ref, {"x": x}, g)


# ---------------------------------------------------------------------------
# t: a trained value; shifts of any size
# ---------------------------------------------------------------------------
def test_trained_t():
    """One SGD step on t (and everything else) on the device, then the layer against the restatement at the moved t."""
    c = cases.dense_case(3, 12, 8, {"seed": 77, "cin": 5, "norm": "layer"})
    conv = _layer("DenseGENConv", c["ref"])
    opt = torch.optim.SGD(conv.parameters(), lr=0.5)
    x, adj, g = c["x"].to(DEV), c["adj"].to(DEV), c["g"].to(DEV)
    (conv(x, adj) * g).sum().backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    moved = float(conv.aggr_module.t.detach())
    assert abs(moved - 1.0) > 1e-3
    ref = copy.deepcopy(c["ref"])
    ref.load_state_dict({k: v.cpu() for k, v in conv.state_dict().items()})
    xd = x.clone().requires_grad_()
    out = conv(xd, adj)
    out.backward(g)
    torch.cuda.synchronize()
    _check(out, {"x": xd.grad, **_param_grads(conv)}, lambda m, x: m(x, c["adj"].to(x.dtype)), ref, {"x": c["x"]},
           c["g"])


@pytest.mark.parametrize("form", ["dense", "csr"])
def test_shift_robustness(form):
    """Logits up to 400 (node 0 holds 10, t = 40) beside rows whose logits are all below 40: the pass shifts by the
    row's own maximum, so neither overflows nor - as a graph-wide shift by 400 would - underflows to 0 / 0."""
    from gcm import _ops
    c = cases.shift_case()
    N = c["x"].shape[0]
    xs, t = c["x"].to(DEV).requires_grad_(), torch.full((1,), c["t"], device=DEV).requires_grad_()
    if form == "dense":
        out = _ops.dense_genagg(xs.unsqueeze(0), c["adj"].unsqueeze(0).to(DEV), t)[0]
    else:
        out = _ops.csr_genagg(xs, t, _with_index(c["ei"], N).gcm_graph)
    out.backward(c["g"].to(DEV))
    torch.cuda.synchronize()
    o = out.detach()
    assert float(o[1].min()) > 9.9 and float(o[3:N - 1].max()) < 1.0 and float(o[N - 1].abs().max()) == 0.0
    assert float(o[3:N - 1].min()) > 0.0                      # rows that a shift by 400 would have lost

    def fn(_, xs, t):
        return softmax_agg(xs, c["ei"], t)

    _check(out, {"xs": xs.grad, "t": t.grad}, fn, None, {"xs": c["x"], "t": torch.tensor([c["t"]])}, c["g"])


# ---------------------------------------------------------------------------
# partial gradients, determinism
# ---------------------------------------------------------------------------
def _full_and_parts(conv, call, x):
    """Gradients of one scalar loss: the full set, then x only / t only / parameters only with x frozen."""
    params = {k: p for k, p in conv.named_parameters() if p.requires_grad}
    xd = x.clone().requires_grad_()
    full = torch.autograd.grad(call(xd), [xd] + list(params.values()))
    full = dict(zip(["x"] + list(params), full))
    xd = x.clone().requires_grad_()
    (gx,) = torch.autograd.grad(call(xd), [xd])
    assert torch.equal(gx, full["x"])
    xd = x.clone().requires_grad_()
    (gt,) = torch.autograd.grad(call(xd), [conv.aggr_module.t])
    assert torch.equal(gt, full["aggr_module.t"])
    gp = torch.autograd.grad(call(x.clone()), list(params.values()))       # x carries no gradient at all
    for k, a in zip(params, gp):
        assert torch.equal(a, full[k]), k
    # parameters switched off: the others are unchanged, t's kernel leg is skipped
    conv.aggr_module.t.requires_grad_(False)
    xd = x.clone().requires_grad_()
    rest = [p for k, p in params.items() if k != "aggr_module.t"]
    got = torch.autograd.grad(call(xd), [xd] + rest)
    assert torch.equal(got[0], full["x"])
    for k, a in zip([k for k in params if k != "aggr_module.t"], got[1:]):
        assert torch.equal(a, full[k]), k
    conv.aggr_module.t.requires_grad_(True)
    torch.cuda.synchronize()


def test_partial_gradients():
    c = cases.dense_case(3, 12, 8, {"cin": 5, "msg_norm": True, "learn_msg_scale": True, "norm": "layer"})
    conv = _layer("DenseGENConv", c["ref"])
    adj, g = c["adj"].to(DEV), c["g"].to(DEV)
    _full_and_parts(conv, lambda x: (conv(x, adj) * g).sum(), c["x"].to(DEV))
    c = cases.csr_case(40, 90, 8, {"cin": 5, "msg_norm": True, "learn_msg_scale": True, "norm": "layer"})
    conv = _layer("GENConv", c["ref"])
    es, g = _with_index(c["ei"], 40), c["g"].to(DEV)
    _full_and_parts(conv, lambda x: (conv(x, es) * g).sum(), c["x"].to(DEV))


def test_two_calls_are_bitwise_equal():
    from gcm import _ops
    torch.manual_seed(15)
    B, N, C = 8, 150, 40
    x = torch.randn(B, N, C, device=DEV)
    adj = (torch.rand(B, N, N, device=DEV) < 0.3).float()
    g = torch.randn(B, N, C, device=DEV)
    ei = _with_index(cases.edges(B * N, 4000, seed=16), B * N)
    for call in (lambda xs, t: _ops.dense_genagg(xs, adj, t),
                 lambda xs, t: _ops.csr_genagg(xs.view(B * N, C), t, ei.gcm_graph).view(B, N, C)):
        runs = []
        for _ in range(2):
            xs, t = x.clone().requires_grad_(), torch.full((1,), 1.7, device=DEV).requires_grad_()
            out = call(xs, t)
            out.backward(g)
            runs.append((out.detach(), xs.grad, t.grad))
        torch.cuda.synchronize()
        for a, b in zip(*runs):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# HIP-graph capture
# ---------------------------------------------------------------------------
def test_hip_graph_capture_two_layers():
    """Forward + backward of two layers with a learnt t, captured and replayed: t is read on the device, so the
    replays equal the eager run - also after t was changed in place between two replays."""
    from gcm import nn as G
    torch.manual_seed(14)
    c1 = G.DenseGENConv(8, 16, t=1.2, learn_t=True, norm="layer", msg_norm=True, learn_msg_scale=True).to(DEV)
    c2 = G.DenseGENConv(16, 16, t=0.4, learn_t=True, norm="layer").to(DEV)
    params = list(c1.parameters()) + list(c2.parameters())
    x = torch.randn(4, 20, 8, device=DEV)
    adj = (torch.rand(4, 20, 20, device=DEV) < 0.3).float()
    gout = torch.randn(4, 20, 16, device=DEV)

    def step():
        out = c2(torch.tanh(c1(x, adj)), adj)
        out.backward(gout)
        return out

    def eager():
        for p in params:
            p.grad = None
        out = step().detach().clone()
        return out, [p.grad.clone() for p in params]

    want, want_g = eager()
    with torch.no_grad():
        c1.aggr_module.t.fill_(3.0)
    want2, want2_g = eager()
    assert not torch.equal(want, want2)
    with torch.no_grad():
        c1.aggr_module.t.fill_(1.2)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            for p in params:
                p.grad = None
            step()
    torch.cuda.current_stream().wait_stream(s)
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(static_out, want, rtol=0, atol=0)
    for a, b in zip([p.grad for p in params], want_g):
        torch.testing.assert_close(a, b, rtol=0, atol=0)
    with torch.no_grad():
        c1.aggr_module.t.fill_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(static_out, want2, rtol=0, atol=0)
    for a, b in zip([p.grad for p in params], want2_g):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


# ---------------------------------------------------------------------------
# end to end through the memories: B 3, N 8, F 4, T 12 (past graph_size: the wrap is crossed)
# ---------------------------------------------------------------------------
def _dense_pair():
    from gcm import nn as G
    sig = "x, adj, weights, B, N"
    r1, r2 = cases.memory_layers(DenseGENRef)
    ref = pyg.Sequential(sig, [(r1, "x, adj -> x"), torch.nn.Tanh(), (r2, "x, adj -> x"), torch.nn.Tanh()])
    d1, d2 = cases.memory_layers(G.DenseGENConv)
    dev = G.Sequential(sig, [(d1, "x, adj -> x"), torch.nn.Tanh(), (d2, "x, adj -> x"), torch.nn.Tanh()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _sparse_pair():
    from gcm import nn as G
    sig = "x, edges, weights"
    r1, r2 = cases.memory_layers(GENRef)
    ref = pyg.Sequential(sig, [(r1, "x, edges -> x"), torch.nn.Tanh(), (r2, "x, edges -> x"), torch.nn.Tanh()])
    d1, d2 = cases.memory_layers(G.GENConv)
    dev = G.Sequential(sig, [(d1, "x, edges -> x"), torch.nn.Tanh(), (d2, "x, edges -> x"), torch.nn.Tanh()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _gw():
    m = cases.MEM
    return torch.randn(m["T"], m["B"], m["H"], generator=torch.Generator().manual_seed(23))


_DENSE_ORACLE = {}


def _dense_oracle(selector):
    """The oracle's state handling with the restatement as the GNN, in float64 and float32; computed once per
    selector and shared."""
    if selector not in _DENSE_ORACLE:
        from _knn_restate import KNNSelector
        ref, _ = _dense_pair()
        obs, gw, res = cases.memory_obs(), _gw(), {}
        for dt in (torch.float64, torch.float32):
            sel = od.TemporalBackedge([1, 2]) if selector == "temporal" else KNNSelector(2, slice(0, 3))
            r = copy.deepcopy(ref).to(dt)
            hid, outs, adjs = None, [], []
            for t in range(cases.MEM["T"]):
                mx, hid = od.dense_step(obs[t].to(dt), hid, r, graph_size=cases.MEM["N"], edge_selectors=sel)
                outs.append(mx)
                adjs.append(hid[1].clone())
            want = torch.stack(outs)
            (want * gw.to(dt)).sum().backward()
            res[dt] = (want.detach(), hid, {k: p.grad for k, p in r.named_parameters()}, adjs)
        _DENSE_ORACLE[selector] = res
    return _DENSE_ORACLE[selector]


@pytest.mark.parametrize("selector", ["temporal", "knn"])
def test_dense_gcm_with_gen_stack(selector):
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.knn import KNNEdge
    from gcm.edge_selectors.temporal import TemporalBackedge
    m = cases.MEM
    _, dev = _dense_pair()
    res = _dense_oracle(selector)
    r64, r32 = res[torch.float64], res[torch.float32]
    obs, gw = cases.memory_obs(), _gw()
    assert float(r32[3][-1].sum()) > 0 and int(r32[1][3].max()) == m["N"]     # edges exist; the wrap was crossed

    def compare(got, hidden):
        assert_bounded(got, r64[0], r32[0], "mx")
        assert_bounded(hidden[0], r64[1][0], r32[1][0], "nodes")
        assert torch.equal(hidden[1].cpu(), r32[1][1])
        for k, p in dev.named_parameters():
            assert_bounded(p.grad, r64[2][k], r32[2][k], k, floor=GRAD_FLOOR, relative=True)

    sel = TemporalBackedge([1, 2]) if selector == "temporal" else KNNEdge(2, slice(0, 3))
    mem = DenseGCM(dev, edge_selectors=sel, graph_size=m["N"])
    assert mem._structure() is None
    hidden, outs = None, []
    for t in range(m["T"]):
        mx, hidden = mem(obs[t].to(DEV), hidden)
        outs.append(mx)
        assert torch.equal(hidden[1].cpu(), r32[3][t]), t     # the adjacency after every step: bit exact
    got = torch.stack(outs)
    (got * gw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    compare(got, hidden)

    dev.zero_grad(set_to_none=True)
    got, hidden = mem.rollout(obs.to(DEV))
    (got * gw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    compare(got, hidden)


def _sparse_oracle(ref, xs, taus_list, gws, dtype):
    """drop (restatement of overflow="wrap") + oracle step per call, the restatement stack as the GNN."""
    N = cases.MEM["N"]
    r = copy.deepcopy(ref).to(dtype)
    hidden = osp.initial_hidden(xs[0], N)
    hidden = (hidden[0].to(dtype), hidden[1], hidden[2])
    outs, loss = [], 0
    for x, taus, gw in zip(xs, taus_list, gws):
        hidden = drop_oldest_ref(hidden, wrap_k(hidden[2], taus, N))
        o, hidden = osp.sparse_step(x.to(dtype), taus, hidden, r, graph_size=N, edge_selectors=osp.TemporalEdge([1, 2]))
        outs.append(o)
        loss = loss + (o * gw.to(dtype)).sum()
    loss.backward()
    return [o.detach() for o in outs], hidden, {k: p.grad for k, p in r.named_parameters()}


@pytest.mark.parametrize("mode", ["stepwise", "one-shot"])
def test_sparse_gcm_with_gen_stack(mode):
    """stepwise: T = 12 calls of one node per graph with overflow="wrap" (graph_size 8: the wrap is crossed), which
    for these 0/1 patterns is DenseGCM + TemporalBackedge([1, 2]) - the beliefs are held against the dense oracle of
    test_dense_gcm_with_gen_stack as well.  one-shot: one call; a call cannot bring more nodes than graph_size, so it
    brings the first 8 observations."""
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    m = cases.MEM
    B, N, T = m["B"], m["N"], m["T"]
    ref, dev = _sparse_pair()
    obs, gw = cases.memory_obs().transpose(0, 1).contiguous(), _gw().transpose(0, 1).contiguous()   # [B,T,*]
    if mode == "stepwise":
        xs, gws = [obs[:, t:t + 1] for t in range(T)], [gw[:, t:t + 1] for t in range(T)]
        taus_list = [torch.ones(B, dtype=torch.long)] * T
    else:
        xs, gws, taus_list = [obs[:, :N]], [gw[:, :N]], [torch.full((B,), N)]
    mem = SparseGCM(dev, edge_selectors=TemporalEdge([1, 2]), graph_size=N, overflow="wrap")
    assert mem._canonical() is None and not mem._native_gnn()
    hidden, loss, got = None, 0, []
    for x, taus, g in zip(xs, taus_list, gws):
        mx, hidden = mem(x.to(DEV), taus.to(DEV), hidden)
        got.append(mx)
        loss = loss + (mx * g.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()

    w64 = _sparse_oracle(ref, xs, taus_list, gws, torch.float64)
    w32 = _sparse_oracle(ref, xs, taus_list, gws, torch.float32)
    for i, mx in enumerate(got):
        assert_bounded(mx, w64[0][i], w32[0][i], f"mx[{i}]")
    assert_bounded(hidden[0], w64[1][0], w32[1][0], "nodes")
    assert torch.equal(hidden[2].cpu(), w32[1][2])
    assert torch.equal(hidden[1].coalesce().indices().cpu(), w32[1][1].coalesce().indices())
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, w64[2][k], w32[2][k], k, floor=GRAD_FLOOR, relative=True)
    if mode == "stepwise":                                    # dense == sparse on these 0/1 patterns
        res = _dense_oracle("temporal")
        r64, r32 = res[torch.float64], res[torch.float32]
        assert_bounded(torch.cat(got, 1).transpose(0, 1), r64[0], r32[0], "mx, dense oracle")
        for k, p in dev.named_parameters():
            assert_bounded(p.grad, r64[2][k], r32[2][k], k + ", dense oracle", floor=GRAD_FLOOR, relative=True)
