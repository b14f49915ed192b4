"""EdgeConv / DenseEdgeConv kernels (csrc/edgeconv.hip) against the eager restatement (tests/_edgeconv_restate.py).
The float64 target is always the LITERAL form (gather [x_i, x_j - x_i], run nn, masked max).  The fp32 evaluation that
sets the bound (tests/_gcn_restate.py's rule: within 3x the restatement's own fp32 distance from float64, floors 2e-6
for outputs and 5e-7 relative for gradients, as in tests/test_gen_gpu.py) is the DECOMPOSED form of the same
restatement, nn[2](act(P_i + Q_j)): the arithmetic the layer is specified to run.  The cases come from
tests/_edgeconv_cases.py; tests/test_edgeconv_cpu.py checks on the same tensors that every (sink, channel) has one
winner in every precision, so the winners are compared exactly.  Needs an MI355X."""
import copy

import pytest
import torch

import _edgeconv_cases as cases
from _edgeconv_restate import (DenseEdgeConvRef, EdgeConvRef, decomposed_pre, dense_edgeconv, edgeconv, make_nn)
from _gcn_restate import assert_bounded
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


def _check(got, grads_got, fn64, fn32, module, inputs, g):
    """got / grads_got against fn64 in float64, bounded by fn32's own fp32 error."""
    o64, g64 = _eval(fn64, module, inputs, g, torch.float64)
    o32, g32 = _eval(fn32, module, inputs, g, torch.float32)
    assert got.shape == o64.shape
    assert torch.isfinite(got).all()
    assert_bounded(got, o64, o32, "out")
    for name, b64 in g64.items():
        assert b64 is not None and grads_got.get(name) is not None, name
        assert torch.isfinite(grads_got[name]).all(), name
        assert_bounded(grads_got[name], b64, g32[name], name, floor=GRAD_FLOOR, relative=True)


def _param_grads(conv):
    return {k: p.grad for k, p in conv.named_parameters() if p.requires_grad}


def _with_index(ei, M, mask=None):
    """(the edge list in CSR order on the device with a ready index attached, as SparseGCM hands it over; the same
    list on the CPU)."""
    from gcm import _ops
    _, perm = torch.sort(ei[1], stable=True)
    sorted_ei = ei[:, perm].contiguous()
    es = sorted_ei.to(DEV)
    es.gcm_graph = _ops.GraphIndex(es, _ops.ptr_from_sorted(es[1].contiguous(), M), M, mask=mask)
    return es, sorted_ei


def _op_terms(c, x):
    """P, Q (fp32, from the case's x and first Linear), W2, b2, slope of a case: the operands of the op alone."""
    nn = c["nn"]
    with torch.no_grad():
        P, Q = decomposed_pre(x, nn)
    slope = nn[1].negative_slope if isinstance(nn[1], torch.nn.LeakyReLU) else 0.0
    ins = {"P": P, "Q": Q, "W2": nn[2].weight.detach()}
    if nn[2].bias is not None:
        ins["b2"] = nn[2].bias.detach()
    return ins, slope


def _act(v, slope):
    return torch.nn.functional.leaky_relu(v, slope)


# ---------------------------------------------------------------------------
# DenseEdgeConv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.DENSE))
def test_dense_op_alone(name):
    """gcm._ops.dense_edgemax on P, Q: output, winners (exact) and the gradients of P, Q, W2, b2."""
    from gcm import _ops
    c = cases.dense_case(name)
    ins, slope = _op_terms(c, c["x"])
    adj = c["adj"]
    dev = {k: t.to(DEV).requires_grad_() for k, t in ins.items()}
    out, win = _ops.dense_edgemax(dev["P"], dev["Q"], adj.to(DEV), dev["W2"], dev.get("b2"), slope, with_winner=True)
    out.backward(c["g"].to(DEV))
    torch.cuda.synchronize()

    def fn(_, P, Q, W2, b2=None):
        m = torch.nn.functional.linear(_act(P.unsqueeze(2) + Q.unsqueeze(1), slope), W2, b2)
        pat = (adj != 0).unsqueeze(-1)
        idx = m.detach().masked_fill(~pat, float("-inf")).argmax(dim=2, keepdim=True)
        o = torch.gather(m, 2, idx).squeeze(2)
        return torch.where(pat.any(dim=2), o, torch.zeros_like(o))

    _check(out, {k: t.grad for k, t in dev.items()}, fn, fn, None, ins, c["g"])
    _, want = dense_edgeconv(c["x"].double(), adj, copy.deepcopy(c["nn"]).double(), with_winner=True)
    assert win.dtype == torch.int32 and torch.equal(win.cpu().long(), want)


@pytest.mark.parametrize("name", list(cases.DENSE))
def test_dense_layer(name):
    from gcm import nn as G
    c = cases.dense_case(name)
    conv = G.DenseEdgeConv(copy.deepcopy(c["nn"])).to(DEV)
    xd = c["x"].to(DEV).requires_grad_()
    ad = c["adj"].to(DEV).requires_grad_()
    out = conv(xd, ad)
    out.backward(c["g"].to(DEV))
    torch.cuda.synchronize()
    assert ad.grad is None                                    # the pattern alone is read

    def fn(m, x):
        return m(x, c["adj"].to(x.dtype))

    inputs = {"x": c["x"]}
    o64, g64 = _eval(fn, DenseEdgeConvRef(c["nn"]), inputs, c["g"], torch.float64)
    o32, g32 = _eval(fn, DenseEdgeConvRef(c["nn"], decomposed=True), inputs, c["g"], torch.float32)
    assert_bounded(out, o64, o32, "out")
    for k, got in {"x": xd.grad, **_param_grads(conv)}.items():
        assert_bounded(got, g64[k], g32[k], k, floor=GRAD_FLOOR, relative=True)
    assert set(g64) == {"x", *_param_grads(conv)}


def test_dense_structure():
    """An empty row gives 0 and sends no gradient; a self entry is counted; the values of adj do not matter; 2-D
    inputs; the mask zeroes rows."""
    from gcm import nn as G
    c = cases.dense_case("D1")
    conv = G.DenseEdgeConv(copy.deepcopy(c["nn"])).to(DEV)
    x, adj = c["x"].to(DEV), c["adj"].to(DEV)
    xd = x.clone().requires_grad_()
    out = conv(xd, adj)
    assert float(out.detach()[:, 3].abs().max()) == 0.0       # D1's empty row
    g = torch.zeros_like(out)
    g[:, 3] = 1.0
    out.backward(g)
    assert float(xd.grad.abs().max()) == 0.0
    assert all(float(p.grad.abs().max()) == 0.0 for p in conv.parameters())
    # a graph whose only entries are self entries: out_i = nn([x_i, 0])
    eye = torch.eye(8, device=DEV).expand(2, 8, 8)
    pair = torch.cat([c["x"], torch.zeros_like(c["x"])], -1)
    with torch.no_grad():
        assert_bounded(conv(x, eye), copy.deepcopy(c["nn"]).double()(pair.double()), c["nn"](pair), "self entries")
    # values, 2-D inputs, mask
    assert torch.equal(conv(x, adj * -3.5), out.detach())
    assert torch.equal(conv(x[0], adj[0]), out.detach()[:1])
    mask = torch.rand(2, 8, generator=torch.Generator().manual_seed(1)) < 0.6
    masked = conv(x, adj, mask.to(DEV))
    assert torch.equal(masked, out.detach() * mask.to(DEV).unsqueeze(-1))
    assert float(masked[~mask.to(DEV)].abs().max()) == 0.0


def test_dense_equal_rows_route_the_gradient_to_the_lower_index():
    """Sources 2 and 5 hold bitwise equal rows and feed sink 7 only (they receive nothing themselves): every channel
    either of them wins goes to 2."""
    from gcm import nn as G
    torch.manual_seed(41)
    conv = G.DenseEdgeConv(make_nn(4, 8, 6)).to(DEV)
    x = torch.randn(1, 8, 4)
    x[0, 2] += 3.0 * x[0, 2].sign()                           # far from the others: the pair wins some channels
    x[0, 5] = x[0, 2]
    adj = torch.zeros(1, 8, 8)
    adj[0, 7, [1, 2, 5]] = 1
    xd = x.to(DEV).requires_grad_()
    out = conv(xd, adj.to(DEV))
    out.sum().backward()
    ref = dense_edgeconv(x.double(), adj, copy.deepcopy(conv.nn).cpu().double(), with_winner=True)[1]
    assert 2 in ref[0, 7].tolist() and 5 not in ref[0, 7].tolist()
    assert float(xd.grad[0, 5].abs().max()) == 0.0 and float(xd.grad[0, 2].abs().max()) > 0.0


def test_dense_rejects_wide_layers():
    from gcm import nn as G
    for H, C in ((130, 4), (4, 130)):
        conv = G.DenseEdgeConv(make_nn(3, H, C)).to(DEV)
        with pytest.raises(RuntimeError, match="code -2"):
            conv(torch.randn(2, 5, 3, device=DEV), torch.ones(2, 5, 5, device=DEV))


# ---------------------------------------------------------------------------
# EdgeConv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.CSR)
def test_csr_op_alone(name):
    from gcm import _ops
    c = cases.csr_case(name)
    M = c["x"].shape[0]
    es, ei = _with_index(c["ei"], M)
    ins, slope = _op_terms(c, c["x"])
    dev = {k: t.to(DEV).requires_grad_() for k, t in ins.items()}
    out, win = _ops.csr_edgemax(dev["P"], dev["Q"], dev["W2"], dev.get("b2"), slope, es.gcm_graph, with_winner=True)
    out.backward(c["g"].to(DEV))
    torch.cuda.synchronize()
    src, dst, E = ei[0], ei[1], ei.shape[1]

    def fn(_, P, Q, W2, b2=None):
        m = torch.nn.functional.linear(_act(P[dst] + Q[src], slope), W2, b2)
        C = m.shape[1]
        d2 = dst.unsqueeze(-1).expand(E, C)
        top = torch.full((M, C), float("-inf"), dtype=m.dtype).scatter_reduce(0, d2, m.detach(), reduce="amax")
        pos = torch.arange(E).unsqueeze(-1).expand(E, C)
        w = torch.full((M, C), E).scatter_reduce(0, d2, torch.where(m.detach() == top[dst], pos, E), reduce="amin")
        o = torch.gather(torch.cat([m, m.new_zeros(1, C)]), 0, w)
        return torch.where(w < E, o, torch.zeros_like(o))

    _check(out, {k: t.grad for k, t in dev.items()}, fn, fn, None, ins, c["g"])
    _, want = edgeconv(c["x"].double(), ei, copy.deepcopy(c["nn"]).double(), with_winner=True)
    assert win.dtype == torch.int32 and torch.equal(win.cpu().long(), want)     # positions in CSR order


@pytest.mark.parametrize("name,indexed", [(n, True) for n in cases.CSR] + [(n, False) for n in ("D1", "D5", cases.CSR_EXTRA)])
def test_csr_layer(name, indexed):
    """indexed: the CSR-ordered list with SparseGCM's index attached; else the raw list, indexed by the layer."""
    from gcm import nn as G
    c = cases.csr_case(name)
    M = c["x"].shape[0]
    conv = G.EdgeConv(copy.deepcopy(c["nn"])).to(DEV)
    xd = c["x"].to(DEV).requires_grad_()
    out = conv(xd, _with_index(c["ei"], M)[0] if indexed else c["ei"].to(DEV))
    out.backward(c["g"].to(DEV))
    torch.cuda.synchronize()

    def fn(m, x):
        return m(x, c["ei"])

    inputs = {"x": c["x"]}
    o64, g64 = _eval(fn, EdgeConvRef(c["nn"]), inputs, c["g"], torch.float64)
    o32, g32 = _eval(fn, EdgeConvRef(c["nn"], decomposed=True), inputs, c["g"], torch.float32)
    assert_bounded(out, o64, o32, "out")
    for k, got in {"x": xd.grad, **_param_grads(conv)}.items():
        assert_bounded(got, g64[k], g32[k], k, floor=GRAD_FLOOR, relative=True)


def test_csr_structure_and_first_entry_ties():
    """No edges at all; isolated nodes give 0; sources 5 and 2 hold bitwise equal rows and feed sink 7 in that order:
    the first CSR entry, 5 -> 7, takes the gradient."""
    from gcm import nn as G
    torch.manual_seed(42)
    conv = G.EdgeConv(make_nn(4, 8, 6)).to(DEV)
    x = torch.randn(8, 4)
    x[2] += 3.0 * x[2].sign()
    x[5] = x[2]
    xd = x.to(DEV).requires_grad_()
    none = conv(xd, torch.zeros(2, 0, dtype=torch.long, device=DEV))
    assert none.shape == (8, 6) and float(none.abs().max()) == 0.0
    none.sum().backward()
    assert float(xd.grad.abs().max()) == 0.0
    xd.grad = None
    ei = torch.tensor([[1, 5, 2], [7, 7, 7]])
    out = conv(xd, ei.to(DEV))
    assert float(out[:7].abs().max()) == 0.0
    out.sum().backward()
    ref = edgeconv(x.double(), ei, copy.deepcopy(conv.nn).cpu().double(), with_winner=True)[1]
    assert 1 in ref[7].tolist() and 2 not in ref[7].tolist()   # entry 1 is 5 -> 7, entry 2 is 2 -> 7
    assert float(xd.grad[2].abs().max()) == 0.0 and float(xd.grad[5].abs().max()) > 0.0


def test_csr_rejects_a_masked_index_and_wide_layers():
    from gcm import nn as G
    M = 10
    ei = torch.randint(0, M, (2, 20), generator=torch.Generator().manual_seed(3))
    es, _ = _with_index(ei, M, mask=torch.ones(M, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="masked GraphIndex"):
        G.EdgeConv(make_nn(4, 4, 4)).to(DEV)(torch.randn(M, 4, device=DEV), es)
    conv = G.EdgeConv(make_nn(3, 130, 4)).to(DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        conv(torch.randn(5, 3, device=DEV), torch.tensor([[0, 1], [1, 2]], device=DEV))


def test_dense_equals_sparse():
    """The same 0/1 graph through both layers with shared weights: bitwise the same messages, so the same output."""
    from gcm import nn as G
    c, s = cases.dense_case("D5"), cases.csr_case("D5")
    dconv = G.DenseEdgeConv(copy.deepcopy(c["nn"])).to(DEV)
    sconv = G.EdgeConv(copy.deepcopy(c["nn"])).to(DEV)
    out_d = dconv(c["x"].to(DEV), c["adj"].to(DEV))
    out_s = sconv(s["x"].to(DEV), s["ei"].to(DEV))
    assert torch.equal(out_d.view_as(out_s), out_s)


# ---------------------------------------------------------------------------
# partial gradients, determinism
# ---------------------------------------------------------------------------
def _full_and_parts(conv, call, x):
    """Gradients of one scalar loss: the full set, then inputs only / nn.2 only / biases only.  The backward has no
    atomics and every output its own kernel: the parts equal the slices of the full backward bitwise."""
    params = dict(conv.named_parameters())
    xd = x.clone().requires_grad_()
    full = dict(zip(["x"] + list(params), torch.autograd.grad(call(xd), [xd] + list(params.values()))))
    xd = x.clone().requires_grad_()
    (gx,) = torch.autograd.grad(call(xd), [xd])
    assert torch.equal(gx, full["x"])
    for keys in (["nn.2.weight", "nn.2.bias"], ["nn.0.bias", "nn.2.bias"]):
        got = torch.autograd.grad(call(x.clone()), [params[k] for k in keys])      # x carries no gradient at all
        for k, a in zip(keys, got):
            assert torch.equal(a, full[k]), k
    # a frozen nn.2: the others are unchanged
    for k in ("nn.2.weight", "nn.2.bias"):
        params[k].requires_grad_(False)
    xd = x.clone().requires_grad_()
    got = torch.autograd.grad(call(xd), [xd, params["nn.0.weight"], params["nn.0.bias"]])
    for k, a in zip(["x", "nn.0.weight", "nn.0.bias"], got):
        assert torch.equal(a, full[k]), k
    torch.cuda.synchronize()


def test_partial_gradients():
    from gcm import nn as G
    c = cases.dense_case("D2-leaky")
    conv = G.DenseEdgeConv(copy.deepcopy(c["nn"])).to(DEV)
    adj, g = c["adj"].to(DEV), c["g"].to(DEV)
    _full_and_parts(conv, lambda x: (conv(x, adj) * g).sum(), c["x"].to(DEV))
    c = cases.csr_case(cases.CSR_EXTRA)
    conv = G.EdgeConv(copy.deepcopy(c["nn"])).to(DEV)
    es, g = _with_index(c["ei"], c["x"].shape[0])[0], c["g"].to(DEV)
    _full_and_parts(conv, lambda x: (conv(x, es) * g).sum(), c["x"].to(DEV))


def test_two_calls_are_bitwise_equal():
    from gcm import nn as G
    torch.manual_seed(15)
    B, N, F = 8, 150, 12
    x = torch.randn(B, N, F, device=DEV)
    adj = (torch.rand(B, N, N, device=DEV) < 0.3).float()
    g = torch.randn(B, N, 40, device=DEV)
    ei = torch.randint(0, B * N, (2, 4000), device=DEV)
    nn = make_nn(F, 24, 40)
    dconv, sconv = G.DenseEdgeConv(copy.deepcopy(nn)).to(DEV), G.EdgeConv(copy.deepcopy(nn)).to(DEV)
    for conv, call in ((dconv, lambda x: dconv(x, adj)), (sconv, lambda x: sconv(x.view(B * N, F), ei).view(B, N, 40))):
        runs = []
        for _ in range(2):
            conv.zero_grad(set_to_none=True)
            xs = x.clone().requires_grad_()
            out = call(xs)
            out.backward(g)
            runs.append((out.detach(), xs.grad, *[p.grad for p in conv.parameters()]))
        torch.cuda.synchronize()
        for a, b in zip(*runs):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# end to end through the memories: B 3, N 8, F 6, T 11 (past graph_size: the overflow is crossed)
# ---------------------------------------------------------------------------
def _dense_pair(decomposed=False):
    from gcm import nn as G
    sig = "x, adj, weights, B, N"
    n1, n2 = cases.memory_nns()
    ref = pyg.Sequential(sig, [(DenseEdgeConvRef(n1, decomposed), "x, adj -> x"), torch.nn.Tanh(),
                               (DenseEdgeConvRef(n2, decomposed), "x, adj -> x"), torch.nn.Tanh()])
    d1, d2 = cases.memory_nns()
    dev = G.Sequential(sig, [(G.DenseEdgeConv(d1), "x, adj -> x"), torch.nn.Tanh(),
                             (G.DenseEdgeConv(d2), "x, adj -> x"), torch.nn.Tanh()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _sparse_pair(decomposed=False):
    from gcm import nn as G
    sig = "x, edges, weights"
    n1, n2 = cases.memory_nns()
    ref = pyg.Sequential(sig, [(EdgeConvRef(n1, decomposed), "x, edges -> x"), torch.nn.Tanh(),
                               (EdgeConvRef(n2, decomposed), "x, edges -> x"), torch.nn.Tanh()])
    d1, d2 = cases.memory_nns()
    dev = G.Sequential(sig, [(G.EdgeConv(d1), "x, edges -> x"), torch.nn.Tanh(),
                             (G.EdgeConv(d2), "x, edges -> x"), torch.nn.Tanh()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _gw():
    m = cases.MEM
    return torch.randn(m["T"], m["B"], m["H"], generator=torch.Generator().manual_seed(33))


def _dense_oracle(selector):
    """The oracle's state handling with the restated layers as the GNN: float64 literal, float32 decomposed."""
    from _knn_restate import KNNSelector
    obs, gw, res = cases.memory_obs(), _gw(), {}
    for dt in (torch.float64, torch.float32):
        sel = od.TemporalBackedge([1, 2]) if selector == "temporal" else KNNSelector(3, slice(0, 3))
        r = _dense_pair(decomposed=dt == torch.float32)[0].to(dt)
        hid, outs, adjs = None, [], []
        for t in range(cases.MEM["T"]):
            mx, hid = od.dense_step(obs[t].to(dt), hid, r, graph_size=cases.MEM["N"], edge_selectors=sel)
            outs.append(mx)
            adjs.append(hid[1].clone())
        want = torch.stack(outs)
        (want * gw.to(dt)).sum().backward()
        res[dt] = (want.detach(), hid, {k: p.grad for k, p in r.named_parameters()}, adjs)
    return res


@pytest.mark.parametrize("selector", ["temporal", "knn"])
def test_dense_gcm_with_edgeconv_stack(selector):
    """T single steps and rollout(obs), each against the oracle driving the restated layers."""
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.knn import KNNEdge
    from gcm.edge_selectors.temporal import TemporalBackedge
    m = cases.MEM
    _, dev = _dense_pair()
    res = _dense_oracle(selector)
    r64, r32 = res[torch.float64], res[torch.float32]
    obs, gw = cases.memory_obs(), _gw()
    assert float(r32[3][-1].sum()) > 0 and int(r32[1][3].max()) == m["N"]     # edges exist; the overflow was crossed

    def compare(got, hidden):
        assert_bounded(got, r64[0], r32[0], "mx")
        assert_bounded(hidden[0], r64[1][0], r32[1][0], "nodes")
        assert torch.equal(hidden[1].cpu(), r32[1][1])
        for k, p in dev.named_parameters():
            assert_bounded(p.grad, r64[2][k], r32[2][k], k, floor=GRAD_FLOOR, relative=True)

    sel = TemporalBackedge([1, 2]) if selector == "temporal" else KNNEdge(3, slice(0, 3))
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
    stepwise = got.detach().clone()

    dev.zero_grad(set_to_none=True)
    got, hidden = mem.rollout(obs.to(DEV))
    (got * gw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    compare(got, hidden)
    assert torch.equal(got.detach(), stepwise)                # rollout(obs) is the T single steps


@pytest.mark.parametrize("max_hops", [None, 2])
@pytest.mark.parametrize("mode", ["stepwise", "one-shot"])
def test_sparse_gcm_with_edgeconv_stack(mode, max_hops):
    """stepwise: 8 calls of one node per graph; one-shot: one call with 8 nodes per graph (a call cannot bring more
    than graph_size)."""
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    m = cases.MEM
    B, N = m["B"], m["N"]
    _, dev = _sparse_pair()
    obs, gw = cases.memory_obs().transpose(0, 1).contiguous()[:, :N], _gw().transpose(0, 1).contiguous()[:, :N]
    if mode == "stepwise":
        xs, gws = [obs[:, t:t + 1] for t in range(N)], [gw[:, t:t + 1] for t in range(N)]
        taus_list = [torch.ones(B, dtype=torch.long)] * N
    else:
        xs, gws, taus_list = [obs], [gw], [torch.full((B,), N)]
    mem = SparseGCM(dev, edge_selectors=TemporalEdge([1, 2]), graph_size=N, max_hops=max_hops)
    assert mem._canonical() is None and not mem._native_gnn()
    hidden, loss, got = None, 0, []
    for x, taus, g in zip(xs, taus_list, gws):
        mx, hidden = mem(x.to(DEV), taus.to(DEV), hidden)
        got.append(mx)
        loss = loss + (mx * g.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()

    res = {}
    for dt in (torch.float64, torch.float32):
        r = _sparse_pair(decomposed=dt == torch.float32)[0].to(dt)
        h0 = osp.initial_hidden(xs[0], N)
        h = (h0[0].to(dt), torch.zeros((B, N, N), dtype=dt, layout=torch.sparse_coo), h0[2])
        loss_r, outs = 0, []
        for x, taus, g in zip(xs, taus_list, gws):
            o, h = osp.sparse_step(x.to(dt), taus, h, r, graph_size=N, edge_selectors=osp.TemporalEdge([1, 2]),
                                   max_hops=max_hops)
            outs.append(o)
            loss_r = loss_r + (o * g.to(dt)).sum()
        loss_r.backward()
        res[dt] = (outs, h, {k: p.grad for k, p in r.named_parameters()})
    w64, w32 = res[torch.float64], res[torch.float32]
    for i, mx in enumerate(got):
        assert_bounded(mx, w64[0][i], w32[0][i], f"mx[{i}]")
    assert_bounded(hidden[0], w64[1][0], w32[1][0], "nodes")
    assert torch.equal(hidden[2].cpu(), w32[1][2])
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, w64[2][k], w32[2][k], k, floor=GRAD_FLOOR, relative=True)
