"""gcm.nn.MessagePassing and gcm.graph_utils on the kernels of csrc/message_passing.hip, against the pure-torch
restatement (tests/_mp_restate.py) evaluated in float64 for the bound and in float32 for the restatement's own error
(tests/_gcn_restate.py's rule: within 3x the restatement's fp32 distance from float64, floors 2e-6 for outputs and 5e-7
relative for gradients).  What only copies - the gathers and the forward of max / min - must be bitwise equal to the
float32 restatement.  Every shape runs with a ready CSR-ordered index (the kernels' perm = NULL path, what SparseGCM
hands over) and with a shuffled list that the base indexes itself.  Needs an MI355X."""
import copy

import pytest
import torch

import _gen_cases as gen_cases
import _mp_cases as cases
import _mp_restate as R
from _gcn_restate import assert_bounded
from _sparse_window_restate import drop_oldest_ref, wrap_k
from oracle import pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)
MODES = ["ready", "shuffled"]
AGGRS = ["add", "mean", "max", "min"]
_IDS = [f"{M}-{E}-{C}" for M, E, C in cases.SHAPES]


def _G():
    from gcm import nn as G
    return G


def _dev_layers():
    G = _G()
    return R.layers(G.MessagePassing, G)


def _ref_layers():
    return R.layers(R.RefMessagePassing)


def _edge_list(ei, M, mode):
    """-> (the list as the caller holds it on the CPU, the same on the device).  ready: stably sorted by sink with the
    index attached, as SparseGCM hands it over; shuffled: as generated, no index."""
    from gcm import _ops
    if mode == "shuffled":
        return ei, ei.to(DEV)
    es, _ = cases.csr_order(ei)
    ed = es.to(DEV)
    ed.gcm_graph = _ops.GraphIndex(ed, _ops.ptr_from_sorted(ed[1].contiguous(), M), M)
    return es, ed


def _sink_index(ed):
    """The sinks of a device list, with the GraphIndex attached when the list carries one (what propagate hands to
    message / aggregate)."""
    index = ed[1]
    if hasattr(ed, "gcm_graph"):
        index.gcm_graph = ed.gcm_graph
    return index


def _eval(fn, module, inputs, g, dtype):
    """fn(module, **inputs) in dtype on the CPU -> (out, {name: gradient}) over the inputs and the parameters."""
    m = None if module is None else copy.deepcopy(module).to(dtype)
    ts = {k: t.detach().to(dtype).requires_grad_() for k, t in inputs.items()}
    out = fn(m, **ts)
    out.backward(g.to(dtype))
    grads = {k: t.grad for k, t in ts.items()}
    if m is not None:
        grads.update({k: p.grad for k, p in m.named_parameters() if p.requires_grad})
    return out.detach(), grads


def _check(got, grads_got, fn, module, inputs, g, exact_out=False):
    o64, g64 = _eval(fn, module, inputs, g, torch.float64)
    o32, g32 = _eval(fn, module, inputs, g, torch.float32)
    assert got.shape == o64.shape and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    if exact_out:
        assert torch.equal(got.detach().cpu(), o32), "a copy must be bitwise equal"
    else:
        assert_bounded(got, o64, o32, "out")
    for name, b64 in g64.items():
        assert b64 is not None and grads_got.get(name) is not None, name
        assert grads_got[name].shape == b64.shape, name
        assert torch.isfinite(grads_got[name]).all(), name
        assert_bounded(grads_got[name], b64, g32[name], name, floor=GRAD_FLOOR, relative=True)
    return o32, g32


def _param_grads(m):
    return {k: p.grad for k, p in m.named_parameters() if p.requires_grad}


def _edges_of(base):
    class Edges(base):
        """Both gathers, handed back untouched."""

        def __init__(self):
            super().__init__(aggr=None, node_dim=0)

        def message(self, x_i, x_j):
            return x_i, x_j

        def aggregate(self, inputs):
            return torch.stack(inputs)

    return Edges()


# ---------------------------------------------------------------------------
# the primitives
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,E,C", cases.SHAPES, ids=_IDS)
def test_gathers(M, E, C, mode):
    """x_i / x_j: bitwise copies; their gradient is a segment sum over the sinks / the sources."""
    c = cases.case(M, E, C)
    es, ed = _edge_list(c["ei"], M, mode)
    g = torch.stack([c["g_e"], c["src"]])                      # two independent gradients, one per gather
    xd = c["x"].to(DEV).requires_grad_()
    out = _edges_of(_G().MessagePassing).propagate(ed, x=xd)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    ref = _edges_of(R.RefMessagePassing)
    _check(out, {"x": xd.grad}, lambda _, x: ref.propagate(es, x=x), None, {"x": c["x"]}, g, exact_out=True)


@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,E,C", cases.SHAPES, ids=_IDS)
def test_default_message_and_aggregate(M, E, C, mode, aggr):
    """propagate with the defaults: gather by source, reduce by sink.  max / min copy; sum / mean by the bound."""
    c = cases.case(M, E, C)
    es, ed = _edge_list(c["ei"], M, mode)
    xd = c["x"].to(DEV).requires_grad_()
    out = _G().MessagePassing(aggr, node_dim=0).propagate(ed, x=xd)
    out.backward(c["g_m"].to(DEV))
    torch.cuda.synchronize()
    ref = R.RefMessagePassing(aggr, node_dim=0)
    _check(out, {"x": xd.grad}, lambda _, x: ref.propagate(es, x=x), None, {"x": c["x"]}, c["g_m"],
           exact_out=aggr in ("max", "min"))
    if E == 0:
        assert float(out.detach().abs().max()) == 0.0
    else:
        assert float(out.detach()[M - 3:].abs().max()) == 0.0           # the isolated nodes: 0 for every aggr


@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,E,C", cases.SHAPES, ids=_IDS)
def test_scatter(M, E, C, mode, reduce):
    """scatter on [E, ...] rows of its own: with the index propagate attaches, and with a bare index it sorts itself."""
    c = cases.case(M, E, C)
    es, ed = _edge_list(c["ei"], M, mode)
    sd = c["src"].to(DEV).requires_grad_()
    out = _G().scatter(sd, _sink_index(ed), dim=0, dim_size=M, reduce=reduce)
    out.backward(c["g_m"].to(DEV))
    torch.cuda.synchronize()
    _check(out, {"src": sd.grad}, lambda _, src: R.scatter(src, es[1], dim_size=M, reduce=reduce), None,
           {"src": c["src"]}, c["g_m"], exact_out=reduce in ("max", "min"))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("M,E,C", cases.SHAPES, ids=_IDS)
def test_softmax(M, E, C, mode):
    c = cases.case(M, E, C)
    es, ed = _edge_list(c["ei"], M, mode)
    sd = c["src"].to(DEV).requires_grad_()
    out = _G().softmax(sd, _sink_index(ed), None, M)
    out.backward(c["g_e"].to(DEV))
    torch.cuda.synchronize()
    _check(out, {"src": sd.grad}, lambda _, src: R.softmax(src, es[1], None, M), None, {"src": c["src"]}, c["g_e"])
    if E:
        total = torch.zeros((M,) + tuple(out.shape[1:]), device=DEV).index_add_(0, ed[1], out.detach())
        deg = torch.bincount(es[1], minlength=M)
        assert float((total[deg > 0] - 1).abs().max()) < 1e-5 and float(total[deg == 0].abs().max()) == 0.0
        if (deg == 1).any():                                   # a one-entry segment gives exactly 1
            assert float((out.detach().cpu()[deg[es[1]] == 1] - 1).abs().max()) == 0.0


def test_softmax_num_nodes_from_the_index():
    """Without num_nodes the segment count comes from the attached index, else from the largest entry (as in PyG)."""
    c = cases.case(40, 90, 8)
    for mode in MODES:
        es, ed = _edge_list(c["ei"], 40, mode)
        a = _G().softmax(c["src"].to(DEV), _sink_index(ed))
        b = _G().softmax(c["src"].to(DEV), _sink_index(ed), None, 40)
        assert torch.equal(a, b)


def test_attached_index_is_refused_when_masked_and_ignored_when_it_does_not_fit():
    from gcm import _ops
    M = 40
    c = cases.case(M, 90, 8)
    es, ed = _edge_list(c["ei"], M, "ready")
    mp = _G().MessagePassing("add")
    # x has one node more than the attached index knows: the base indexes the list itself
    x41 = torch.cat([c["x"], torch.ones(1, 8)])
    out = mp.propagate(ed, x=x41.to(DEV))
    ref = R.RefMessagePassing("add")
    assert out.shape == (41, 8)
    assert_bounded(out, ref.propagate(es, x=x41.double()), ref.propagate(es, x=x41), "out")
    ed.gcm_graph = _ops.GraphIndex(ed, ed.gcm_graph.row_ptr, M, mask=torch.ones(M, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match="masked GraphIndex"):
        mp.propagate(ed, x=c["x"].to(DEV))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# the tie rule, the softmax's shift
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_tie_gradient_goes_to_the_first_edge_in_the_callers_order(mode):
    """The list of tests/_mp_cases.py::tie_case is in no sorted order: sorted by sink the tied edges keep their order
    (a stable sort), so both modes give the gradient to the same edge of the caller's list."""
    from gcm import _ops
    c = cases.tie_case()
    ei, M = c["ei"], c["M"]
    ed = ei.to(DEV)
    if mode == "ready":                                        # an index built ahead, for the list as it is
        ed.gcm_graph = _ops.GraphIndex.from_edge_index(ed, M)
    for reduce, rows in (("max", {(1, 0), (0, 1), (2, 0), (2, 1)}), ("min", {(3, 0), (1, 1), (2, 0), (2, 1)})):
        msgs = c["x"][ei[0]].to(DEV).requires_grad_()
        out = _G().scatter(msgs, _sink_index(ed), dim_size=M, reduce=reduce)
        out.sum().backward()
        want = torch.zeros(6, 2)
        for e, ch in rows:
            want[e, ch] = 1.0
        assert torch.equal(msgs.grad.cpu(), want), reduce
        # through propagate: the gradient of x is what the restatement's rule gives, exactly (sums of 0 and 1)
        xd = c["x"].to(DEV).requires_grad_()
        _G().MessagePassing(reduce).propagate(ed, x=xd).sum().backward()
        xr = c["x"].clone().requires_grad_()
        R.RefMessagePassing(reduce).propagate(ei, x=xr).sum().backward()
        assert torch.equal(xd.grad.cpu(), xr.grad), reduce
    torch.cuda.synchronize()


def test_softmax_shift_robustness():
    """tests/_gen_cases.py::shift_case: logits up to 400 (node 0 holds 10, t = 40) beside sinks whose logits are all
    below 40 - a graph-wide shift by 400 would underflow every term of theirs.  Row N - 1 is an empty segment; one-entry
    segments are checked in test_softmax."""
    c = gen_cases.shift_case()
    N, ei = c["x"].shape[0], c["ei"]
    logits = (c["t"] * c["x"])[ei[0]].contiguous()             # [E, C], the same float32 numbers on both sides
    g = torch.randn(logits.shape, generator=torch.Generator().manual_seed(41))
    for mode in MODES:
        es, ed = _edge_list(ei, N, mode)
        perm = cases.csr_order(ei)[1] if mode == "ready" else torch.arange(ei.shape[1])
        lg, gg = logits[perm].contiguous(), g[perm].contiguous()
        sd = lg.to(DEV).requires_grad_()
        out = _G().softmax(sd, _sink_index(ed), None, N)
        out.backward(gg.to(DEV))
        torch.cuda.synchronize()
        _check(out, {"src": sd.grad}, lambda _, src: R.softmax(src, es[1], None, N), None, {"src": lg}, gg)
        o = out.detach().cpu()
        assert float(o[(es[1] == 1) & (es[0] == 0)].min()) == 1.0   # beside a 400 the others of row 1 round to nothing
        assert float(o[es[1] >= 3].min()) > 0.0                # rows that a shift by 400 would have lost
        assert not (es[1] == N - 1).any()


# ---------------------------------------------------------------------------
# the restated layers over gcm.nn.MessagePassing, and beside the fused layers
# ---------------------------------------------------------------------------
def _mlp(cin, hidden, cout, seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(cin, hidden), torch.nn.ReLU(), torch.nn.Linear(hidden, cout))


_LAYER_CASES = {
    "graphconv-add": lambda L: L.GraphConv(8, 6, aggr="add"),
    "graphconv-mean": lambda L: L.GraphConv(8, 6, aggr="mean"),
    "graphconv-max": lambda L: L.GraphConv(8, 6, aggr="max"),
    "gcn": lambda L: L.GCN(8, 6),
    "gin": lambda L: L.GIN(_mlp(8, 12, 6, 3), eps=0.25, train_eps=True),
    "edgeconv": lambda L: L.EdgeConv(_mlp(16, 12, 6, 4)),
    "gatv2": lambda L: L.GATv2(8, 4, heads=3),
}
_FUSED = {
    "graphconv-add": lambda G: G.GraphConv(8, 6, aggr="add"),
    "graphconv-mean": lambda G: G.GraphConv(8, 6, aggr="mean"),
    "graphconv-max": lambda G: G.GraphConv(8, 6, aggr="max"),
    "gin": lambda G: G.GINConv(_mlp(8, 12, 6, 3), eps=0.25, train_eps=True),
    "edgeconv": lambda G: G.EdgeConv(_mlp(16, 12, 6, 4)),
}


def _layer_pair(name):
    torch.manual_seed(11)
    ref = _LAYER_CASES[name](_ref_layers())
    dev = _LAYER_CASES[name](_dev_layers())
    dev.load_state_dict(ref.state_dict())
    assert isinstance(dev, _G().MessagePassing) and not isinstance(ref, _G().MessagePassing)
    return ref, dev.to(DEV)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(_LAYER_CASES))
def test_restated_layers(name, mode):
    """The same layer body over gcm.nn.MessagePassing and over the restatement base; GraphConv, GIN and EdgeConv also
    beside gcm.nn's fused layer with the same weights, each bounded against the float64 restatement."""
    M, E = 40, 90
    c = cases.case(M, E, 8)
    es, ed = _edge_list(c["ei"], M, mode)
    ref, dev = _layer_pair(name)
    weighted = name.startswith("graphconv")
    w = torch.rand(es.shape[1], generator=torch.Generator().manual_seed(5)) + 0.5 if weighted else None
    g = torch.randn(M, 12 if name == "gatv2" else 6, generator=torch.Generator().manual_seed(6))
    inputs = {"x": c["x"], **({"w": w} if weighted else {})}

    def fn(m, x, w=None):
        return m(x, es, w) if weighted else m(x, es)

    def run(layer):
        xd = c["x"].to(DEV).requires_grad_()
        wd = w.to(DEV).requires_grad_() if weighted else None
        out = layer(xd, ed, wd) if weighted else layer(xd, ed)
        out.backward(g.to(DEV))
        torch.cuda.synchronize()
        return out, {"x": xd.grad, **({"w": wd.grad} if weighted else {}), **_param_grads(layer)}

    out, grads = run(dev)
    _check(out, grads, fn, ref, inputs, g)
    if name in _FUSED:
        fused = _FUSED[name](_G())
        fused.load_state_dict(ref.state_dict())
        out_f, grads_f = run(fused.to(DEV))
        _check(out_f, grads_f, fn, ref, inputs, g)


def test_partial_gradients():
    """Inputs only, parameters only: the same numbers as the full set, and a skipped gradient launches nothing that
    changes them."""
    M = 40
    c = cases.case(M, 90, 8)
    _, ed = _edge_list(c["ei"], M, "ready")
    for name in ("graphconv-max", "gatv2"):
        _, dev = _layer_pair(name)
        g = torch.randn(M, 12 if name == "gatv2" else 6, device=DEV)
        params = dict(dev.named_parameters())

        def loss(x):
            return (dev(x, ed) * g).sum()

        xd = c["x"].to(DEV).requires_grad_()
        full = dict(zip(["x"] + list(params), torch.autograd.grad(loss(xd), [xd] + list(params.values()))))
        xd = c["x"].to(DEV).requires_grad_()
        (gx,) = torch.autograd.grad(loss(xd), [xd])
        assert torch.equal(gx, full["x"])
        gp = torch.autograd.grad(loss(c["x"].to(DEV)), list(params.values()))     # x carries no gradient at all
        for k, a in zip(params, gp):
            assert torch.equal(a, full[k]), k
        for p in params.values():
            p.requires_grad_(False)
        xd = c["x"].to(DEV).requires_grad_()
        (gx,) = torch.autograd.grad(loss(xd), [xd])
        assert torch.equal(gx, full["x"])
    torch.cuda.synchronize()


def test_two_calls_are_bitwise_equal():
    M, E = 600, 6000
    ei = cases.edges(M, E, seed=16)
    x = torch.randn(M, 40, generator=torch.Generator().manual_seed(15)).to(DEV)
    g = torch.randn(M, 40, device=DEV)
    for mode in MODES:
        _, ed = _edge_list(ei, M, mode)
        for aggr in AGGRS:
            mp = _G().MessagePassing(aggr)
            runs = []
            for _ in range(2):
                xd = x.clone().requires_grad_()
                out = mp.propagate(ed, x=xd)
                out.backward(g)
                runs.append((out.detach(), xd.grad))
            for a, b in zip(*runs):
                assert torch.equal(a, b), (mode, aggr)
        _, dev = _layer_pair("gatv2")
        runs = []
        for _ in range(2):
            xd = x[:, :8].clone().requires_grad_()
            out = dev(xd, ed)
            out.sum().backward()
            runs.append((out.detach(), xd.grad, dev.att.grad.clone()))
            dev.zero_grad(set_to_none=True)
        for a, b in zip(*runs):
            assert torch.equal(a, b), mode
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# HIP-graph capture
# ---------------------------------------------------------------------------
def test_hip_graph_capture_two_layers():
    """Forward + backward of two subclassed layers over a ready index, captured and replayed: no host read, no
    allocation outside torch's pool, so the replay equals the eager run bit for bit."""
    M = 40
    c = cases.case(M, 90, 8)
    _, ed = _edge_list(c["ei"], M, "ready")
    L = _dev_layers()
    torch.manual_seed(14)
    c1, c2 = L.GraphConv(8, 8, aggr="max").to(DEV), L.GATv2(8, 4, heads=2).to(DEV)
    params = list(c1.parameters()) + list(c2.parameters())
    x = c["x"].to(DEV)
    gout = torch.randn(M, 8, device=DEV)

    def step():
        out = c2(torch.tanh(c1(x, ed)), ed)
        out.backward(gout)
        return out

    for p in params:
        p.grad = None
    want = step().detach().clone()
    want_g = [p.grad.clone() for p in params]

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


# ---------------------------------------------------------------------------
# end to end through SparseGCM: B 3, N 8, F 4, H 8, T 12
# ---------------------------------------------------------------------------
def _sparse_pair():
    G = _G()
    r1, r2 = cases.memory_stack(_ref_layers())
    ref = pyg.Sequential("x, edges, weights", [(r1, "x, edges, weights -> x"), torch.nn.Tanh(),
                                               (r2, "x, edges -> x"), torch.nn.Tanh()])
    d1, d2 = cases.memory_stack(_dev_layers())
    dev = G.Sequential("x, edges, weights", [(d1, "x, edges, weights -> x"), torch.nn.Tanh(), (d2, "x, edges -> x"),
                                             torch.nn.Tanh()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _gw():
    m = cases.MEM
    return torch.randn(m["B"], m["T"], m["H"], generator=torch.Generator().manual_seed(23))


def _sparse_oracle(ref, xs, taus_list, gws, dtype, wrap, max_hops):
    """The oracle's step per call (after the restatement of overflow="wrap" when asked), the restated stack as GNN."""
    N = cases.MEM["N"]
    r = copy.deepcopy(ref).to(dtype)
    hidden = osp.initial_hidden(xs[0], N)
    hidden = (hidden[0].to(dtype), hidden[1], hidden[2])
    outs, loss = [], 0
    for x, taus, gw in zip(xs, taus_list, gws):
        if wrap:
            hidden = drop_oldest_ref(hidden, wrap_k(hidden[2], taus, N))
        o, hidden = osp.sparse_step(x.to(dtype), taus, hidden, r, graph_size=N,
                                    edge_selectors=osp.TemporalEdge([1, 2]), max_hops=max_hops)
        outs.append(o)
        loss = loss + (o * gw.to(dtype)).sum()
    loss.backward()
    return [o.detach() for o in outs], hidden, {k: p.grad for k, p in r.named_parameters()}


@pytest.mark.parametrize("mode,option", [("stepwise", "wrap"), ("one-shot", "wrap"), ("stepwise", "max_hops"),
                                         ("one-shot", "max_hops")])
def test_sparse_gcm_with_subclassed_stack(mode, option):
    """A two-layer subclassed stack as SparseGCM's GNN (its generic path), against the oracle running the same bodies on
    the restatement base.  wrap: T = 12 single-node calls cross graph_size 8 with overflow="wrap"; max_hops=2: the
    relabelled lists of the k-hop path, which carry no index, over the first 8 observations.  one-shot: one call (at
    most graph_size nodes)."""
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    m = cases.MEM
    B, N = m["B"], m["N"]
    T = m["T"] if (mode, option) == ("stepwise", "wrap") else N
    ref, dev = _sparse_pair()
    obs, gw = cases.memory_obs().transpose(0, 1).contiguous(), _gw()               # [B, T, *]
    if mode == "stepwise":
        xs, gws = [obs[:, t:t + 1] for t in range(T)], [gw[:, t:t + 1] for t in range(T)]
        taus_list = [torch.ones(B, dtype=torch.long)] * T
    else:
        xs, gws, taus_list = [obs[:, :N]], [gw[:, :N]], [torch.full((B,), N)]
    wrap, max_hops = option == "wrap", 2 if option == "max_hops" else None
    mem = SparseGCM(dev, edge_selectors=TemporalEdge([1, 2]), graph_size=N, max_hops=max_hops,
                    **({"overflow": "wrap"} if wrap else {}))
    assert mem._canonical() is None and not mem._native_gnn()
    hidden, loss, got = None, 0, []
    for x, taus, g in zip(xs, taus_list, gws):
        mx, hidden = mem(x.to(DEV), taus.to(DEV), hidden)
        got.append(mx)
        loss = loss + (mx * g.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()

    w64 = _sparse_oracle(ref, xs, taus_list, gws, torch.float64, wrap, max_hops)
    w32 = _sparse_oracle(ref, xs, taus_list, gws, torch.float32, wrap, max_hops)
    for i, mx in enumerate(got):
        assert_bounded(mx, w64[0][i], w32[0][i], f"mx[{i}]")
    assert_bounded(hidden[0], w64[1][0], w32[1][0], "nodes")
    assert torch.equal(hidden[2].cpu(), w32[1][2])
    assert torch.equal(hidden[1].coalesce().indices().cpu(), w32[1][1].coalesce().indices())
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, w64[2][k], w32[2][k], k, floor=GRAD_FLOOR, relative=True)
