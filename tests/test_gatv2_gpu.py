"""GATv2Conv / DenseGATv2Conv kernels (csrc/gatv2conv.hip) against the eager restatement (tests/_gatv2_restate.py),
evaluated in float64 for the bound and in float32 for the restatement's own error (tests/_gcn_restate.py's rule: 3 x
that error, floors 2e-6 for outputs and 5e-7 of the gradient's scale for gradients).  The inputs of the case tables are
quantised so that every LeakyReLU argument is exact in fp32 (tests/test_gatv2_cpu.py checks it): the side of the kink
cannot differ between the kernels and the reference.  Needs an MI355X."""
import copy

import pytest
import torch

from _gatv2_restate import (DENSE_CASES, SPARSE_CASES, DenseGATv2Ref, GATv2Ref, case_id, dense_case, layer_kwargs,
                            quant_layer, sparse_case)
from _gcn_restate import assert_bounded
from _gine_restate import RelativeEdgeAttrRef, quant
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _make(cls, case, seed, **variant):
    """A gcm.gatv2 layer of the case with quantised Linear parameters (on the CPU) and the arguments it was built
    from."""
    kw = {**layer_kwargs(case), **variant}
    conv = cls(**kw)
    quant_layer(conv, torch.Generator().manual_seed(seed))
    return conv, kw


def _with_index(ei, M):
    """The edge list (already in CSR order) on the device with a ready index attached, as SparseGCM hands it over."""
    from gcm import _ops
    es = ei.contiguous().to(DEV)
    es.gcm_graph = _ops.GraphIndex(es, _ops.ptr_from_sorted(es[1].contiguous(), M), M)
    return es


def _named_grads(conv):
    return {k: p.grad for k, p in conv.named_parameters()}


def _ref_eval(ref_cls, conv, kw, call, inputs, g, dtype):
    """The restated module with conv's state in dtype -> (out, {name: gradient})."""
    kw = {k: v for k, v in kw.items() if k != "dropout"}
    ref = ref_cls(**kw)
    ref.load_state_dict(conv.state_dict())
    ref = ref.to(dtype)
    ts = {k: t.detach().to(dtype).requires_grad_() for k, t in inputs.items() if t is not None}
    out = call(ref, **ts)
    out.backward(g.to(dtype))
    grads = {k: t.grad for k, t in ts.items()}
    grads.update(_named_grads(ref))
    return out, grads


def _check(out, got, ref_cls, conv, kw, call, inputs, g):
    o64, g64 = _ref_eval(ref_cls, conv, kw, call, inputs, g, torch.float64)
    o32, g32 = _ref_eval(ref_cls, conv, kw, call, inputs, g, torch.float32)
    assert out.shape == o64.shape
    assert not torch.isnan(out).any()
    assert_bounded(out, o64, o32, "out")
    assert set(g64) <= set(got), (sorted(g64), sorted(got))
    for name, b64 in g64.items():
        assert b64 is not None and got[name] is not None, name
        assert got[name].shape == b64.shape, name
        assert not torch.isnan(got[name]).any(), name
        assert_bounded(got[name], b64, g32[name], name, floor=GRAD_FLOOR, relative=True)


# ---------------------------------------------------------------------------
# GATv2Conv
# ---------------------------------------------------------------------------
def _sparse_operands(case, presorted):
    x, ei, ea = sparse_case(*case)
    if presorted:
        _, perm = torch.sort(ei[1], stable=True)
        ei, ea = ei[:, perm].contiguous(), None if ea is None else ea[perm].contiguous()
    return x, ei, ea


def _run_sparse(case, indexed=True, presorted=None, loops=True, eval_mode=False, **variant):
    from gcm import gatv2 as GV
    M, E, Fi, H, C, D, _ = case
    presorted = indexed if presorted is None else presorted
    x, ei, ea = _sparse_operands(case, presorted)
    conv, kw = _make(GV.GATv2Conv, case, M + E, add_self_loops=loops, **variant)
    Fo = H * C if kw["concat"] else C
    g = torch.randn(M, Fo, generator=torch.Generator().manual_seed(E))
    dconv = copy.deepcopy(conv).to(DEV)
    if eval_mode:
        dconv.eval()
    xd = x.float().to(DEV).requires_grad_()
    ead = None if ea is None else ea.float().to(DEV).requires_grad_()
    out = dconv(xd, _with_index(ei, M) if indexed else ei.to(DEV), ead)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    got = {"x": xd.grad, "edge_attr": None if ead is None else ead.grad, **_named_grads(dconv)}
    if ea is not None and loops:                                  # a skipped i -> i edge gets no gradient
        assert not ead.grad[(ei[0] == ei[1]).to(DEV)].any()
    _check(out, got, GATv2Ref, conv, kw, lambda ref, x, edge_attr=None: ref(x, ei, edge_attr),
           {"x": x, "edge_attr": ea}, g)
    return out, got


@pytest.mark.parametrize("indexed", [True, False], ids=["attached-index", "plain-list"])
@pytest.mark.parametrize("case", SPARSE_CASES, ids=case_id)
def test_gatv2conv(case, indexed):
    """Output and every gradient; with SparseGCM's attached index (the list in CSR order) and with a plain list in no
    particular order, which the layer indexes itself."""
    _run_sparse(case, indexed)


_MEAN, _FILL = SPARSE_CASES[2], SPARSE_CASES[3]


@pytest.mark.parametrize("variant", [
    dict(share_weights=True), dict(bias=False), dict(negative_slope=0.05), dict(negative_slope=0.5),
    dict(loops=False), dict(dropout=0.5, eval_mode=True), dict(share_weights=True, bias=False, loops=False)],
    ids=["share_weights", "no-bias", "slope0.05", "slope0.5", "no-self-loops", "eval-dropout", "shared-no-bias-no-loops"])
@pytest.mark.parametrize("case", [_MEAN, _FILL], ids=case_id)
def test_gatv2conv_variants(case, variant):
    """bias=False: z can be exactly 0 (the convention at 0); add_self_loops=False: isolated destinations output bias."""
    out, _ = _run_sparse(case, **variant)
    if variant.get("loops") is False and variant.get("bias", True):
        assert out[-3:].abs().max() > 0 and torch.equal(out[-3], out[-1])         # bias, thrice


def test_an_unsorted_list_equals_the_presorted_one_bit_for_bit():
    """The csr_perm path: edge_attr stays in the caller's order and is reached through the index's permutation."""
    out_u, got_u = _run_sparse(_MEAN, indexed=False, presorted=False)
    out_s, got_s = _run_sparse(_MEAN, indexed=True)
    out_p, _ = _run_sparse(_MEAN, indexed=False, presorted=True)
    _, perm = torch.sort(sparse_case(*_MEAN)[1][1], stable=True)
    assert torch.equal(out_u, out_s) and torch.equal(out_p, out_s)
    for k in got_s:
        a = got_u[k][perm.to(DEV)] if k == "edge_attr" else got_u[k]
        assert torch.equal(a, got_s[k]), k


def test_wide_layers_are_refused_before_any_launch():
    from gcm import gatv2 as GV
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    with pytest.raises(ValueError, match="128"):
        GV.GATv2Conv(130, 4).to(DEV)(torch.randn(5, 130, device=DEV), ei)
    with pytest.raises(ValueError, match="128"):
        GV.GATv2Conv(4, 33, heads=4).to(DEV)(torch.randn(5, 4, device=DEV), ei)
    with pytest.raises(ValueError, match="32"):
        GV.GATv2Conv(4, 4, edge_dim=33).to(DEV)(torch.randn(5, 4, device=DEV), ei, torch.randn(2, 33, device=DEV))
    with pytest.raises(ValueError, match="128"):
        GV.DenseGATv2Conv(4, 65, heads=2).to(DEV)(torch.randn(1, 3, 4, device=DEV), torch.ones(1, 3, 3, device=DEV))
    from gcm import _hip                                          # and by the library itself: a code, not a fault
    t = torch.zeros(64, device=DEV)
    p = _hip.ptr(t)
    rc = _hip.lib().gcm_csr_gatv2_fwd(p, p, None, None, None, p, p, None, p, p, p, None, p, p, None, p, p, None, 0,
                                      2, 1, 4, 2, 2, 33, 1, 1, 1, 0.0, 0.2, _hip.stream())
    assert rc == _hip.GCM_EUNSUPPORTED
    rc = _hip.lib().gcm_csr_gatv2_fwd(p, None, None, None, None, p, None, None, None, p, p, None, p, p, None, p, p,
                                      None, 0, 2, 1, 4, 2, 2, 0, 1, 1, 1, 0.0, 0.2, _hip.stream())
    assert rc == _hip.EINVAL


# ---------------------------------------------------------------------------
# DenseGATv2Conv
# ---------------------------------------------------------------------------
def _run_dense(case, weights=None, adj_grad=False, **variant):
    from gcm import gatv2 as GV
    B, N, Fi, H, C, D, opts = case
    add_loop = opts.get("add_loop", True)
    x, adj, ea, mask = dense_case(*case)
    conv, kw = _make(GV.DenseGATv2Conv, case, B + N, **variant)
    Fo = H * C if kw["concat"] else C
    g = torch.randn(B, N, Fo, generator=torch.Generator().manual_seed(N))
    dconv = copy.deepcopy(conv).to(DEV)
    ea_dev = None
    if ea is not None:                                            # the unset entries are not read
        ea_dev = torch.where((adj != 0).unsqueeze(-1), ea.float(), torch.full((), float("nan"))).to(DEV).requires_grad_()
    xd = x.float().to(DEV).requires_grad_()
    ad = (adj if weights is None else adj * weights).float().to(DEV).requires_grad_(adj_grad)
    out = dconv(xd, ad, ea_dev, None if mask is None else mask.to(DEV), add_loop=add_loop)
    out.backward(g.to(DEV).view(out.shape))
    torch.cuda.synchronize()
    assert ad.grad is None
    got = {"x": xd.grad, "edge_attr": None if ea is None else ea_dev.grad, **_named_grads(dconv)}
    if ea is not None:                                            # zero where unset
        assert ea_dev.grad.shape == ea_dev.shape
        assert not ea_dev.grad[(ad.detach() == 0).expand_as(ea_dev[..., 0])].any()
    _check(out, got, DenseGATv2Ref, conv, kw,
           lambda ref, x, edge_attr=None: ref(x, adj, edge_attr, mask, add_loop).view(out.shape),
           {"x": x, "edge_attr": ea}, g.view(out.shape))
    return out, got


@pytest.mark.parametrize("case", DENSE_CASES, ids=case_id)
def test_dense_gatv2conv(case):
    """Also: NaN in edge_attr at the unset entries.  N = 130 is five neighbour tiles, the last with two entries, and
    more than one workgroup of rows per graph; N <= 32 is a single tile."""
    _run_dense(case)


@pytest.mark.parametrize("variant", [dict(fill_value=0.5), dict(share_weights=True), dict(bias=False),
                                     dict(negative_slope=0.5)],
                         ids=["fill0.5", "share_weights", "no-bias", "slope0.5"])
def test_dense_gatv2conv_variants(variant):
    _run_dense(DENSE_CASES[2], **variant)


@pytest.mark.parametrize("form", ["two_d", "broadcast"])
def test_dense_operand_forms(form):
    """[N,F] / [N,N] / [N,N,D] operands, and one adjacency and edge_attr for the whole batch."""
    _run_dense((1 if form == "two_d" else 4, 20, 6, 2, 4, 2, {form: True}))


def test_an_adjacency_that_requires_grad_gets_none():
    _run_dense(DENSE_CASES[2], adj_grad=True)


def test_only_the_pattern_matters():
    case = DENSE_CASES[2]
    B, N = case[:2]
    w = quant((B, N, N), 4, 8, torch.Generator().manual_seed(5), 1 / 8)           # both signs, never 0
    out_w, got_w = _run_dense(case, weights=w)
    out_1, got_1 = _run_dense(case)
    assert torch.equal(out_w, out_1)
    for k in got_1:
        assert torch.equal(got_w[k], got_1[k]), k


@pytest.mark.parametrize("fill", ["mean", 0.5])
@pytest.mark.parametrize("add_loop", [True, False], ids=["loops", "no-loops"])
def test_dense_equals_sparse(add_loop, fill):
    """A {0,1} adjacency through DenseGATv2Conv, and through GATv2Conv on DenseToSparse(transpose=True)'s list with
    add_self_loops = add_loop and the same state: each within its bound of the same float64 restatement."""
    from gcm import gatv2 as GV
    from gcm.gcm import DenseToSparse
    case = (3, 40, 8, 2, 8, 3, {"add_loop": add_loop, "fill_value": fill})
    B, N, Fi, H, C, D, _ = case
    x, adj, ea, _ = dense_case(*case)
    conv, kw = _make(GV.DenseGATv2Conv, case, 3)
    g = torch.randn(B, N, H * C, generator=torch.Generator().manual_seed(7))
    dconv = copy.deepcopy(conv).to(DEV)
    sconv = GV.GATv2Conv(add_self_loops=add_loop, **kw).to(DEV)
    sconv.load_state_dict(dconv.state_dict())
    ad = adj.float().to(DEV)
    xa, xb = x.float().to(DEV).requires_grad_(), x.float().to(DEV).requires_grad_()
    ea_a, ea_b = ea.float().to(DEV).requires_grad_(), ea.float().to(DEV).requires_grad_()
    out_d = dconv(xa, ad, ea_a, add_loop=add_loop)
    x_sp, ei, _ = DenseToSparse(transpose=True)(xb, ad)
    bb, ii, jj = ad.nonzero(as_tuple=True)                        # the list's order: (b, row, column)
    assert torch.equal(ei, torch.stack([bb * N + jj, bb * N + ii]))
    out_s = sconv(x_sp, ei, ea_b[bb, ii, jj]).view(B, N, H * C)
    out_d.backward(g.to(DEV))
    out_s.backward(g.to(DEV))
    torch.cuda.synchronize()
    for out, xg, eg, c in ((out_d, xa.grad, ea_a.grad, dconv), (out_s, xb.grad, ea_b.grad, sconv)):
        got = {"x": xg, "edge_attr": eg, **_named_grads(c)}
        _check(out, got, DenseGATv2Ref, conv, kw, lambda ref, x, edge_attr: ref(x, adj, edge_attr, None, add_loop),
               {"x": x, "edge_attr": ea}, g)


# ---------------------------------------------------------------------------
# subsets of wanted gradients, determinism, capture
# ---------------------------------------------------------------------------
def _sparse_setup():
    from gcm import gatv2 as GV
    case = _FILL
    x, ei, ea = _sparse_operands(case, True)
    conv, kw = _make(GV.GATv2Conv, case, 1)
    return (conv.to(DEV), x.float().to(DEV), _with_index(ei, case[0]), ea.float().to(DEV),
            torch.randn(case[0], case[3] * case[4], device=DEV))


def _dense_setup():
    from gcm import gatv2 as GV
    case = (2, 40, 16, 4, 4, 4, {})
    x, adj, ea, _ = dense_case(*case)
    conv, kw = _make(GV.DenseGATv2Conv, case, 2)
    return conv.to(DEV), x.float().to(DEV), adj.float().to(DEV), ea.float().to(DEV), torch.randn(2, 40, 16, device=DEV)


@pytest.mark.parametrize("setup", [_sparse_setup, _dense_setup], ids=["sparse", "dense"])
def test_subsets_of_wanted_gradients(setup):
    """Each gradient is computed only when wanted, and then equals the full run's bit for bit."""
    conv, x, edges, ea, g = setup()
    groups = {"lin_l": list(conv.lin_l.parameters()), "lin_r": list(conv.lin_r.parameters()), "att": [conv.att],
              "lin_edge": list(conv.lin_edge.parameters()), "bias": [conv.bias]}
    every = tuple(groups)

    def run(frozen=(), wanted=("x", "edge_attr")):
        for name, ps in groups.items():
            for p in ps:
                p.requires_grad_(name not in frozen)
                p.grad = None
        xs, eas = x.clone().requires_grad_("x" in wanted), ea.clone().requires_grad_("edge_attr" in wanted)
        out = conv(xs, edges, eas)
        ins = [t for t in (xs, eas) if t.requires_grad]
        params = [p for p in conv.parameters() if p.requires_grad]
        grads = torch.autograd.grad(out, ins + params, g)
        res = {k: None for k in ("x", "edge_attr")}
        res.update({k: None for k, _ in conv.named_parameters()})
        res.update(dict(zip([k for k in ("x", "edge_attr") if k in wanted], grads)))
        res.update(dict(zip([k for k, p in conv.named_parameters() if p.requires_grad], grads[len(ins):])))
        return res

    full = run()
    assert all(v is not None for v in full.values())
    for frozen, wanted in [(("lin_r",), ("x", "edge_attr")), (every, ("x", "edge_attr")), (every, ("x",)),
                           (tuple(k for k in every if k != "att"), ()), (every, ("edge_attr",)),
                           (("lin_l", "lin_edge"), ("edge_attr",)), (("att", "bias"), ("x",))]:
        part = run(frozen, wanted)
        for k, v in part.items():
            absent = k.split(".")[0] in frozen or (k in ("x", "edge_attr") and k not in wanted)
            if absent:
                assert v is None, (frozen, wanted, k)
            else:
                assert torch.equal(v, full[k]), (frozen, wanted, k)


@pytest.mark.parametrize("setup", [_sparse_setup, _dense_setup], ids=["sparse", "dense"])
def test_backward_is_deterministic(setup):
    conv, x, edges, ea, g = setup()
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        xs, eas = x.clone().requires_grad_(), ea.clone().requires_grad_()
        out = conv(xs, edges, eas)
        out.backward(g)
        runs.append([out.detach(), xs.grad, eas.grad] + [p.grad.clone() for p in conv.parameters()])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


_REL_KW = dict(pose_slice=slice(0, 2), time_scale=0.25)


def test_cuda_graph_capture_two_layers_behind_relative_edge_attr():
    """Forward + backward of RelativeEdgeAttr and two GATv2Conv layers on an attached index, captured on one stream and
    replayed: nothing is read on the host, so the replays equal the eager run - also after x and att were changed in
    place between two replays."""
    from gcm import gatv2 as GV, gine as GE
    M, F, H, C = 40, 8, 2, 8
    x0, ei, _ = _sparse_operands((M, 90, F, H, C, None, {"mixed": True}), True)
    es = _with_index(ei, M)
    rel = GE.RelativeEdgeAttr(**_REL_KW)
    torch.manual_seed(14)
    c1 = GV.GATv2Conv(F, C, heads=H, edge_dim=3).to(DEV)
    c2 = GV.GATv2Conv(H * C, C, heads=H, edge_dim=3, fill_value=0.5, share_weights=True).to(DEV)
    params = list(c1.parameters()) + list(c2.parameters())
    x = x0.float().to(DEV).requires_grad_()
    x1 = quant((M, F), 8, 16, torch.Generator().manual_seed(9)).float().to(DEV)
    att0, att1 = c1.att.detach().clone(), torch.randn(1, H, C, device=DEV)
    gout = torch.randn(M, H * C, device=DEV)

    def step():
        ea = rel(x, es)
        out = c2(torch.tanh(c1(x, es, ea)), es, ea)
        out.backward(gout)
        return out

    def eager():
        for p in params + [x]:
            p.grad = None
        out = step().detach().clone()
        return out, [p.grad.clone() for p in params + [x]]

    want, want_g = eager()
    with torch.no_grad():
        c1.att.copy_(att1)
        x.copy_(x1)
    want2, want2_g = eager()
    assert not torch.equal(want, want2)
    with torch.no_grad():
        c1.att.copy_(att0)
        x.copy_(x0.float().to(DEV))

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
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want)
    for a, b in zip([p.grad for p in params + [x]], want_g):
        assert torch.equal(a, b)
    with torch.no_grad():
        c1.att.copy_(att1)
        x.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want2)
    for a, b in zip([p.grad for p in params + [x]], want2_g):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# end to end through the memories.  The observations and the parameters are random here, not quantised: a memory's
# in-degrees (three under TemporalEdge([1,2,4])) make the "mean" loop feature a third, which no quantisation keeps
# exact; a LeakyReLU argument within rounding of 0 has no measurable probability on continuous inputs.
# ---------------------------------------------------------------------------
def _gatv2_layer(cls, F, H, C):
    torch.manual_seed(5)
    return cls(F, C, heads=H, edge_dim=3)


def _obs(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("max_hops", [None, 2])
@pytest.mark.parametrize("stepwise", [False, True], ids=["one-shot", "stepwise"])
def test_sparse_gcm_with_gatv2_stack(stepwise, max_hops):
    from gcm import gatv2 as GV, gine as GE, nn as G
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    B, F, H, C, N = 3, 8, 2, 8, 16
    HC = H * C
    torch.manual_seed(8)
    ref = pyg.Sequential("x, edges, weights", [
        (RelativeEdgeAttrRef(**_REL_KW), "x, edges -> ea"), (_gatv2_layer(GATv2Ref, F, H, C), "x, edges, ea -> x"),
        (pyg.GraphConv(HC, HC), "x, edges -> x"), torch.nn.Tanh()])
    dev = G.Sequential("x, edges, weights", [
        (GE.RelativeEdgeAttr(**_REL_KW), "x, edges -> ea"), (_gatv2_layer(GV.GATv2Conv, F, H, C), "x, edges, ea -> x"),
        (G.GraphConv(HC, HC), "x, edges -> x"), torch.nn.Tanh()])
    dev.load_state_dict(ref.state_dict())
    dev = dev.to(DEV)
    if stepwise:
        calls = [(_obs((B, 6, F), 1), torch.tensor([6, 4, 5])), (_obs((B, 6, F), 2), torch.tensor([3, 6, 1]))]
    else:
        calls = [(_obs((B, 12, F), 3), torch.tensor([12, 7, 9]))]
    gws = [torch.randn(B, x.shape[1], HC, generator=torch.Generator().manual_seed(4)) for x, _ in calls]

    mem = SparseGCM(dev, edge_selectors=TemporalEdge([1, 2, 4]), graph_size=N, max_hops=max_hops)
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
            mx, h = osp.sparse_step(x.to(dt), taus, h, r, graph_size=N, edge_selectors=osp.TemporalEdge([1, 2, 4]),
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


@pytest.mark.parametrize("bridge", [False, True], ids=["dense-twin", "sparse-behind-the-bridge"])
def test_dense_gcm_with_gatv2_stack(bridge):
    """T > N: past the overflow roll."""
    from gcm import gatv2 as GV, gine as GE, nn as G
    from gcm.gcm import DenseGCM, DenseToSparse, SparseToDense
    from gcm.edge_selectors.temporal import TemporalBackedge
    B, F, H, C, N, T = 3, 8, 2, 8, 8, 12
    HC = H * C
    torch.manual_seed(8)
    ref = pyg.Sequential("x, adj, weights, B, N", [
        (RelativeEdgeAttrRef(**_REL_KW), "x, adj -> ea"), (_gatv2_layer(DenseGATv2Ref, F, H, C), "x, adj, ea -> x"),
        (pyg.DenseGraphConv(HC, HC), "x, adj -> x"), torch.nn.Tanh()])
    if bridge:
        dev = G.Sequential("x, adj, weights, B, N", [
            (DenseToSparse(transpose=True), "x, adj -> x_sp, edge_index, batch_idx"),
            (GE.RelativeEdgeAttr(**_REL_KW), "x_sp, edge_index -> ea"),
            (_gatv2_layer(GV.GATv2Conv, F, H, C), "x_sp, edge_index, ea -> x_sp"),
            (G.GraphConv(HC, HC), "x_sp, edge_index -> x_sp"), torch.nn.Tanh(),
            (SparseToDense(), "x_sp, edge_index, batch_idx, B, N -> x, adj"), (lambda x: x, "x -> x")])
        # the same parameters one stage later (the bridge is stage 0)
        names = {k: "module_%d.%s" % (int(k.split(".")[0][7:]) - 1, k.split(".", 1)[1]) for k, _ in dev.named_parameters()}
        assert set(names.values()) == {k for k, _ in ref.named_parameters()}
        with torch.no_grad():
            for k, p in dev.named_parameters():
                p.copy_(dict(ref.named_parameters())[names[k]])
    else:
        dev = G.Sequential("x, adj, weights, B, N", [
            (GE.RelativeEdgeAttr(**_REL_KW), "x, adj -> ea"), (_gatv2_layer(GV.DenseGATv2Conv, F, H, C), "x, adj, ea -> x"),
            (G.DenseGraphConv(HC, HC), "x, adj -> x"), torch.nn.Tanh()])
        dev.load_state_dict(ref.state_dict())
        names = {k: k for k, _ in dev.named_parameters()}
    dev = dev.to(DEV)
    obs = _obs((T, B, F), 11)
    gw = torch.randn(T, B, HC, generator=torch.Generator().manual_seed(12))

    res = {}
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(ref).to(dt)
        want, h = od.dense_rollout(obs.to(dt), None, r, graph_size=N, edge_selectors=od.TemporalBackedge([1, 2]))
        (want * gw.to(dt)).sum().backward()
        res[dt] = (want, h, {k: p.grad for k, p in r.named_parameters()})

    mem = DenseGCM(dev, edge_selectors=TemporalBackedge([1, 2]), graph_size=N)
    hidden, outs = None, []
    for t in range(T):
        mx, hidden = mem(obs[t].to(DEV), hidden)
        outs.append(mx)
    got = torch.stack(outs)
    (got * gw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert_bounded(got, res[torch.float64][0], res[torch.float32][0], "mx")
    assert_bounded(hidden[0], res[torch.float64][1][0], res[torch.float32][1][0], "nodes")
    assert torch.equal(hidden[1].cpu(), res[torch.float32][1][1])
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][names[k]], res[torch.float32][2][names[k]], k, floor=GRAD_FLOOR,
                       relative=True)
