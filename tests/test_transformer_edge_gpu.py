"""gcm.transformer's TransformerConv / DenseTransformerConv kernels (csrc/transformer_edge.hip) against the per-edge
eager restatement (tests/_transformer_edge_restate.py), evaluated in float64 for the bound and in float32 for the
restatement's own error (tests/_gcn_restate.py's rule: 3 x that error, floors 2e-6 for outputs and 5e-7 of the
gradient's scale for gradients).  The kernels compute the factored form; the reference forms lin_edge(edge_attr) per
edge.  Needs an MI355X."""
import copy

import pytest
import torch

from _gcn_restate import assert_bounded
from _gine_restate import RelativeEdgeAttrRef
from _transformer_edge_restate import (DENSE_CASES, SPARSE_CASES, DenseTransformerEdgeRef, TransformerEdgeRef, case_id,
                                       dense_case, layer_kwargs, mp_layer, sparse_case)
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _make(cls, case, seed, **variant):
    """A gcm.transformer layer of the case (torch.nn.Linear's default init, on the CPU) and its arguments."""
    kw = {**layer_kwargs(case), **variant}
    torch.manual_seed(seed)
    return cls(**kw), kw


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
    ref = ref_cls(**kw)
    ref.load_state_dict(conv.state_dict())
    ref = ref.to(dtype)
    ts = {k: t.detach().to(dtype).requires_grad_() for k, t in inputs.items()}
    out = call(ref, **ts)
    out.backward(g.to(dtype))
    grads = {k: t.grad for k, t in ts.items()}
    grads.update(_named_grads(ref))
    return out, grads


def _check(out, got, ref_cls, conv, kw, call, inputs, g):
    """Output and every gradient (x, edge_attr, every parameter - lin_key.bias, whose true value is 0, included)."""
    o64, g64 = _ref_eval(ref_cls, conv, kw, call, inputs, g, torch.float64)
    o32, g32 = _ref_eval(ref_cls, conv, kw, call, inputs, g, torch.float32)
    assert out.shape == o64.shape
    assert not torch.isnan(out).any()
    assert_bounded(out, o64, o32, "out")
    assert set(g64) == set(got), (sorted(g64), sorted(got))
    for name, b64 in g64.items():
        assert b64 is not None and got[name] is not None, name
        assert got[name].shape == b64.shape, name
        assert not torch.isnan(got[name]).any(), name
        assert_bounded(got[name], b64, g32[name], name, floor=GRAD_FLOOR, relative=True)


# ---------------------------------------------------------------------------
# TransformerConv
# ---------------------------------------------------------------------------
def _sparse_operands(case, presorted):
    x, ei, ea = sparse_case(*case)
    if presorted:
        _, perm = torch.sort(ei[1], stable=True)
        ei, ea = ei[:, perm].contiguous(), ea[perm].contiguous()
    return x, ei, ea


def _run_sparse(case, indexed=True, presorted=None, eval_mode=False, **variant):
    from gcm import transformer as T
    M, E, Fi, H, C, D, _ = case
    presorted = indexed if presorted is None else presorted
    x, ei, ea = _sparse_operands(case, presorted)
    conv, kw = _make(T.TransformerConv, case, M + E, **variant)
    Fo = H * C if kw.get("concat", True) else C
    g = torch.randn(M, Fo, generator=torch.Generator().manual_seed(E))
    dconv = copy.deepcopy(conv).to(DEV)
    if eval_mode:
        dconv.eval()
    xd, ead = x.float().to(DEV).requires_grad_(), ea.float().to(DEV).requires_grad_()
    out = dconv(xd, _with_index(ei, M) if indexed else ei.to(DEV), ead)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    got = {"x": xd.grad, "edge_attr": ead.grad, **_named_grads(dconv)}
    _check(out, got, TransformerEdgeRef, conv, kw, lambda ref, x, edge_attr: ref(x, ei, edge_attr),
           {"x": x, "edge_attr": ea}, g)
    return out, got


@pytest.mark.parametrize("indexed", [True, False], ids=["attached-index", "plain-list"])
@pytest.mark.parametrize("case", SPARSE_CASES, ids=case_id)
def test_transformerconv(case, indexed):
    """Output and every gradient; with SparseGCM's attached index (the list in CSR order) and with a plain list in no
    particular order, which the layer indexes itself.  The C values take every lane-group width; each graph has a hub
    of 70 in-edges or more, a node without an in-edge, a loop and a duplicated edge."""
    _run_sparse(case, indexed)


@pytest.mark.parametrize("variant", [dict(beta=True), dict(root_weight=False), dict(bias=False),
                                     dict(dropout=0.5, eval_mode=True), dict(beta=True, concat=False)],
                         ids=["beta", "no-root", "no-bias", "eval-dropout", "beta-mean"])
@pytest.mark.parametrize("case", [SPARSE_CASES[0], SPARSE_CASES[6]], ids=case_id)
def test_transformerconv_variants(case, variant):
    out, _ = _run_sparse(case, **variant)
    if variant.get("root_weight") is False:
        assert not out[-1].any()                                  # no in-edge, no skip: exactly 0


@pytest.mark.parametrize("case", [SPARSE_CASES[0], SPARSE_CASES[5]], ids=case_id)
def test_an_unsorted_list_equals_the_presorted_one_bit_for_bit(case):
    """The csr_perm path: edge_attr stays in the caller's order and is reached through the index's permutation."""
    out_u, got_u = _run_sparse(case, indexed=False, presorted=False)
    out_s, got_s = _run_sparse(case, indexed=True)
    _, perm = torch.sort(sparse_case(*case)[1][1], stable=True)
    assert torch.equal(out_u, out_s)
    for k in got_s:
        a = got_u[k][perm.to(DEV)] if k == "edge_attr" else got_u[k]
        assert torch.equal(a, got_s[k]), k


def test_wide_layers_are_refused_before_any_launch():
    from gcm import transformer as T, _hip
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    ea = torch.randn(2, 3, device=DEV)
    with pytest.raises(ValueError, match="128"):
        T.TransformerConv(130, 4, edge_dim=3).to(DEV)(torch.randn(5, 130, device=DEV), ei, ea)
    with pytest.raises(ValueError, match="128"):
        T.TransformerConv(4, 33, heads=4, edge_dim=3).to(DEV)(torch.randn(5, 4, device=DEV), ei, ea)
    with pytest.raises(ValueError, match="32"):
        T.TransformerConv(4, 4, edge_dim=33).to(DEV)(torch.randn(5, 4, device=DEV), ei, torch.randn(2, 33, device=DEV))
    with pytest.raises(ValueError, match="128"):
        T.DenseTransformerConv(4, 65, heads=2, edge_dim=3).to(DEV)(
            torch.randn(1, 3, 4, device=DEV), torch.ones(1, 3, 3, device=DEV), torch.randn(1, 3, 3, 3, device=DEV))
    t = torch.zeros(64, device=DEV)                               # and by the library itself: a code, not a fault
    p = _hip.ptr(t)
    rc = _hip.lib().gcm_csr_transformer_edge_fwd(*([p] * 11), 0, 2, 1, 4, 1, 4, 33, 1, 1, _hip.stream())
    assert rc == _hip.GCM_EUNSUPPORTED
    rc = _hip.lib().gcm_csr_transformer_edge_fwd(p, None, p, None, None, p, p, p, None, p, p, 0, 2, 1, 4, 1, 4, 3, 1, 1,
                                                 _hip.stream())
    assert rc == _hip.EINVAL


# ---------------------------------------------------------------------------
# DenseTransformerConv
# ---------------------------------------------------------------------------
def _run_dense(case, pattern="band", add_loop=False, weights=None, mask=False, adj_grad=False, form=None, **variant):
    from gcm import transformer as T
    B, N, Fi, H, C, D, _ = case
    x, adj, ea = dense_case(*case, pattern=pattern)
    if form is not None:                                          # one adjacency and edge_attr for the whole batch
        adj, ea = adj[1:2], ea[1:2]
    if form == "two_d":
        x = x[:1]
    m = (torch.rand(B, N, generator=torch.Generator().manual_seed(2)) < 0.7) if mask else None
    conv, kw = _make(T.DenseTransformerConv, case, B + N, **variant)
    Fo = H * C if kw.get("concat", True) else C
    g = torch.randn(x.shape[0], N, Fo, generator=torch.Generator().manual_seed(N))
    dconv = copy.deepcopy(conv).to(DEV)
    on = adj != 0
    if add_loop:
        on = on | torch.eye(N, dtype=torch.bool)
    nan = torch.full((), float("nan"))
    ea_dev = torch.where(on.unsqueeze(-1), ea.float(), nan).to(DEV)          # NaN wherever there is no term
    xd = x.float().to(DEV)
    ad = (adj if weights is None else adj * weights).float().to(DEV)
    if form == "two_d":
        xd, ad, ea_dev = xd[0], ad[0], ea_dev[0]
    xd, ea_dev, ad = xd.requires_grad_(), ea_dev.requires_grad_(), ad.requires_grad_(adj_grad)
    out = dconv(xd, ad, ea_dev, None if m is None else m.to(DEV), add_loop=add_loop)
    out.backward(g.to(DEV).view(out.shape))
    torch.cuda.synchronize()
    assert ad.grad is None
    assert ea_dev.grad.shape == ea_dev.shape                      # written whole, zero where there is no term
    assert not ea_dev.grad.view(-1, N, N, D)[~on.expand(ea_dev.grad.view(-1, N, N, D).shape[0], N, N).to(DEV)].any()
    got = {"x": xd.grad.view(x.shape), "edge_attr": ea_dev.grad.view(ea.shape), **_named_grads(dconv)}
    _check(out.view(x.shape[0], N, Fo), got, DenseTransformerEdgeRef, conv, kw,
           lambda ref, x, edge_attr: ref(x, adj, edge_attr, m, add_loop), {"x": x, "edge_attr": ea}, g)
    return out, got


@pytest.mark.parametrize("add_loop", [False, True], ids=["no-loops", "loops"])
@pytest.mark.parametrize("pattern", ["band", "lower"])
@pytest.mark.parametrize("case", DENSE_CASES, ids=case_id)
def test_dense_transformerconv(case, pattern, add_loop):
    """TemporalBackedge([1,2,4])'s band and the lower triangle, each with an empty row and a full row; NaN in edge_attr
    wherever there is no term.  N = 40: a partial tile; N = 130: five tiles and two row blocks; C = 128, D = 32: both
    limits."""
    _run_dense(case, pattern, add_loop)


@pytest.mark.parametrize("variant", [dict(beta=True), dict(concat=False), dict(root_weight=False), dict(mask=True),
                                     dict(beta=True, concat=False, mask=True, add_loop=True)],
                         ids=["beta", "mean", "no-root", "mask", "beta-mean-mask-loops"])
def test_dense_transformerconv_variants(variant):
    _run_dense(DENSE_CASES[0], **variant)


@pytest.mark.parametrize("form", ["two_d", "broadcast"])
def test_dense_operand_forms(form):
    """[N,F] / [N,N] / [N,N,D] operands, and one adjacency and edge_attr for the whole batch."""
    _run_dense(DENSE_CASES[0], form=form)


def test_an_adjacency_that_requires_grad_gets_none():
    _run_dense(DENSE_CASES[0], adj_grad=True)


def test_only_the_pattern_matters():
    case = DENSE_CASES[0]
    B, N = case[:2]
    gen = torch.Generator().manual_seed(5)
    w = (torch.randint(1, 9, (B, N, N), generator=gen).double() / 8) * (torch.randint(0, 2, (B, N, N), generator=gen) * 2 - 1)
    out_w, got_w = _run_dense(case, weights=w)
    out_1, got_1 = _run_dense(case)
    assert torch.equal(out_w, out_1)
    for k in got_1:
        assert torch.equal(got_w[k], got_1[k]), k


@pytest.mark.parametrize("kw", [dict(), dict(beta=True, concat=False)], ids=["plain", "beta-mean"])
def test_dense_equals_sparse(kw):
    """A {0,1} adjacency through DenseTransformerConv, and through TransformerConv on DenseToSparse(transpose=True)'s
    list with edge_attr[b,i,j] gathered in that order: each within its bound of the same float64 restatement."""
    from gcm import transformer as T
    from gcm.gcm import DenseToSparse
    case = DENSE_CASES[0]
    B, N, Fi, H, C, D, _ = case
    x, adj, ea = dense_case(*case, pattern="lower")
    conv, kw = _make(T.DenseTransformerConv, case, 3, **kw)
    Fo = H * C if kw.get("concat", True) else C
    g = torch.randn(B, N, Fo, generator=torch.Generator().manual_seed(7))
    dconv = copy.deepcopy(conv).to(DEV)
    sconv = T.TransformerConv(**kw).to(DEV)
    sconv.load_state_dict(dconv.state_dict())
    ad = adj.float().to(DEV)
    xa, xb = x.float().to(DEV).requires_grad_(), x.float().to(DEV).requires_grad_()
    ea_a, ea_b = ea.float().to(DEV).requires_grad_(), ea.float().to(DEV).requires_grad_()
    out_d = dconv(xa, ad, ea_a)
    x_sp, ei, _ = DenseToSparse(transpose=True)(xb, ad)
    bb, ii, jj = ad.nonzero(as_tuple=True)                        # the list's order: (b, row, column)
    assert torch.equal(ei, torch.stack([bb * N + jj, bb * N + ii]))
    out_s = sconv(x_sp, ei, ea_b[bb, ii, jj]).view(B, N, Fo)
    out_d.backward(g.to(DEV))
    out_s.backward(g.to(DEV))
    torch.cuda.synchronize()
    off = (adj == 0).unsqueeze(-1)
    for out, xg, eg, c in ((out_d, xa.grad, ea_a.grad, dconv), (out_s, xb.grad, ea_b.grad, sconv)):
        got = {"x": xg, "edge_attr": eg, **_named_grads(c)}
        _check(out, got, DenseTransformerEdgeRef, conv, kw, lambda ref, x, edge_attr: ref(x, adj, edge_attr),
               {"x": x, "edge_attr": ea}, g)
        assert not eg[off.expand_as(eg).to(DEV)].any()


# ---------------------------------------------------------------------------
# edge_dim=None is gcm.nn's layer; a zero lin_edge is the edge-free layer
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(beta=True, concat=False)], ids=["plain", "beta-mean"])
def test_without_edge_dim_the_layers_are_gcm_nn_s_bit_for_bit(kw):
    from gcm import nn as G, transformer as T
    case = SPARSE_CASES[0]
    M, E, Fi, H, C, D, _ = case
    x, ei, ea = _sparse_operands(case, True)
    xd, adj, _ = dense_case(3, 40, Fi, H, C, D)
    g = torch.Generator().manual_seed(1)
    for mine, theirs, args in ((T.TransformerConv, G.TransformerConv, (x.float().to(DEV), _with_index(ei, M), ea.float().to(DEV))),
                               (T.DenseTransformerConv, G.DenseTransformerConv, (xd.float().to(DEV), adj.float().to(DEV)))):
        torch.manual_seed(2)
        a = mine(Fi, C, heads=H, **kw).to(DEV)
        b = theirs(Fi, C, heads=H, **kw).to(DEV)
        b.load_state_dict(a.state_dict())
        res = []
        for conv in (a, b):
            xs = args[0].clone().requires_grad_()
            out = conv(xs, *args[1:])
            gout = torch.randn(out.shape, generator=g.manual_seed(1)).to(DEV)
            out.backward(gout)
            res.append([out.detach(), xs.grad] + [p.grad for _, p in sorted(conv.named_parameters())])
        torch.cuda.synchronize()
        for u, v in zip(*res):
            assert torch.equal(u, v)


def test_with_a_zero_lin_edge_it_is_the_edge_free_layer():
    from gcm import nn as G, transformer as T
    from _transformer_restate import DenseTransformerRef, TransformerRef
    case = SPARSE_CASES[0]
    M, E, Fi, H, C, D, _ = case
    x, ei, ea = _sparse_operands(case, True)
    xd, adj, ead = dense_case(3, 40, Fi, H, C, D)
    for cls, ref_cls, args, rargs in (
            (T.TransformerConv, TransformerRef, (x, _with_index(ei, M), ea), (x, ei)),
            (T.DenseTransformerConv, DenseTransformerRef, (xd, adj, ead), (xd, adj))):
        torch.manual_seed(3)
        conv = cls(Fi, C, heads=H, edge_dim=D)
        with torch.no_grad():
            conv.lin_edge.weight.zero_()
        sd = {k: v for k, v in conv.state_dict().items() if not k.startswith("lin_edge")}
        refs = {}
        for dt in (torch.float64, torch.float32):
            ref = ref_cls(Fi, C, heads=H)
            ref.load_state_dict(sd)
            refs[dt] = ref.to(dt)(*[t.to(dt) if t.is_floating_point() else t for t in rargs]).detach()
        out = conv.to(DEV)(*[t.float().to(DEV) if t.is_floating_point() else t for t in args])
        assert_bounded(out, refs[torch.float64], refs[torch.float32], cls.__name__)


# ---------------------------------------------------------------------------
# subsets of wanted gradients, determinism, capture
# ---------------------------------------------------------------------------
def _sparse_setup():
    from gcm import transformer as T
    case = SPARSE_CASES[0]
    x, ei, ea = _sparse_operands(case, True)
    conv, kw = _make(T.TransformerConv, case, 1, beta=True)
    return (conv.to(DEV), x.float().to(DEV), _with_index(ei, case[0]), ea.float().to(DEV),
            torch.randn(case[0], case[3] * case[4], device=DEV))


def _dense_setup():
    from gcm import transformer as T
    case = DENSE_CASES[0]
    x, adj, ea = dense_case(*case)
    conv, kw = _make(T.DenseTransformerConv, case, 2, beta=True)
    return (conv.to(DEV), x.float().to(DEV), adj.float().to(DEV), ea.float().to(DEV),
            torch.randn(case[0], case[1], case[3] * case[4], device=DEV))


@pytest.mark.parametrize("setup", [_sparse_setup, _dense_setup], ids=["sparse", "dense"])
def test_subsets_of_wanted_gradients(setup):
    """Each gradient is computed only when wanted, and then equals the full run's bit for bit."""
    conv, x, edges, ea, g = setup()
    groups = {k: list(getattr(conv, k).parameters())
              for k in ("lin_key", "lin_query", "lin_value", "lin_edge", "lin_skip", "lin_beta")}
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
    for frozen, wanted in [(("lin_edge",), ("x", "edge_attr")), (every, ("x", "edge_attr")), (every, ("x",)),
                           (every, ("edge_attr",)), (tuple(k for k in every if k != "lin_edge"), ()),
                           (("lin_key", "lin_query", "lin_value", "lin_skip"), ("edge_attr",)),
                           (("lin_beta", "lin_edge"), ("x",))]:
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
    """Forward + backward of RelativeEdgeAttr and two TransformerConv layers on an attached index, captured on one
    stream and replayed: nothing is read on the host, so the replays equal the eager run - also after x and a weight
    were changed in place between two replays."""
    from gcm import gine as GE, transformer as T
    M, F, H, C = 40, 8, 2, 8
    x0, ei, _ = _sparse_operands(SPARSE_CASES[0], True)
    es = _with_index(ei, M)
    rel = GE.RelativeEdgeAttr(**_REL_KW)
    torch.manual_seed(14)
    c1 = T.TransformerConv(F, C, heads=H, edge_dim=3).to(DEV)
    c2 = T.TransformerConv(H * C, C, heads=H, edge_dim=3, beta=True).to(DEV)
    params = list(c1.parameters()) + list(c2.parameters())
    x = x0.float().to(DEV).requires_grad_()
    x1 = torch.randn(M, F, generator=torch.Generator().manual_seed(9)).to(DEV)
    w0, w1 = c1.lin_edge.weight.detach().clone(), torch.randn(H * C, 3, device=DEV)
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
        c1.lin_edge.weight.copy_(w1)
        x.copy_(x1)
    want2, want2_g = eager()
    assert not torch.equal(want, want2)
    with torch.no_grad():
        c1.lin_edge.weight.copy_(w0)
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
        c1.lin_edge.weight.copy_(w1)
        x.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want2)
    for a, b in zip([p.grad for p in params + [x]], want2_g):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# nothing per edge of width H*C exists
# ---------------------------------------------------------------------------
def test_no_per_edge_array_of_width_hc_is_allocated():
    """M = 2048, E = 65 536, H*C = 128, D = 3: forward + backward of the fused layer allocates less than one
    [E, H*C] float array at its peak; the same layer on gcm.nn.MessagePassing, which forms lin_edge(edge_attr), the
    keys and the messages per edge, allocates more - so the measurement can tell the two apart."""
    from gcm import nn as G, transformer as T
    from gcm.graph_utils import softmax
    M, E, F, H, C, D = 2048, 65536, 32, 4, 32, 3
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(M, F, generator=gen).to(DEV)
    ei = torch.stack([torch.randint(0, M, (E,), generator=gen), torch.randint(0, M, (E,), generator=gen).sort()[0]])
    es = _with_index(ei, M)
    ea = torch.randn(E, D, generator=gen).to(DEV)
    gout = torch.randn(M, H * C, generator=gen).to(DEV)
    cap = E * H * C * 4
    torch.manual_seed(0)
    fused = T.TransformerConv(F, C, heads=H, edge_dim=D).to(DEV)
    unfused = mp_layer(G.MessagePassing, softmax)(F, C, heads=H, edge_dim=D).to(DEV)

    def peak(conv):
        def call():
            conv.zero_grad(set_to_none=True)
            xs, eas = x.clone().requires_grad_(), ea.clone().requires_grad_()
            conv(xs, es, eas).backward(gout)
        call()                                                    # warm-up: the index's CSC view, the allocator
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        call()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    got, base = peak(fused), peak(unfused)
    print(f"peak bytes over the call: fused {got}, on MessagePassing {base}, one [E,H*C] array {cap}")
    assert got < cap
    assert base > cap


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
def _layer(cls, F, H, C):
    torch.manual_seed(5)
    return cls(F, C, heads=H, edge_dim=3)


def _obs(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("max_hops", [None, 2])
@pytest.mark.parametrize("stepwise", [False, True], ids=["one-shot", "stepwise"])
def test_sparse_gcm_with_transformer_stack(stepwise, max_hops):
    from gcm import gine as GE, nn as G, transformer as T
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    B, F, H, C, N = 3, 8, 2, 8, 16
    HC = H * C
    torch.manual_seed(8)
    ref = pyg.Sequential("x, edges, weights", [
        (RelativeEdgeAttrRef(**_REL_KW), "x, edges -> ea"), (_layer(TransformerEdgeRef, F, H, C), "x, edges, ea -> x"),
        (pyg.GraphConv(HC, HC), "x, edges -> x"), torch.nn.Tanh()])
    dev = G.Sequential("x, edges, weights", [
        (GE.RelativeEdgeAttr(**_REL_KW), "x, edges -> ea"), (_layer(T.TransformerConv, F, H, C), "x, edges, ea -> x"),
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
def test_dense_gcm_with_transformer_stack(bridge):
    """T > N: past the overflow roll."""
    from gcm import gine as GE, nn as G, transformer as T
    from gcm.gcm import DenseGCM, DenseToSparse, SparseToDense
    from gcm.edge_selectors.temporal import TemporalBackedge
    B, F, H, C, N, TT = 3, 8, 2, 8, 8, 12
    HC = H * C
    torch.manual_seed(8)
    ref = pyg.Sequential("x, adj, weights, B, N", [
        (RelativeEdgeAttrRef(**_REL_KW), "x, adj -> ea"), (_layer(DenseTransformerEdgeRef, F, H, C), "x, adj, ea -> x"),
        (pyg.DenseGraphConv(HC, HC), "x, adj -> x"), torch.nn.Tanh()])
    if bridge:
        dev = G.Sequential("x, adj, weights, B, N", [
            (DenseToSparse(transpose=True), "x, adj -> x_sp, edge_index, batch_idx"),
            (GE.RelativeEdgeAttr(**_REL_KW), "x_sp, edge_index -> ea"),
            (_layer(T.TransformerConv, F, H, C), "x_sp, edge_index, ea -> x_sp"),
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
            (GE.RelativeEdgeAttr(**_REL_KW), "x, adj -> ea"), (_layer(T.DenseTransformerConv, F, H, C), "x, adj, ea -> x"),
            (G.DenseGraphConv(HC, HC), "x, adj -> x"), torch.nn.Tanh()])
        dev.load_state_dict(ref.state_dict())
        names = {k: k for k, _ in dev.named_parameters()}
    dev = dev.to(DEV)
    obs = _obs((TT, B, F), 11)
    gw = torch.randn(TT, B, HC, generator=torch.Generator().manual_seed(12))

    res = {}
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(ref).to(dt)
        want, h = od.dense_rollout(obs.to(dt), None, r, graph_size=N, edge_selectors=od.TemporalBackedge([1, 2]))
        (want * gw.to(dt)).sum().backward()
        res[dt] = (want, h, {k: p.grad for k, p in r.named_parameters()})

    mem = DenseGCM(dev, edge_selectors=TemporalBackedge([1, 2]), graph_size=N)
    hidden, outs = None, []
    for t in range(TT):
        mx, hidden = mem(obs[t].to(DEV), hidden)
        outs.append(mx)
    got = torch.stack(outs)
    (got * gw.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert_bounded(got, res[torch.float64][0], res[torch.float32][0], "mx")
    assert_bounded(hidden[0], res[torch.float64][1][0], res[torch.float32][1][0], "nodes")
    assert torch.equal(hidden[1].cpu(), res[torch.float32][1][1])
    assert torch.equal(hidden[3].cpu(), res[torch.float32][1][3])
    for k, p in dev.named_parameters():
        assert_bounded(p.grad, res[torch.float64][2][names[k]], res[torch.float32][2][names[k]], k, floor=GRAD_FLOOR,
                       relative=True)
