"""GINEConv / DenseGINEConv / RelativeEdgeAttr kernels against the eager restatement (tests/_gine_restate.py),
evaluated in float64 for the bound and in float32 for the restatement's own error (tests/_gcn_restate.py's rule).  The
inputs are quantised so that no ReLU argument sits on the kink (tests/test_gine_cpu.py checks the construction).
Needs an MI355X."""
import copy

import pytest
import torch

from _gcn_restate import assert_bounded
from _gine_restate import (DENSE_CASES, SPARSE_CASES, DenseGINERef, GINERef, RelativeEdgeAttrRef, dense_case,
                           dense_gine, dense_rel_edge_attr, gine, quant, quant_lin, rel_edge_attr, sparse_case)
from oracle import dense as od, pyg, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)
KINDS = [("identity", 0.3), ("mlp", 0.2), ("mlp", -1.0)]
KIND_IDS = ["identity", "mlp", "mlp-eps-1"]


class _Identity(torch.nn.Identity):
    """The aggregation alone, and something for `lin` to read its width from."""

    def __init__(self, in_features):
        super().__init__()
        self.in_features = in_features


def _nn(kind, cin, cout):
    if kind == "identity":
        return _Identity(cin)
    return torch.nn.Sequential(torch.nn.Linear(cin, 2 * cout), torch.nn.Tanh(), torch.nn.Linear(2 * cout, cout))


def _make(cls, kind, F, D, eps, seed):
    """A layer with random nn and eps and a quantised lin."""
    torch.manual_seed(seed)
    Fo = F if kind == "identity" else max(3, F // 2)
    nn = _nn(kind, F, Fo)
    conv = cls(nn, eps=eps, train_eps=True, edge_dim=D)
    if D is not None:
        quant_lin(conv.lin, torch.Generator().manual_seed(seed))
    return conv, Fo


def _with_index(ei, M, mask=None):
    """The edge list (already in CSR order) on the device with a ready index attached, as SparseGCM hands it over."""
    from gcm import _ops
    es = ei.contiguous().to(DEV)
    es.gcm_graph = _ops.GraphIndex(es, _ops.ptr_from_sorted(es[1].contiguous(), M), M, mask=mask)
    return es


def _named_grads(conv):
    return {k: p.grad for k, p in conv.named_parameters()}


def _ref_eval(ref_cls, conv, call, inputs, g, dtype):
    """The restated module with conv's state in dtype -> (out, {name: gradient})."""
    ref = ref_cls(copy.deepcopy(conv.nn), conv.initial_eps, True, conv.edge_dim)
    ref.load_state_dict(conv.state_dict())
    ref = ref.to(dtype)
    ts = {k: t.detach().to(dtype).requires_grad_(req) for k, (t, req) in inputs.items()}
    out = call(ref, **ts)
    out.backward(g.to(dtype))
    grads = {k: t.grad for k, t in ts.items() if t.requires_grad}
    grads.update(_named_grads(ref))
    return out, grads


def _check(out, got, ref_cls, conv, call, inputs, g):
    o64, g64 = _ref_eval(ref_cls, conv, call, inputs, g, torch.float64)
    o32, g32 = _ref_eval(ref_cls, conv, call, inputs, g, torch.float32)
    assert out.shape == o64.shape
    assert not torch.isnan(out).any()
    assert_bounded(out, o64, o32, "out")
    assert set(g64) <= set(got), (sorted(g64), sorted(got))
    for name, b64 in g64.items():
        if b64 is None:                                       # unused by the restatement (eps without add_loop)
            continue
        assert got[name] is not None, name
        assert not torch.isnan(got[name]).any(), name
        assert_bounded(got[name], b64, g32[name], name, floor=GRAD_FLOOR, relative=True)


# ---------------------------------------------------------------------------
# GINEConv
# ---------------------------------------------------------------------------
def _sorted_case(case):
    x, ei, ea = sparse_case(*case)
    _, perm = torch.sort(ei[1], stable=True)
    return x, ei[:, perm].contiguous(), ea[perm].contiguous()


def _run_sparse(case, kind, eps, presorted=True):
    from gcm import gine as GE
    M, E, F, D = case
    x, ei, ea = _sorted_case(case) if presorted else sparse_case(*case)
    conv, Fo = _make(GE.GINEConv, kind, F, D, eps, seed=M + E + F)
    g = torch.randn(M, Fo, generator=torch.Generator().manual_seed(E))
    dconv = copy.deepcopy(conv).to(DEV)
    xd, ead = x.float().to(DEV).requires_grad_(), ea.float().to(DEV).requires_grad_()
    out = dconv(xd, _with_index(ei, M) if presorted else ei.to(DEV), ead)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    got = {"x": xd.grad, "edge_attr": ead.grad, **_named_grads(dconv)}
    _check(out, got, GINERef, conv, lambda ref, x, edge_attr: ref(x, ei, edge_attr),
           {"x": (x, True), "edge_attr": (ea, True)}, g)
    return out, got


@pytest.mark.parametrize("kind,eps", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("case", SPARSE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_gineconv(case, kind, eps):
    _run_sparse(case, kind, eps)


def test_gineconv_unsorted_list_equals_presorted_bit_for_bit():
    """The csr_perm path: edge_attr stays in the caller's order and is reached through the index's permutation."""
    case = (40, 90, 8, 5)
    out_u, got_u = _run_sparse(case, "mlp", 0.2, presorted=False)
    out_s, got_s = _run_sparse(case, "mlp", 0.2, presorted=True)
    _, perm = torch.sort(sparse_case(*case)[1][1], stable=True)
    assert torch.equal(out_u, out_s)
    for k in got_s:
        a = got_u[k][perm.to(DEV)] if k == "edge_attr" else got_u[k]
        assert torch.equal(a, got_s[k]), k


def test_gineconv_rejects_a_masked_index():
    from gcm import gine as GE
    M = 10
    _, ei, _ = _sorted_case((M, 20, 4, None))
    es = _with_index(ei, M, mask=torch.ones(M, dtype=torch.bool, device=DEV))
    conv = GE.GINEConv(torch.nn.Identity()).to(DEV)
    with pytest.raises(ValueError, match="masked GraphIndex"):
        conv(torch.randn(M, 4, device=DEV), es, torch.randn(20, 4, device=DEV))


def test_wide_layers_are_refused_before_any_launch():
    from gcm import gine as GE
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    with pytest.raises(ValueError, match="128"):
        GE.GINEConv(torch.nn.Identity()).to(DEV)(torch.randn(5, 130, device=DEV), ei, torch.randn(2, 130, device=DEV))
    with pytest.raises(ValueError, match="32"):
        GE.GINEConv(torch.nn.Linear(4, 4), edge_dim=33).to(DEV)(torch.randn(5, 4, device=DEV), ei,
                                                              torch.randn(2, 33, device=DEV))
    with pytest.raises(ValueError, match="128"):
        GE.DenseGINEConv(torch.nn.Identity()).to(DEV)(torch.randn(1, 3, 130, device=DEV), torch.ones(1, 3, 3, device=DEV),
                                                     torch.randn(1, 3, 3, 130, device=DEV))


# ---------------------------------------------------------------------------
# DenseGINEConv
# ---------------------------------------------------------------------------
def _run_dense(case, kind, eps, adj_grad):
    from gcm import gine as GE
    B, N, F, D, opts = case
    add_loop = opts.get("add_loop", True)
    x, adj, ea, mask = dense_case(*case)
    conv, Fo = _make(GE.DenseGINEConv, kind, F, D, eps, seed=B + N + F)
    g = torch.randn(B, N, Fo, generator=torch.Generator().manual_seed(N))
    dconv = copy.deepcopy(conv).to(DEV)
    ea_dev = ea.float()
    if not adj_grad:                                          # the unset entries are not read
        ea_dev = torch.where((adj != 0).unsqueeze(-1), ea_dev, torch.full((), float("nan")))
    xd, ead = x.float().to(DEV).requires_grad_(), ea_dev.to(DEV).requires_grad_()
    ad = adj.float().to(DEV).requires_grad_(adj_grad)
    out = dconv(xd, ad, ead, None if mask is None else mask.to(DEV), add_loop=add_loop)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    got = {"x": xd.grad, "edge_attr": ead.grad, "adj": ad.grad, **_named_grads(dconv)}
    if not add_loop:                                          # eps is not used: its gradient is exactly zero
        assert got["eps"] is None or float(got["eps"].abs().max()) == 0.0
    assert ead.grad.shape == ead.shape
    assert not ead.grad[(ad.detach() == 0).expand_as(ead[..., 0])].any()                  # zero where unset
    _check(out, got, DenseGINERef, conv,
           lambda ref, x, adj, edge_attr: ref(x, adj, edge_attr, mask, add_loop).view(out.shape),
           {"x": (x, True), "adj": (adj, adj_grad), "edge_attr": (ea, True)}, g.view(out.shape))


@pytest.mark.parametrize("adj_grad", [False, True], ids=["pattern", "adj-grad"])
@pytest.mark.parametrize("kind,eps", KINDS[:2], ids=KIND_IDS[:2])
@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: "-".join(map(str, c[:4])))
def test_dense_gineconv(case, kind, eps, adj_grad):
    _run_dense(case, kind, eps, adj_grad)


def test_dense_equals_sparse():
    """A {0,1} adjacency through DenseGINEConv, and through GINEConv on DenseToSparse(transpose=True)'s list, with
    shared weights: each against the same float64 restatement.  Also the no-lin form of the dense twin."""
    from gcm import gine as GE
    from gcm.gcm import DenseToSparse
    B, N, F, D = 3, 40, 8, 3
    gen = torch.Generator().manual_seed(7)
    adj = (torch.rand(B, N, N, generator=gen) < 0.25).double()
    x, ea = quant((B, N, F), 8, 16, gen), quant((B, N, N, D), 4, 8, gen)
    conv, Fo = _make(GE.DenseGINEConv, "mlp", F, D, 0.3, seed=3)
    g = torch.randn(B, N, Fo, generator=gen)
    dconv = copy.deepcopy(conv).to(DEV)
    sconv = GE.GINEConv(copy.deepcopy(conv.nn), train_eps=True, edge_dim=D).to(DEV)
    sconv.load_state_dict(dconv.state_dict())
    ad = adj.float().to(DEV)
    xa, xb = x.float().to(DEV).requires_grad_(), x.float().to(DEV).requires_grad_()
    ea_a, ea_b = ea.float().to(DEV).requires_grad_(), ea.float().to(DEV).requires_grad_()
    out_d = dconv(xa, ad, ea_a)
    x_sp, ei, _ = DenseToSparse(transpose=True)(xb, ad)
    bb, ii, jj = ad.nonzero(as_tuple=True)                    # the list's order: (b, row, column)
    assert torch.equal(ei, torch.stack([bb * N + jj, bb * N + ii]))
    out_s = sconv(x_sp, ei, ea_b[bb, ii, jj]).view(B, N, Fo)
    out_d.backward(g.to(DEV))
    out_s.backward(g.to(DEV))
    torch.cuda.synchronize()
    for out, xg, eg, c in ((out_d, xa.grad, ea_a.grad, dconv), (out_s, xb.grad, ea_b.grad, sconv)):
        got = {"x": xg, "edge_attr": eg, **_named_grads(c)}
        _check(out, got, DenseGINERef, conv, lambda ref, x, edge_attr: ref(x, adj.to(x.dtype), edge_attr),
               {"x": (x, True), "edge_attr": (ea, True)}, g)
    # without lin: edge_attr [B,N,N,F] in eighths + 1/16
    ea = quant((B, N, N, F), 8, 16, gen, 1 / 16)
    conv, Fo = _make(GE.DenseGINEConv, "mlp", F, None, 0.3, seed=4)
    dconv = copy.deepcopy(conv).to(DEV)
    xa, ea_a = x.float().to(DEV).requires_grad_(), ea.float().to(DEV).requires_grad_()
    out = dconv(xa, ad, ea_a)
    out.backward(g.to(DEV))
    torch.cuda.synchronize()
    _check(out, {"x": xa.grad, "edge_attr": ea_a.grad, **_named_grads(dconv)}, DenseGINERef, conv,
           lambda ref, x, edge_attr: ref(x, adj.to(x.dtype), edge_attr), {"x": (x, True), "edge_attr": (ea, True)}, g)


# ---------------------------------------------------------------------------
# RelativeEdgeAttr
# ---------------------------------------------------------------------------
_REL = [dict(time=True), dict(time=False, pose_slice=slice(1, 4)), dict(time=False, pose_slice=slice(-2, None)),
        dict(time=True, pose_slice=slice(1, 4), time_scale=0.25)]


def _bounded_grad(got, make, x, g):
    res = {}
    for dt in (torch.float64, torch.float32):
        xr = x.detach().clone().to(dt).requires_grad_()
        make(xr).backward(g.to(dt))
        res[dt] = xr.grad
    assert_bounded(got, res[torch.float64], res[torch.float32], "x.grad", floor=GRAD_FLOOR, relative=True)


@pytest.mark.parametrize("kw", _REL, ids=["time", "pose", "pose-negative", "both-scaled"])
def test_relative_edge_attr_sparse(kw):
    from gcm import gine as GE
    M, E, F = 40, 90, 6
    x, ei, _ = sparse_case(M, E, F, None)
    mod = GE.RelativeEdgeAttr(**kw)
    want = rel_edge_attr(x, ei, **kw)
    assert want.shape == (E, mod.out_channels)
    xd = x.float().to(DEV).requires_grad_()
    got = mod(xd, ei.to(DEV))
    assert torch.equal(got.cpu(), want.float())               # exact on eighth-quantised x
    # the attached index (the list in CSR order) gives the same rows
    _, perm = torch.sort(ei[1], stable=True)
    got_sorted = mod(xd, _with_index(ei[:, perm], M))
    assert torch.equal(got_sorted, got[perm.to(DEV)])
    if kw.get("pose_slice") is None:
        assert not got.requires_grad
        return
    g = torch.randn(E, mod.out_channels, generator=torch.Generator().manual_seed(1))
    (got * g.to(DEV)).sum().backward()
    g_plain = xd.grad.clone()
    _bounded_grad(g_plain, lambda xr: rel_edge_attr(xr, ei, **kw), x, g)
    xd.grad = None
    (got_sorted * g[perm].to(DEV)).sum().backward()
    _bounded_grad(xd.grad, lambda xr: rel_edge_attr(xr, ei, **kw), x, g)
    assert float(xd.grad[:, :1].abs().max()) == 0.0 or kw["pose_slice"].start == 0      # outside the pose: zero


@pytest.mark.parametrize("kw", _REL, ids=["time", "pose", "pose-negative", "both-scaled"])
def test_relative_edge_attr_dense(kw):
    from gcm import gine as GE
    B, N, F = 3, 33, 6
    x = quant((B, N, F), 8, 16, torch.Generator().manual_seed(2))
    mod = GE.RelativeEdgeAttr(**kw)
    want = dense_rel_edge_attr(x, **kw)
    xd = x.float().to(DEV).requires_grad_()
    got = mod(xd, torch.zeros(B, N, N, device=DEV))
    assert got.shape == (B, N, N, mod.out_channels) and torch.equal(got.cpu(), want.float())
    assert torch.equal(mod(xd[0], torch.zeros(N, N, device=DEV)), got[:1])               # 2-D operands
    if kw.get("pose_slice") is None:
        assert not got.requires_grad
        return
    g = torch.randn(B, N, N, mod.out_channels, generator=torch.Generator().manual_seed(3))
    got.backward(g.to(DEV))
    _bounded_grad(xd.grad, lambda xr: dense_rel_edge_attr(xr, **kw), x, g)


def test_relative_edge_attr_on_sparse_gcm_index():
    """The list SparseGCM builds (TemporalEdge, attached index, batches) against the same list indexed here."""
    from gcm import _ops, gine as GE
    B, n, F = 3, 7, 6
    M = B * n
    src, dst = [], []
    for b in range(B):
        for t in range(n):
            for h in (1, 2, 4):
                if t - h >= 0:
                    src.append(b * n + t - h), dst.append(b * n + t)
    ei = torch.tensor([src, dst])
    x = quant((M, F), 8, 16, torch.Generator().manual_seed(4))
    mod = GE.RelativeEdgeAttr(pose_slice=slice(0, 2), time_scale=0.25)
    es = ei.to(DEV)
    off = torch.arange(B + 1, device=DEV) * n
    es.gcm_graph = _ops.GraphIndex(es, _ops.ptr_from_sorted(es[1].contiguous(), M), M, batches=(off, B, n))
    g = torch.randn(ei.shape[1], 3, generator=torch.Generator().manual_seed(5)).to(DEV)
    grads = []
    for edges in (es, ei.to(DEV)):
        xd = x.float().to(DEV).requires_grad_()
        out = mod(xd, edges)
        assert torch.equal(out.cpu(), rel_edge_attr(x, ei, True, slice(0, 2), 0.25).float())
        assert set(out[:, 0].tolist()) == {0.25, 0.5, 1.0}    # the time gap in steps, scaled
        out.backward(g)
        grads.append(xd.grad)
    assert torch.equal(grads[0], grads[1])


# ---------------------------------------------------------------------------
# subsets of wanted gradients, determinism, capture
# ---------------------------------------------------------------------------
def _sparse_setup(seed=0):
    from gcm import gine as GE
    case = (33, 200, 32, 4)
    x, ei, ea = _sorted_case(case)
    conv, Fo = _make(GE.GINEConv, "mlp", 32, 4, 0.2, seed=seed)
    return conv.to(DEV), x.float().to(DEV), _with_index(ei, 33), ea.float().to(DEV), torch.randn(33, Fo, device=DEV)


def _dense_setup(seed=0):
    from gcm import gine as GE
    case = (2, 40, 16, 4, {"weighted": True})
    x, adj, ea, _ = dense_case(*case)
    conv, Fo = _make(GE.DenseGINEConv, "mlp", 16, 4, 0.2, seed=seed)
    return conv.to(DEV), x.float().to(DEV), adj.float().to(DEV), ea.float().to(DEV), torch.randn(2, 40, Fo, device=DEV)


@pytest.mark.parametrize("setup", [_sparse_setup, _dense_setup], ids=["sparse", "dense"])
def test_subsets_of_wanted_gradients(setup):
    conv, x, edges, ea, g = setup()
    groups = {"eps": [conv.eps], "lin": list(conv.lin.parameters()), "nn": list(conv.nn.parameters())}

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
    for frozen, wanted in [(("eps",), ("x", "edge_attr")), (("lin",), ("x", "edge_attr")), (("nn",), ("x", "edge_attr")),
                           ((), ("x",)), ((), ("edge_attr",)), (("eps", "lin"), ()), (("lin", "nn"), ("x",))]:
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
    dense = edges.dtype == torch.float32
    runs = []
    for _ in range(2):
        conv.zero_grad(set_to_none=True)
        xs, eas = x.clone().requires_grad_(), ea.clone().requires_grad_()
        es = edges.clone().requires_grad_() if dense else edges
        out = conv(xs, es, eas)
        out.backward(g)
        runs.append([out.detach(), xs.grad, eas.grad] + ([es.grad] if dense else [])
                    + [p.grad.clone() for p in conv.parameters()])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_cuda_graph_capture_two_layers_behind_relative_edge_attr():
    """Forward + backward of RelativeEdgeAttr and two GINEConv layers on an attached index, captured on one stream and
    replayed: eps is read on the device, so the replays equal the eager run - also after x and eps were changed in
    place between two replays."""
    from gcm import gine as GE
    M, F, H = 40, 8, 16
    x0, ei, _ = _sorted_case((M, 90, F, None))
    es = _with_index(ei, M)
    rel = GE.RelativeEdgeAttr(pose_slice=slice(0, 2), time_scale=0.25)
    torch.manual_seed(14)
    c1 = GE.GINEConv(_nn("mlp", F, H), eps=0.2, train_eps=True, edge_dim=3).to(DEV)
    c2 = GE.GINEConv(_nn("mlp", H, H), eps=-0.1, train_eps=True, edge_dim=3).to(DEV)
    params = list(c1.parameters()) + list(c2.parameters())
    x = x0.float().to(DEV).requires_grad_()
    x1 = quant((M, F), 8, 16, torch.Generator().manual_seed(9)).float().to(DEV)
    gout = torch.randn(M, H, device=DEV)

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
        c1.eps.fill_(0.7)
        x.copy_(x1)
    want2, want2_g = eager()
    assert not torch.equal(want, want2)
    with torch.no_grad():
        c1.eps.fill_(0.2)
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
        c1.eps.fill_(0.7)
        x.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want2)
    for a, b in zip([p.grad for p in params + [x]], want2_g):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# end to end through the memories
# ---------------------------------------------------------------------------
_REL_KW = dict(pose_slice=slice(0, 2), time_scale=0.25)


def _gine_layer(cls, F, H):
    torch.manual_seed(5)
    conv = cls(torch.nn.Sequential(torch.nn.Linear(F, H), torch.nn.Tanh()), eps=0.1, train_eps=True, edge_dim=3)
    quant_lin(conv.lin, torch.Generator().manual_seed(6), half_cols=(1, 2))   # the pose offsets are in eighths
    return conv


def _sparse_pair(F, H):
    from gcm import gine as GE, nn as G
    torch.manual_seed(8)
    ref = pyg.Sequential("x, edges, weights", [
        (RelativeEdgeAttrRef(**_REL_KW), "x, edges -> ea"), (_gine_layer(GINERef, F, H), "x, edges, ea -> x"),
        (pyg.GraphConv(H, H), "x, edges -> x"), torch.nn.Tanh()])
    dev = G.Sequential("x, edges, weights", [
        (GE.RelativeEdgeAttr(**_REL_KW), "x, edges -> ea"), (_gine_layer(GE.GINEConv, F, H), "x, edges, ea -> x"),
        (G.GraphConv(H, H), "x, edges -> x"), torch.nn.Tanh()])
    dev.load_state_dict(ref.state_dict())
    return ref, dev.to(DEV)


def _obs(shape, seed):
    return quant(shape, 8, 16, torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("max_hops", [None, 2])
@pytest.mark.parametrize("stepwise", [False, True], ids=["one-shot", "stepwise"])
def test_sparse_gcm_with_gine_stack(stepwise, max_hops):
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    B, F, H, N = 3, 8, 16, 16
    ref, dev = _sparse_pair(F, H)
    if stepwise:
        calls = [(_obs((B, 6, F), 1), torch.tensor([6, 4, 5])), (_obs((B, 6, F), 2), torch.tensor([3, 6, 1]))]
    else:
        calls = [(_obs((B, 12, F), 3), torch.tensor([12, 7, 9]))]
    gws = [torch.randn(B, x.shape[1], H, generator=torch.Generator().manual_seed(4)) for x, _ in calls]

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
def test_dense_gcm_with_gine_stack(bridge):
    """T > N: the overflow roll moves both ends of every edge alike, the time column does not change."""
    from gcm import gine as GE, nn as G
    from gcm.gcm import DenseGCM, DenseToSparse, SparseToDense
    from gcm.edge_selectors.temporal import TemporalBackedge
    B, F, H, N, T = 3, 8, 16, 8, 12
    torch.manual_seed(8)
    ref = pyg.Sequential("x, adj, weights, B, N", [
        (RelativeEdgeAttrRef(**_REL_KW), "x, adj -> ea"), (_gine_layer(DenseGINERef, F, H), "x, adj, ea -> x"),
        (pyg.DenseGraphConv(H, H), "x, adj -> x"), torch.nn.Tanh()])
    if bridge:
        dev = G.Sequential("x, adj, weights, B, N", [
            (DenseToSparse(transpose=True), "x, adj -> x_sp, edge_index, batch_idx"),
            (GE.RelativeEdgeAttr(**_REL_KW), "x_sp, edge_index -> ea"),
            (_gine_layer(GE.GINEConv, F, H), "x_sp, edge_index, ea -> x_sp"),
            (G.GraphConv(H, H), "x_sp, edge_index -> x_sp"), torch.nn.Tanh(),
            (SparseToDense(), "x_sp, edge_index, batch_idx, B, N -> x, adj"), (lambda x: x, "x -> x")])
        # the same parameters one stage later (the bridge is stage 0)
        names = {k: "module_%d.%s" % (int(k.split(".")[0][7:]) - 1, k.split(".", 1)[1]) for k, _ in dev.named_parameters()}
        assert set(names.values()) == {k for k, _ in ref.named_parameters()}
        with torch.no_grad():
            for k, p in dev.named_parameters():
                p.copy_(dict(ref.named_parameters())[names[k]])
    else:
        dev = G.Sequential("x, adj, weights, B, N", [
            (GE.RelativeEdgeAttr(**_REL_KW), "x, adj -> ea"), (_gine_layer(GE.DenseGINEConv, F, H), "x, adj, ea -> x"),
            (G.DenseGraphConv(H, H), "x, adj -> x"), torch.nn.Tanh()])
        dev.load_state_dict(ref.state_dict())
        names = {k: k for k, _ in dev.named_parameters()}
    dev = dev.to(DEV)
    obs = _obs((T, B, F), 11)
    gw = torch.randn(T, B, H, generator=torch.Generator().manual_seed(12))

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
