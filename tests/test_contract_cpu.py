"""The calling contract of the conv layers of gcm.nn (gcm/nn.py: _dense_contract / _sparse_contract), the half that
needs no GPU: every REJECTION is tested here and only here - a wrong dtype, a wrong shape or a host tensor handed to a
kernel is what faults a device, so tests/test_contract_gpu.py passes accepted operands only.

Per layer class of tests/_contract.py's table, on its smallest case:
  * dtype: x float64 / float16, adj float64, edge_index int32, edge_weight float64, module.double() -> TypeError that
    names the operand;
  * shape: x one column too wide, adj [B,N,N+1], edge_index [3,E] and [E,2], a mask one entry short -> ValueError;
  * the float32 call on the host -> HipLibraryError, "no CPU fallback";
  * in all of these nothing is reached: _ops._call, _ops.ptr_from_sorted and torch.sort are replaced by functions that
    fail the test.
The device rule is tested on the helpers with duck-typed stand-ins for device tensors, the normaliser on CPU tensors
through `device=False`, which skips the device check alone."""
import pytest
import torch

import _contract as C

LAYER_IDS = C.LAYER_IDS
DENSE_IDS = [lid for lid in LAYER_IDS if lid.startswith("Dense")]
SPARSE_IDS = [lid for lid in LAYER_IDS if not lid.startswith("Dense")]
# the layers without an in_channels of their own: GIN's width is its nn's business (the nn refuses a wrong one itself),
# GatedGraphConv takes any width up to out_channels (its own rule, a ValueError too: tested with out_channels + 1)
NO_IN_CHANNELS = ("GINConv", "DenseGINConv")
GATED = ("GatedGraphConv", "DenseGatedGraphConv")


def _reached(what):
    def fail(*a, **k):
        raise AssertionError("%s was reached before the contract's error" % what)
    return fail


@pytest.fixture
def small(lid):
    """The layer's smallest case, built before `nothing_runs` takes torch.sort away (the case builders use it)."""
    return C.smallest(lid)


@pytest.fixture
def nothing_runs(monkeypatch):
    """No library call, no index build, no sort: what the old code reached before (or instead of) its error."""
    from gcm import _ops
    monkeypatch.setattr(_ops, "_call", _reached("_ops._call"))
    monkeypatch.setattr(_ops, "ptr_from_sorted", _reached("_ops.ptr_from_sorted"))
    monkeypatch.setattr(torch, "sort", _reached("torch.sort"))


def _rejects(c, conv, ops, exc, names):
    with pytest.raises(exc) as info:
        C.call(conv, ops)
    msg = str(info.value)
    assert any(n in msg for n in names), "%s: the message names none of %s: %s" % (c.id, names, msg)
    assert type(conv).__name__ + ": " in msg, "%s: the message does not name the layer: %s" % (c.id, msg)


# which operand, as which dtype (or the module converted), per layer: only what the layer takes
WEIGHTED = ("GraphConv-add", "GraphConv-mean", "GraphConv-max", "GCNConv", "GatedGraphConv", "TAGConv")
_FLOATS = {"float64": torch.float64, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _dtype_cases(lid):
    whats = ["x-float64", "x-float16", "x-bfloat16", "module-double", "module-half"]
    if lid.startswith("Dense"):
        return whats + ["adj-float64", "mask-int64"]
    whats += ["edge_index-int32", "edge_index-float32"]
    whats += ["edge_weight-float64"] if lid in WEIGHTED else []
    return whats + (["edge_type-int32"] if lid == "RGCNConv" else [])


DTYPE_CASES = [(lid, what) for lid in LAYER_IDS for what in _dtype_cases(lid)]


@pytest.mark.parametrize("lid,what", DTYPE_CASES, ids=["%s-%s" % lw for lw in DTYPE_CASES])
def test_dtypes_are_rejected_not_cast(lid, what, small, nothing_runs):
    c = small
    assert ("edge_weight" in c.ops) == (lid in WEIGHTED) and ("edge_type" in c.ops) == (lid == "RGCNConv")
    operand, dtype = what.split("-")
    conv, ops = c.product(), dict(c.ops)
    if operand == "module":
        conv = conv.double() if dtype == "double" else conv.half()
        names = ["parameter "]
    elif operand == "mask":
        ops["mask"] = C.mask_of(c).to(torch.int64)
        names = ["mask must be bool or float32"]
    else:
        ops[operand] = ops[operand].to(_FLOATS.get(dtype, torch.int32))
        names = ["%s must be %s" % (operand, "int64" if operand in ("edge_index", "edge_type") else "float32")]
    _rejects(c, conv, ops, TypeError, names)


@pytest.mark.parametrize("lid", LAYER_IDS)
def test_shapes_are_value_errors(lid, small, nothing_runs):
    c = small
    conv = c.product()
    x = c.ops["x"]
    if lid not in NO_IN_CHANNELS:
        width = conv.out_channels + 1 if lid in GATED else x.shape[-1] + 1
        wide = torch.zeros(*x.shape[:-1], width)
        wide[..., :x.shape[-1]] = x
        with pytest.raises(ValueError):
            C.call(conv, {**c.ops, "x": wide})
    with pytest.raises(ValueError, match="x must be"):
        C.call(conv, {**c.ops, "x": x.reshape(-1)})
    if c.dense:
        adj = c.ops["adj"]
        B, N = x.shape[:2]
        for bad in (torch.zeros(B, N, N + 1), torch.zeros(B, N + 1, N), torch.zeros(B + 1, N, N), torch.zeros(N * N)):
            with pytest.raises(ValueError, match="adj must be"):
                C.call(conv, {**c.ops, "adj": bad})
        with pytest.raises(ValueError, match="x must be"):
            C.call(conv, {**c.ops, "x": x[None], "adj": adj})
        mask = C.mask_of(c)
        with pytest.raises(ValueError, match="mask must hold"):
            C.call(conv, {**c.ops, "mask": mask.reshape(-1)[:-1]})
    else:
        ei = c.ops["edge_index"]
        for bad in (torch.cat([ei, ei[:1]]), ei.t().contiguous(), ei.reshape(-1), ei[None]):
            assert bad.shape[0] != 2 or bad.dim() != 2
            with pytest.raises(ValueError, match="edge_index must be"):
                C.call(conv, {**c.ops, "edge_index": bad})


@pytest.mark.parametrize("lid", LAYER_IDS)
def test_a_host_call_fails_before_any_work(lid, small, nothing_runs):
    from gcm import _hip
    c = small
    ops = dict(c.ops)
    if c.dense:
        ops["mask"] = C.mask_of(c)
    conv = c.product()
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback") as info:
        C.call(conv, ops)
    assert type(conv).__name__ + ": x is on 'cpu'" in str(info.value)


def test_dtype_comes_before_shape_and_shape_before_device(nothing_runs):
    """The order of the steps: a call wrong in all three ways reports its dtype, wrong in two its shape."""
    from gcm import nn as G
    conv = G.GCNConv(3, 4)
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(TypeError, match="edge_index must be int64"):
        conv(torch.zeros(3, 9), ei.int().t())
    with pytest.raises(ValueError, match="in_channels=3"):
        conv(torch.zeros(3, 9), ei)
    with pytest.raises(ValueError, match="edge_weight has 5 entries for 2 edges"):
        conv(torch.zeros(3, 3), ei, torch.ones(5))            # GCNConv's own rule stays, and stays a shape error
    G.GraphConv(3, 4)                                         # (GraphConv ignores a wrong-length weight: on the device)


# ---------------------------------------------------------------------------
# the device rule, on the helpers: a machine without a GPU has no device tensor, so a stand-in plays it
# ---------------------------------------------------------------------------
class OnDevice:
    """What the contract reads of a tensor up to its device step."""

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.dtype = torch.Size(shape), dtype
        self.is_cuda, self.device = True, torch.device("cuda", 0)

    def is_contiguous(self):
        return True

    def numel(self):
        return self.shape.numel()


def test_every_operand_is_checked_for_its_device(nothing_runs):
    from gcm import nn as G, _hip
    sparse = G.GraphConv(3, 4)
    x, ei = OnDevice(5, 3), OnDevice(2, 7, dtype=torch.int64)
    with pytest.raises(_hip.HipLibraryError, match="GraphConv: edge_index is on 'cpu'.*no CPU fallback"):
        G._sparse_contract(sparse, x, torch.zeros(2, 7, dtype=torch.int64), 3)
    with pytest.raises(_hip.HipLibraryError, match="GraphConv: edge_weight is on 'cpu'.*no CPU fallback"):
        G._sparse_contract(sparse, x, ei, 3, edge_weight=torch.ones(7))
    with pytest.raises(_hip.HipLibraryError, match="GraphConv: edge_attr is on 'cpu'.*no CPU fallback"):
        G._sparse_contract(sparse, x, ei, 3, edge_attr=torch.ones(7, 2))
    with pytest.raises(_hip.HipLibraryError, match="GraphConv: edge_type is on 'cpu'.*no CPU fallback"):
        G._sparse_contract(sparse, x, ei, 3, edge_type=torch.zeros(7, dtype=torch.int64))
    with pytest.raises(_hip.HipLibraryError, match="GraphConv: x is on 'cpu'.*no CPU fallback"):
        G._sparse_contract(sparse, torch.zeros(5, 3), ei, 3)
    dense = G.DenseGraphConv(3, 4)
    x, adj = OnDevice(2, 5, 3), OnDevice(2, 5, 5)
    with pytest.raises(_hip.HipLibraryError, match="DenseGraphConv: adj is on 'cpu'.*no CPU fallback"):
        G._dense_contract(dense, x, torch.zeros(2, 5, 5), None, 3)
    with pytest.raises(_hip.HipLibraryError, match="DenseGraphConv: mask is on 'cpu'.*no CPU fallback"):
        G._dense_contract(dense, x, adj, torch.ones(2, 5, dtype=torch.bool), 3)
    with pytest.raises(_hip.HipLibraryError, match="DenseRGCNConv: rel is on 'cpu'.*no CPU fallback"):
        G._dense_contract(G.DenseRGCNConv(3, 4, 2), x, adj, None, 3, planes=[("rel", torch.zeros(2, 5, 5))])
    # with every operand on the device, the module's own tensors are next: a parameter, named
    with pytest.raises(_hip.HipLibraryError, match="DenseGraphConv: parameter lin_rel.weight is on 'cpu'"):
        G._dense_contract(dense, x, adj, None, 3)
    with pytest.raises(_hip.HipLibraryError, match="GINConv: parameter nn.0.weight is on 'cpu'"):
        G._sparse_contract(G.GINConv(torch.nn.Sequential(torch.nn.Linear(3, 4))), OnDevice(5, 3), ei)


# ---------------------------------------------------------------------------
# the normaliser, on CPU tensors
# ---------------------------------------------------------------------------
def _same_values_kernel_ready(got, view, what):
    assert C.is_kernel_ready(got), what + ": not contiguous and 16-byte aligned"
    assert got.shape == view.shape and torch.equal(got, view), what + ": the values changed"


def test_kernel_ready_copies_only_what_it_must():
    from gcm import _hip
    v = torch.randn(3, 7, 5)
    for name, (base, select) in (("columns", C.embed_columns(v)), ("transposed", C.embed_transposed(v)),
                                 ("offset", C.embed_offset(v)), ("expanded", C.embed_expanded(v[:1].repeat(3, 1, 1))),
                                 ("every other", C.embed_every_other(v.reshape(-1)))):
        view = select(base)
        assert not C.is_kernel_ready(view), name + ": the form is not awkward"
        _same_values_kernel_ready(_hip.kernel_ready(view), view, name)
    off = C.embed_offset(v)
    assert off[1](off[0]).is_contiguous() and off[1](off[0]).data_ptr() % 16 == 4      # only the alignment is off
    assert _hip.kernel_ready(v) is v and _hip.kernel_ready(None) is None
    aligned = torch.zeros(64)[4:36]                                                   # a view, but 16 bytes in
    assert _hip.kernel_ready(aligned) is aligned
    empty = torch.zeros(0, 3)
    assert _hip.kernel_ready(empty) is empty
    # under autograd the copy is a node: the gradient reaches the leaf, zero outside the view
    base, select = C.embed_offset(v)
    base.requires_grad_()
    g = torch.randn(3, 7, 5)
    _hip.kernel_ready(select(base)).backward(g)
    assert torch.equal(base.grad, C.expected_grad(base.detach(), select, g)) and base.grad[0] == 0


def test_dense_contract_normalises_every_layout():
    from gcm import nn as G
    conv = G.DenseGraphConv(5, 4)
    B, N, F = 3, 7, 5
    x, adj = torch.randn(B, N, F), torch.rand(B, N, N)
    got = G._dense_contract(conv, x, adj, None, F, device=False)
    assert got[0] is x and got[1] is adj, "kernel-ready operands must come back as they are: no copy"
    for name, embed in (("column slice", C.embed_columns), ("transposed", C.embed_transposed),
                        ("offset", C.embed_offset)):
        for which, value in (("x", x), ("adj", adj)):
            base, select = embed(value)
            view = select(base)
            ops = {"x": x, "adj": adj, which: view}
            gx, ga = G._dense_contract(conv, ops["x"], ops["adj"], None, F, device=False)
            _same_values_kernel_ready({"x": gx, "adj": ga}[which], view, "%s as a %s" % (which, name))
            assert (ga if which == "x" else gx) is (adj if which == "x" else x)
    one = adj[:1].clone()
    for bcast in (one, one[0], one.expand(B, -1, -1)):                 # [1,N,N], [N,N], a zero-stride batch
        gx, ga = G._dense_contract(conv, x, bcast, None, F, device=False)
        _same_values_kernel_ready(ga, one.repeat(B, 1, 1), "a broadcast adj")
    gx, ga = G._dense_contract(conv, x[0], adj[0], None, F, device=False)          # 2-D operands: a batch of one
    assert gx.shape == (1, N, F) and ga.shape == (1, N, N) and C.is_kernel_ready(gx) and C.is_kernel_ready(ga)
    gx, ga, gr = G._dense_contract(G.DenseRGCNConv(F, 4, 2), x, adj, None, F, planes=[("rel", one[0].long())],
                                   device=False)
    _same_values_kernel_ready(gr, one.long().repeat(B, 1, 1), "a broadcast plane")
    # the mask goes through torch alone: any layout, by reshape
    out = torch.randn(B, N, 4)
    mask = torch.rand(B, N) < 0.5
    want = out * mask[..., None]
    for m in (mask, mask.t().contiguous().t(), mask.float(), C.embed_every_other(mask.reshape(-1))[1](
            C.embed_every_other(mask.reshape(-1))[0])):
        assert torch.equal(G._masked(out, m, x), want)


def test_sparse_contract_normalises_every_layout():
    from gcm import nn as G
    conv = G.GraphConv(5, 4)
    M, E, F = 9, 21, 5
    x, w = torch.randn(M, F), torch.rand(E)
    ei = torch.randint(0, M, (2, E))
    et = torch.randint(0, 3, (E,))
    got = G._sparse_contract(conv, x, ei, F, edge_weight=w, edge_type=et, device=False)
    assert got[0] is x and got[1] is ei and got[2] is w and got[3] is et, "kernel-ready operands: no copy"
    forms = [("x", x, C.embed_columns), ("x", x, C.embed_transposed), ("x", x, C.embed_offset),
             ("edge_index", ei, C.embed_pairs), ("edge_index", ei, C.embed_wide_index),
             ("edge_weight", w, C.embed_every_other), ("edge_weight", w, C.embed_offset),
             ("edge_type", et, C.embed_every_other)]
    for which, value, embed in forms:
        base, select = embed(value)
        view = select(base)
        assert not C.is_kernel_ready(view) or embed is C.embed_offset
        ops = {"x": x, "edge_index": ei, "edge_weight": w, "edge_type": et, which: view}
        got = dict(zip(("x", "edge_index", "edge_weight", "edge_type"),
                       G._sparse_contract(conv, ops["x"], ops["edge_index"], F, edge_weight=ops["edge_weight"],
                                          edge_type=ops["edge_type"], device=False)))
        _same_values_kernel_ready(got[which], view, "%s as %s" % (which, embed.__name__))
        for other in got:
            assert other == which or got[other] is ops[other]
    # what the memories attach survives a copy or forbids it
    pairs = ei.t().contiguous().t()
    pairs.gcm_graph = type("Index", (), {"M": M})()
    assert G._sparse_contract(conv, x, pairs, F, device=False)[1] is pairs, "an indexed list is not read again"
    pairs.gcm_graph.M = M + 1
    assert C.is_kernel_ready(G._sparse_contract(conv, x, pairs, F, device=False)[1])
    unit = C.embed_every_other(torch.ones(E))
    unit = unit[1](unit[0])
    unit.gcm_unit_weights = True
    assert G._sparse_contract(conv, x, ei, F, edge_weight=unit, device=False)[2].gcm_unit_weights is True
