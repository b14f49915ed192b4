"""DenseRGCNConv / RGCNConv kernels against the eager restatement (tests/_rgcn_restate.py), evaluated in float64 for
the bound and in float32 for the restatement's own error (tests/_gcn_restate.py's rule): output and every gradient.
The cases are tests/_rgcn_cases.py's; tests/test_rgcn_cpu.py asserts their preconditions.  Needs an MI355X."""
import copy

import pytest
import torch

from _gcn_restate import assert_bounded
from _rgcn_cases import (DENSE, SPARSE, dense_id, dense_operands, layer_kwargs, sparse_id, sparse_operands)
from _rgcn_restate import RGCNRef, bridge_edges

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7       # tests/_golden.py's floor for gradients (outputs: 2e-6)


def _layer(cls, Fi, Fo, R, opts, **extra):
    """(the layer with parameters away from their init - a zero bias hides a missing bias gradient path - , its
    restatement with the same parameters)."""
    from gcm import nn as G
    kw = layer_kwargs(opts)
    conv = getattr(G, cls)(Fi, Fo, R, **kw, **extra)
    with torch.no_grad():
        for p in conv.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
    ref = RGCNRef(Fi, Fo, R, **kw)
    ref.load_state_dict(conv.state_dict())
    return conv, ref


def _ref_eval(ref, call, inputs, g, dtype):
    ref_ = copy.deepcopy(ref).to(dtype)
    ts = {k: t.detach().to(dtype).requires_grad_() for k, t in inputs.items()}
    out = call(ref_, **ts)
    out.backward(g.to(dtype))
    grads = {k: t.grad for k, t in ts.items()}
    grads.update({k: p.grad for k, p in ref_.named_parameters()})
    return out, grads


def _check(out, got, ref, call, inputs, g):
    o64, g64 = _ref_eval(ref, call, inputs, g, torch.float64)
    o32, g32 = _ref_eval(ref, call, inputs, g, torch.float32)
    assert out.shape == o64.shape
    assert_bounded(out, o64, o32, "out")
    for name, b64 in g64.items():
        assert got[name] is not None, name
        assert_bounded(got[name], b64, g32[name], name, floor=GRAD_FLOOR, relative=True)


def _run_dense(case):
    B, N, Fi, Fo, R, opts = case
    ops = dense_operands(case)
    conv, ref = _layer("DenseRGCNConv", Fi, Fo, R, opts)
    dconv = copy.deepcopy(conv).to(DEV)
    xd = ops["x"].to(DEV).requires_grad_()
    ad = ops["adj"].to(DEV).requires_grad_(not opts.get("no_adj_grad"))
    rd = ops["rel"].to(DEV)
    mask = ops["mask"]
    out = dconv(xd, ad, rd, None if mask is None else mask.to(DEV))
    out.backward(ops["g"].to(DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    got = {"x": xd.grad, "adj": ad.grad}
    got.update({k: p.grad for k, p in dconv.named_parameters()})
    inputs = {"x": ops["x"], "adj": ops["adj"]}
    if opts.get("no_adj_grad"):
        assert ad.grad is None
        inputs.pop("adj")
    rel = ops["rel"]

    def call(ref_, x, adj=None):
        adj = ops["adj"].to(x.dtype) if adj is None else adj
        return ref_(x, adj, rel, mask)

    _check(out, got, ref, call, inputs, ops["g"])
    return out, got


@pytest.mark.parametrize("case", DENSE, ids=dense_id)
def test_dense_rgcnconv(case):
    _run_dense(case)


def _run_sparse(case, mode, attached):
    from gcm import _ops
    M, E, R, opts = case
    Fi, Fo = 6, 5
    ops = sparse_operands(case, Fi, Fo)
    mask_mode = mode != "ids"
    conv, ref = _layer("RGCNConv", Fi, Fo, R, opts, relation_mask=mask_mode)
    dconv = copy.deepcopy(conv).to(DEV)
    et = {"ids": ops["ids"], "codes": ops["codes"], "float_codes": ops["codes"].float()}[mode]
    xd = ops["x"].to(DEV).requires_grad_()
    ei = ops["edge_index"].to(DEV)
    if attached:
        ei.gcm_graph = _ops.GraphIndex.from_edge_index(ei, M)
    out = dconv(xd, ei, et.to(DEV))
    out.backward(ops["g"].to(DEV))
    torch.cuda.synchronize()
    got = {"x": xd.grad}
    got.update({k: p.grad for k, p in dconv.named_parameters()})

    def call(ref_, x):
        return ref_.sparse(x, ops["edge_index"], et.long(), mask_mode)

    _check(out, got, ref, call, {"x": ops["x"]}, ops["g"])
    return out, got


@pytest.mark.parametrize("attached", [False, True], ids=["built", "attached"])
@pytest.mark.parametrize("mode", ["ids", "codes"])
@pytest.mark.parametrize("case", SPARSE, ids=sparse_id)
def test_rgcnconv(case, mode, attached):
    _run_sparse(case, mode, attached)


def test_rgcnconv_float_codes_and_add():
    """Mask mode takes float32 codes too (what the bridge's edge values are); and the sum aggregation."""
    _run_sparse(SPARSE[1], "float_codes", False)
    M, E, R, _ = SPARSE[3]
    _run_sparse((M, E, R, {"hub": True, "aggr": "add", "num_bases": 2}), "codes", False)


def test_dense_equals_sparse_through_the_bridge():
    """The same planes through DenseToSparse(transpose=True, edge_values=True) into RGCNConv(relation_mask=True)."""
    from gcm import nn as G
    from gcm.gcm import DenseToSparse
    case = DENSE[4]
    B, N, Fi, Fo, R, opts = case
    ops = dense_operands(case)
    dense, ref = _layer("DenseRGCNConv", Fi, Fo, R, opts)
    sparse = G.RGCNConv(Fi, Fo, R, relation_mask=True)
    sparse.load_state_dict(dense.state_dict())
    dense, sparse = dense.to(DEV), sparse.to(DEV)
    x, rel = ops["x"].to(DEV), ops["rel"].to(DEV)
    adj = (rel > 0).float()
    out_d = dense(x, adj, rel)
    x_sp, edge_index, _, codes = DenseToSparse(transpose=True, edge_values=True)(x, rel)
    out_s = sparse(x_sp, edge_index, codes).view(B, N, Fo)
    ei_ref, codes_ref = bridge_edges(ops["rel"])
    assert codes.numel() == codes_ref.numel() and torch.equal(codes.cpu().sort().values, codes_ref.sort().values)
    o64 = ref.double()(ops["x"].double(), adj.cpu().double(), ops["rel"])
    o32 = ref.float()(ops["x"], adj.cpu(), ops["rel"])
    assert_bounded(out_d, o64, o32, "dense")
    assert_bounded(out_s, o64, o32, "sparse")


def test_bitwise_reproducible():
    for case in (DENSE[4], DENSE[15]):
        a, ga = _run_dense(case)
        b, gb = _run_dense(case)
        assert torch.equal(a, b)
        for k in ga:
            assert ga[k] is None and gb[k] is None or torch.equal(ga[k], gb[k]), k
    a, ga = _run_sparse(SPARSE[3], "codes", False)
    b, gb = _run_sparse(SPARSE[3], "codes", False)
    assert torch.equal(a, b) and all(torch.equal(ga[k], gb[k]) for k in ga)


def test_limits_raise_before_a_launch():
    from gcm import nn as G
    conv = G.DenseRGCNConv(129, 4, 2).to(DEV)
    with pytest.raises(NotImplementedError):
        conv(torch.zeros(1, 3, 129, device=DEV), torch.zeros(1, 3, 3, device=DEV), torch.zeros(1, 3, 3, device=DEV))
    sp = G.RGCNConv(4, 129, 2).to(DEV)
    with pytest.raises(NotImplementedError):
        sp(torch.zeros(3, 4, device=DEV), torch.zeros(2, 0, dtype=torch.long, device=DEV),
           torch.zeros(0, dtype=torch.long, device=DEV))
