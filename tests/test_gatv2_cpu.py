"""GATv2Conv / DenseGATv2Conv host side: parameters, refusals, the placeholder gcm.nn keeps, the restatement the GPU
tests compare against (checked against the GATv2 body already pinned in tests/_mp_restate.py, dense against sparse,
and on hand-computed cases) and the exactness of the quantised inputs.  No kernel runs."""
import math

import pytest
import torch

from _gatv2_restate import (DENSE_CASES, SPARSE_CASES, DenseGATv2Ref, GATv2Ref, case_id, dense_case, dense_gatv2,
                            exactness, gatv2, layer_kwargs, quant_layer, sparse_case, terms)
from _gine_restate import quant
from _mp_restate import RefMessagePassing, layers

CLASSES = ["GATv2Conv", "DenseGATv2Conv"]


def _cls(name):
    from gcm import gatv2 as GV
    return getattr(GV, name)


# ---- construction ---------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [False, True], ids=["own-lin_r", "share_weights"])
@pytest.mark.parametrize("edge_dim", [None, 3])
@pytest.mark.parametrize("concat,bias", [(True, True), (False, True), (True, False)])
def test_parameters(concat, bias, edge_dim, share):
    Fi, C, H = 6, 5, 2
    want = {"att": (1, H, C), "lin_l.weight": (H * C, Fi), "lin_r.weight": (H * C, Fi)}
    if bias:
        want.update({"lin_l.bias": (H * C,), "lin_r.bias": (H * C,), "bias": (H * C if concat else C,)})
    if edge_dim is not None:
        want["lin_edge.weight"] = (H * C, edge_dim)
    kw = dict(heads=H, concat=concat, edge_dim=edge_dim, bias=bias, share_weights=share)
    s, d = _cls("GATv2Conv")(Fi, C, **kw), _cls("DenseGATv2Conv")(Fi, C, **kw)
    for m in (s, d, GATv2Ref(Fi, C, **kw), DenseGATv2Ref(Fi, C, **kw)):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
        assert (m.lin_r is m.lin_l) == share
        assert len(list(m.parameters())) == len(want) - (2 if bias else 1) * share      # the shared weight once
        assert (m.bias is None) == (not bias) and (m.lin_edge is None) == (edge_dim is None)
        assert m.lin_edge is None or m.lin_edge.bias is None
    # one loads into the other, and into the restatement
    s2 = _cls("GATv2Conv")(Fi, C, **kw)
    s2.load_state_dict(d.state_dict())
    d2 = _cls("DenseGATv2Conv")(Fi, C, **kw)
    d2.load_state_dict(s.state_dict())
    for k, v in d.state_dict().items():
        assert torch.equal(s2.state_dict()[k], v)
    GATv2Ref(Fi, C, **kw).load_state_dict(s.state_dict())
    assert repr(s) == "GATv2Conv(6, 5, heads=2)" and repr(d) == "DenseGATv2Conv(6, 5, heads=2)"
    assert s.add_self_loops is True and s.fill_value == "mean" and s.negative_slope == 0.2 and s.dropout == 0.0


@pytest.mark.parametrize("cls", CLASSES)
def test_reset_parameters(cls):
    H, C = 3, 4
    conv = _cls(cls)(6, C, heads=H, edge_dim=2)
    with torch.no_grad():
        for p in conv.parameters():
            p.fill_(9.0)
    torch.manual_seed(0)
    conv.reset_parameters()
    for lin in (conv.lin_l, conv.lin_r, conv.lin_edge):
        bound = math.sqrt(6.0 / (lin.in_features + lin.out_features))                  # xavier uniform
        top = float(lin.weight.detach().abs().max())
        assert 0.5 * bound < top <= bound
        assert lin.bias is None or not lin.bias.any()
    bound = math.sqrt(6.0 / (H + C))                                                   # glorot on the last two dims
    assert float(conv.att.detach().abs().max()) <= bound and float(conv.att.detach().std()) > 0.2 * bound
    assert not conv.bias.any()


# ---- refusals -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_constructor_refusals(cls):
    C = _cls(cls)
    for bad in ("max", None, [1.0], True):
        with pytest.raises(NotImplementedError, match="fill_value"):
            C(4, 4, edge_dim=2, fill_value=bad)
    with pytest.raises(NotImplementedError, match="in_channels"):
        C((4, 4), 4)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="dropout"):
            C(4, 4, dropout=bad)
    C(4, 4, dropout=1.0), C(4, 4, fill_value=2), C(4, 4, fill_value=0.5)
    if cls == "GATv2Conv":
        with pytest.raises(NotImplementedError, match="residual"):
            C(4, 4, residual=True)


def test_call_refusals():
    GV2 = _cls("GATv2Conv")
    x, ei = torch.randn(5, 4), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(NotImplementedError, match="return_attention_weights"):
        GV2(4, 4)(x, ei, return_attention_weights=True)
    for cls, edges in (("GATv2Conv", ei), ("DenseGATv2Conv", torch.ones(1, 5, 5))):
        conv = _cls(cls)(4, 4, dropout=0.5)
        with pytest.raises(NotImplementedError, match="dropout"):
            conv(x, edges)                                         # training mode
        conv.eval()
        with pytest.raises(Exception) as info:                     # eval mode gets past it: the next stop is the device
            conv(x, edges)
        assert "dropout" not in str(info.value)
        with pytest.raises(ValueError, match="edge_attr"):
            _cls(cls)(4, 4, edge_dim=2)(x, edges)


@pytest.mark.parametrize("cls", CLASSES)
def test_width_limits(cls):
    C = _cls(cls)
    x, edges = (torch.randn(5, 130), torch.tensor([[0, 1], [1, 2]])) if cls == "GATv2Conv" else \
        (torch.randn(1, 5, 130), torch.ones(1, 5, 5))
    with pytest.raises(ValueError, match="in_channels=130.*128"):
        C(130, 4)(x, edges)
    with pytest.raises(ValueError, match="heads \\* out_channels = 132.*128"):
        C(4, 33, heads=4)(x[..., :4], edges)
    with pytest.raises(ValueError, match="edge_dim=33.*32"):
        C(4, 4, edge_dim=33)(x[..., :4], edges, torch.randn(2, 33))


def test_placeholder_in_gcm_nn_stays():
    from gcm import gatv2 as GV, nn as G
    with pytest.raises(NotImplementedError, match="GATv2Conv is not implemented"):
        G.GATv2Conv(4, 4)
    assert GV.GATv2Conv is not G.GATv2Conv and not hasattr(G, "DenseGATv2Conv")
    assert "from gcm.gatv2 import GATv2Conv" in GV.__doc__


# ---- the restatement ------------------------------------------------------------------------------
def test_restatement_agrees_with_the_pinned_message_passing_body():
    """tests/_mp_restate.py's GATv2 on RefMessagePassing: add_self_loops=False, no edge_dim, concat, float64; a list
    with duplicates, self edges and isolated nodes."""
    M, Fi, H, C = 9, 4, 3, 5
    torch.manual_seed(1)
    body = layers(RefMessagePassing).GATv2(Fi, C, heads=H, negative_slope=0.3).double()
    with torch.no_grad():
        body.bias.copy_(torch.randn(H * C))
    ei = torch.tensor([[0, 1, 1, 2, 3, 3, 5, 0, 4], [1, 2, 2, 2, 0, 0, 5, 4, 1]])       # 7, 8 isolated; 6 a source of none
    x = torch.randn(M, Fi, dtype=torch.float64)
    ref = GATv2Ref(Fi, C, heads=H, negative_slope=0.3, add_self_loops=False).double()
    ref.load_state_dict(body.state_dict())
    want, got = body(x, ei), ref(x, ei)
    assert float((want - got).detach().abs().max()) <= 1e-12
    assert torch.equal(got[6:], ref.bias.expand(3, -1))            # no in-edge: bias


@pytest.mark.parametrize("fill", ["mean", 0.75])
@pytest.mark.parametrize("add_loop", [True, False])
def test_dense_restatement_equals_sparse(add_loop, fill):
    B, N, Fi, H, C, D = 2, 9, 4, 2, 3, 3
    gen = torch.Generator().manual_seed(2)
    adj = (torch.rand(B, N, N, generator=gen) < 0.3).double()
    adj[:, 2] = 0
    adj[:, 1, 1] = 1
    x, ea = torch.randn(B, N, Fi, generator=gen).double(), torch.randn(B, N, N, D, generator=gen).double()
    torch.manual_seed(3)
    ref = DenseGATv2Ref(Fi, C, heads=H, edge_dim=D, fill_value=fill).double()
    sp = GATv2Ref(Fi, C, heads=H, edge_dim=D, fill_value=fill, add_self_loops=add_loop).double()
    sp.load_state_dict(ref.state_dict())
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])                   # adj[b, i, j]: j -> i
    want = sp(x.view(B * N, Fi), ei, ea[bb, ii, jj]).view(B, N, H * C)
    got = ref(x, adj, ea, add_loop=add_loop)
    assert float((want - got).detach().abs().max()) <= 1e-12
    if not add_loop:
        assert torch.equal(got[:, 2], ref.bias.expand(B, -1))      # the empty row
    # NaN at the unset entries is not read
    ea_nan = torch.where((adj != 0).unsqueeze(-1), ea, torch.full((), float("nan"), dtype=torch.float64))
    assert torch.equal(ref(x, adj, ea_nan, add_loop=add_loop), got)


def _hand_layer(H=1, C=2, D=None, **kw):
    ref = GATv2Ref(2, C, heads=H, edge_dim=D, **kw).double()
    with torch.no_grad():
        ref.lin_l.weight.copy_(torch.tensor([[1.0, 0.0], [0.0, 2.0]]))
        ref.lin_r.weight.copy_(torch.tensor([[0.5, 0.0], [0.0, -1.0]]))
        ref.lin_l.bias.zero_(), ref.lin_r.bias.zero_()
        ref.att.copy_(torch.tensor([[[1.0, -1.0]]]))
        ref.bias.copy_(torch.tensor([10.0, 20.0]))
        if D is not None:
            ref.lin_edge.weight.copy_(torch.tensor([[1.0], [0.0]]))
    return ref


def test_hand_computed_cases():
    x = torch.tensor([[1.0, 2.0], [3.0, -1.0], [0.5, 0.5]], dtype=torch.float64)
    # one in-edge 0 -> 1: alpha = 1, out_1 = x_l[0] + bias; nodes 0 and 2 have no in-edge: bias
    ref = _hand_layer(add_self_loops=False)
    out = ref(x, torch.tensor([[0], [1]]))
    assert torch.equal(out, torch.tensor([[10.0, 20.0], [11.0, 24.0], [10.0, 20.0]], dtype=torch.float64))
    # two in-edges of node 2, by hand: z = x_l[j] + x_r[2], s = lrelu(z0) - lrelu(z1)
    ei = torch.tensor([[0, 1], [2, 2]])
    out = ref(x, ei)
    xl = torch.tensor([[1.0, 4.0], [3.0, -2.0]])
    xr2 = torch.tensor([0.25, -0.5])
    lrelu = lambda v: v if v > 0 else 0.2 * v
    s = [lrelu(float(xl[k, 0] + xr2[0])) - lrelu(float(xl[k, 1] + xr2[1])) for k in range(2)]
    a0 = math.exp(s[0]) / (math.exp(s[0]) + math.exp(s[1]))
    want = a0 * xl[0].double() + (1 - a0) * xl[1].double() + torch.tensor([10.0, 20.0], dtype=torch.float64)
    assert float((out[2] - want).detach().abs().max()) <= 1e-12
    # the "mean" loop feature: node 2 has in-edges with features 1 and 3 -> its loop sees 2; node 0 has none -> 0.
    # lin_edge adds the feature to channel 0 of z.
    ref = _hand_layer(D=1)
    ea = torch.tensor([[1.0], [3.0]], dtype=torch.float64)
    _, dst, _, _, e, _ = terms(x, ei, ref.lin_l, ref.lin_r, ref.lin_edge, ea, 1, True, "mean")
    assert dst.tolist() == [2, 2, 0, 1, 2]                         # the loops come after the edges
    assert e[:, 0, 0].tolist() == [1.0, 3.0, 0.0, 0.0, 2.0] and not e[:, 0, 1].any()
    # node 0, loop only: alpha = 1, out_0 = x_l[0] + bias
    assert torch.equal(ref(x, ei, ea)[0], torch.tensor([11.0, 24.0], dtype=torch.float64))
    # a number is broadcast
    _, _, _, _, e, _ = terms(x, ei, ref.lin_l, ref.lin_r, ref.lin_edge, ea, 1, True, 0.5)
    assert e[:, 0, 0].tolist() == [1.0, 3.0, 0.5, 0.5, 0.5]
    # an i -> i edge is replaced by the loop: its own feature (100) is not seen, and does not enter the mean
    ei2 = torch.tensor([[0, 1, 2], [2, 2, 2]])
    ea2 = torch.tensor([[1.0], [3.0], [100.0]], dtype=torch.float64)
    assert torch.equal(ref(x, ei2, ea2), ref(x, ei, ea))
    # without add_self_loops it is an ordinary term
    ref.add_self_loops = False
    assert not torch.equal(ref(x, ei2, ea2)[2], ref(x, ei, ea)[2])


def test_derivative_at_zero_is_the_negative_slope():
    """z = 0 on one channel: the gradient that passes through it is scaled by negative_slope (torch's convention)."""
    ref = _hand_layer(add_self_loops=False)
    x = torch.tensor([[1.0, 2.0], [-2.0, 4.0]], dtype=torch.float64, requires_grad=True)  # z = x_l[0] + x_r[1] = (0, 0)
    ei = torch.tensor([[0, 0], [1, 1]])
    src, dst, x_l, x_r, _, z = terms(x, ei, ref.lin_l, ref.lin_r, heads=1, add_self_loops=False)
    assert not z.any()
    s = (torch.nn.functional.leaky_relu(z, 0.2) * ref.att).sum()
    g, = torch.autograd.grad(s, z)
    assert torch.equal(g, 0.2 * ref.att.detach().expand_as(g))


# ---- the inputs of the GPU cases are exact --------------------------------------------------------
def _exact(x_l, x_r, e, z):
    ok, top = exactness([x_l, x_r, e, z])
    assert ok and top < 2 ** 12, (ok, top)


@pytest.mark.parametrize("case", SPARSE_CASES, ids=case_id)
def test_sparse_cases_are_exact(case):
    M, E, Fi, H, C, D, opts = case
    x, ei, ea = sparse_case(*case)
    assert x.shape == (M, Fi) and ei.shape == (2, E) and (ea is None) == (D is None)
    kw = layer_kwargs(case)
    for variant in ({}, {"bias": False}, {"share_weights": True}):
        conv = GATv2Ref(**{**kw, **variant}).double()
        quant_layer(conv, torch.Generator().manual_seed(M + E))
        for loops in (True, False):
            _, dst, x_l, x_r, e, z = terms(x, ei, conv.lin_l, conv.lin_r, conv.lin_edge, ea, H, loops, conv.fill_value)
            _exact(x_l, x_r, e, z)
    if opts.get("mixed") and E >= 8:
        assert (ei[0] == ei[1]).any() and E > len({tuple(c) for c in ei.t().tolist()})
    assert M < 4 or not (ei >= M - 3).any()                        # isolated nodes


@pytest.mark.parametrize("case", DENSE_CASES, ids=case_id)
def test_dense_cases_are_exact(case):
    B, N, Fi, H, C, D, opts = case
    x, adj, ea, mask = dense_case(*case)
    add_loop = opts.get("add_loop", True)
    conv = GATv2Ref(**layer_kwargs(case)).double()
    quant_layer(conv, torch.Generator().manual_seed(B + N))
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])
    _, _, x_l, x_r, e, z = terms(x.view(B * N, Fi), ei, conv.lin_l, conv.lin_r, conv.lin_edge,
                                 None if ea is None else ea[bb, ii, jj], H, add_loop, conv.fill_value)
    _exact(x_l, x_r, e, z)
    if N > 1:
        assert adj[:, 1, 1].all()
    if not add_loop:
        assert not adj[:, 2].any()


def test_quantised_values_are_eighths():
    x = quant((5, 3), 8, 16, torch.Generator().manual_seed(0))
    assert torch.equal(x * 8, (x * 8).round()) and float(x.abs().max()) <= 2
