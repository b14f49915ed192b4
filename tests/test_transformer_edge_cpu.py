"""gcm.transformer's TransformerConv / DenseTransformerConv (edge_dim) host side: parameters, refusals, the C ABI's
validation, and the restatements the GPU tests compare against - the per-edge form pinned by hand-computed answers and
by the edge-free restatement, the factored form (the kernels' algebra, backward by hand) held against autograd of the
per-edge form in float64.  No kernel runs."""
import itertools
import math

import pytest
import torch

import _mp_restate as MP
import _transformer_restate as TR
from _transformer_edge_restate import (SPARSE_CASES, DenseTransformerEdgeRef, TransformerEdgeRef, dense_case,
                                       dense_transformer_edge, factored, mp_layer, sparse_case, transformer_edge)


# ---- parameters -----------------------------------------------------------------------------------
@pytest.mark.parametrize("edge_dim", [None, 3])
@pytest.mark.parametrize("concat,beta,root_weight,bias", list(itertools.product([True, False], repeat=4)))
def test_parameters(concat, beta, root_weight, bias, edge_dim):
    from gcm import nn as G, transformer as T
    F, C, H = 6, 5, 3
    D = H * C if concat else C
    want = {"lin_key.weight": (H * C, F), "lin_key.bias": (H * C,), "lin_query.weight": (H * C, F),
            "lin_query.bias": (H * C,), "lin_value.weight": (H * C, F), "lin_value.bias": (H * C,)}
    if edge_dim is not None:
        want["lin_edge.weight"] = (H * C, edge_dim)
    if root_weight:
        want["lin_skip.weight"] = (D, F)
        if bias:
            want["lin_skip.bias"] = (D,)
        if beta:
            want["lin_beta.weight"] = (1, 3 * D)
    kw = dict(heads=H, concat=concat, beta=beta, root_weight=root_weight, bias=bias, edge_dim=edge_dim)
    d, s, r = T.DenseTransformerConv(F, C, **kw), T.TransformerConv(F, C, **kw), TransformerEdgeRef(F, C, **kw)
    for m in (d, s, r):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert d.beta == s.beta == (beta and root_weight)
    sd = s.state_dict()
    assert 0 < float(sd["lin_query.weight"].abs().max()) <= 1 / math.sqrt(F)      # torch.nn.Linear's default init
    if edge_dim is not None:
        assert 0 < float(sd["lin_edge.weight"].abs().max()) <= 1 / math.sqrt(edge_dim)
    d.load_state_dict(s.state_dict())
    DenseTransformerEdgeRef(F, C, **kw).load_state_dict(d.state_dict())
    if edge_dim is None:                                          # each loads into the gcm.nn classes and back
        kw.pop("edge_dim")
        G.TransformerConv(F, C, **kw).load_state_dict(d.state_dict())
        s.load_state_dict(G.DenseTransformerConv(F, C, **kw).state_dict())
    before = {k: v.clone() for k, v in s.state_dict().items()}
    torch.manual_seed(1)
    s.reset_parameters()
    assert all(not torch.equal(v, before[k]) for k, v in s.state_dict().items())
    assert "heads=3" in repr(s) and "heads=3" in repr(d)


# ---- refusals -------------------------------------------------------------------------------------
def test_refusals():
    from gcm import nn as G, transformer as T, _hip
    assert _hip.TRE_MAX_EDGE_DIM == 32
    x, ei, ea = torch.zeros(3, 2), torch.tensor([[0, 1], [1, 2]]), torch.zeros(2, 3)
    adj, dea = torch.ones(3, 3), torch.zeros(3, 3, 3)
    for conv, args in ((T.TransformerConv(2, 2, dropout=0.5, edge_dim=3), (x, ei, ea)),
                       (T.DenseTransformerConv(2, 2, dropout=0.5, edge_dim=3), (x, adj, dea)),
                       (T.TransformerConv(2, 2, dropout=0.5), (x, ei))):
        with pytest.raises(NotImplementedError, match="dropout"):
            conv(*args)
        conv.eval()                                   # dropout is a no-op in eval mode: the call reaches the kernels
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            conv(*args)
    with pytest.raises(NotImplementedError, match="return_attention_weights"):
        T.TransformerConv(2, 2, edge_dim=3)(x, ei, ea, return_attention_weights=True)
    for cls in (T.TransformerConv, T.DenseTransformerConv):
        with pytest.raises(NotImplementedError, match="tuple"):
            cls((2, 3), 2, edge_dim=3)
    for conv, args, what in ((T.TransformerConv(130, 4, edge_dim=3), (torch.zeros(3, 130), ei, ea), "128"),
                             (T.TransformerConv(2, 33, heads=4, edge_dim=3), (x, ei, ea), "128"),
                             (T.TransformerConv(2, 2, edge_dim=33), (x, ei, torch.zeros(2, 33)), "32"),
                             (T.DenseTransformerConv(130, 4, edge_dim=3), (torch.zeros(3, 130), adj, dea), "128"),
                             (T.DenseTransformerConv(2, 65, heads=2, edge_dim=3), (x, adj, dea), "128"),
                             (T.DenseTransformerConv(2, 2, edge_dim=33), (x, adj, torch.zeros(3, 3, 33)), "32")):
        with pytest.raises(ValueError, match=what):
            conv(*args)
    with pytest.raises(ValueError, match="edge_attr is required"):
        T.TransformerConv(2, 2, edge_dim=3)(x, ei)
    with pytest.raises(ValueError, match="edge_attr is required"):
        T.DenseTransformerConv(2, 2, edge_dim=3)(x, adj)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):           # accepted and ignored without edge_dim
        T.TransformerConv(2, 2)(x, ei, ea)
    with pytest.raises(NotImplementedError, match="edge_dim"):                   # gcm.nn's layer stays as it was
        G.TransformerConv(2, 2, edge_dim=3)


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {
    "gcm_dense_transformer_edge_fwd_workspace_bytes", "gcm_dense_transformer_edge_fwd",
    "gcm_dense_transformer_edge_bwd_workspace_bytes", "gcm_dense_transformer_edge_bwd",
    "gcm_csr_transformer_edge_fwd_workspace_bytes", "gcm_csr_transformer_edge_fwd",
    "gcm_csr_transformer_edge_bwd_workspace_bytes", "gcm_csr_transformer_edge_bwd"}


def test_library_exports_every_symbol_of_the_header():
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_transformer_edge.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_transformer_edge.h")))
    assert declared == set(_hip.TRE_PROTOTYPES) == _FUNCTIONS
    assert not declared & (set(_hip.PROTOTYPES) | set(_hip.TRANSFORMER_PROTOTYPES) | set(_hip.GATV2_PROTOTYPES))
    lib = _hip.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == _hip.TRE_PROTOTYPES[name][1]
    assert lib.gcm_abi_version() == 8                         # the section is additive


def test_c_abi_rejects_null_pointers_and_wide_layers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_transformer_edge_fwd(*([None] * 9), 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, None) == _hip.EINVAL
    assert lib.gcm_dense_transformer_edge_bwd(*([None] * 14), 0, 1, 1, 1, 1, 1, 1, 1, 1, None) == _hip.EINVAL
    assert lib.gcm_csr_transformer_edge_fwd(*([None] * 11), 0, 1, 0, 1, 1, 1, 1, 1, 1, None) == _hip.EINVAL
    assert lib.gcm_csr_transformer_edge_bwd(*([None] * 20), 0, 1, 0, 1, 1, 1, 1, 1, 1, None) == _hip.EINVAL
    # widths over the limits are refused before anything is read or launched: any non-null address will do
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    for Fi, H, C, D in ((129, 1, 4, 3), (4, 2, 65, 3), (4, 1, 4, 33)):
        assert lib.gcm_dense_transformer_edge_fwd(*([p] * 9), 0, 1, 2, Fi, H, C, D, 1, 1, 0, None) \
            == _hip.GCM_EUNSUPPORTED
        assert lib.gcm_dense_transformer_edge_bwd(*([p] * 14), 0, 1, 2, Fi, H, C, D, 1, 1, None) \
            == _hip.GCM_EUNSUPPORTED
        assert lib.gcm_csr_transformer_edge_fwd(*([p] * 11), 0, 2, 1, Fi, H, C, D, 1, 1, None) == _hip.GCM_EUNSUPPORTED
        assert lib.gcm_csr_transformer_edge_bwd(*([p] * 20), 0, 2, 1, Fi, H, C, D, 1, 1, None) == _hip.GCM_EUNSUPPORTED


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    D = 3
    for concat, root in itertools.product((0, 1), repeat=2):
        for H, C in ((1, 32), (4, 8)):
            P = 3 * H * C + ((H * C if concat else C) if root else 0)
            base = lib.gcm_dense_transformerconv_fwd_workspace_bytes(256, 128, 32, H, C, concat, root)
            fwd = lib.gcm_dense_transformer_edge_fwd_workspace_bytes(256, 128, 32, H, C, D, concat, root)
            bwd = lib.gcm_dense_transformer_edge_bwd_workspace_bytes(256, 128, 32, H, C, D, concat, root)
            assert fwd >= base + 256 * 128 * 4 * 2 * H * D                       # u and abar beside the edge-free set
            assert bwd >= 256 * 128 * 4 * (P + H * C + 2 * H * D)
            assert fwd < base + 256 * 128 * 128 * 4                              # nothing [B,N,N]-sized
            M, E = 512 * 512, 512 * 511
            base = lib.gcm_csr_transformerconv_fwd_workspace_bytes(M, E, 32, H, C, concat, root)
            fwd = lib.gcm_csr_transformer_edge_fwd_workspace_bytes(M, E, 32, H, C, D, concat, root)
            bwd = lib.gcm_csr_transformer_edge_bwd_workspace_bytes(M, E, 32, H, C, D, concat, root)
            assert base + M * 4 * 2 * H * D <= fwd < base + M * 4 * 2 * H * D + 4096
            assert bwd >= 4 * (M * (P + H * C + 2 * H * D) + 2 * E * H)
            no_edges = lib.gcm_csr_transformer_edge_bwd_workspace_bytes(M, 0, 32, H, C, D, concat, root)
            assert bwd - no_edges <= 4 * E * 2 * H + 512                         # per edge: alpha and dS [E,H] only
    assert lib.gcm_csr_transformer_edge_bwd_workspace_bytes(1000, 0, 32, 2, 16, 3, 1, 1) > 0
    assert lib.gcm_dense_transformer_edge_fwd_workspace_bytes(0, 128, 32, 1, 32, 3, 1, 1) == 0
    assert lib.gcm_dense_transformer_edge_bwd_workspace_bytes(4, 128, 32, 1, 32, 0, 1, 1) == 0
    assert lib.gcm_csr_transformer_edge_fwd_workspace_bytes(0, 0, 32, 1, 32, 3, 1, 1) == 0
    assert lib.gcm_csr_transformer_edge_bwd_workspace_bytes(8, -1, 32, 1, 32, 3, 1, 1) == 0


# ---- the per-edge restatement -----------------------------------------------------------------------
def _ref(case, dense=False, seed=0, **kw):
    M, E, Fi, H, C, D, opts = case
    torch.manual_seed(seed)
    cls = DenseTransformerEdgeRef if dense else TransformerEdgeRef
    return cls(Fi, C, heads=H, edge_dim=D, **{**opts, **kw}).double()


@pytest.mark.parametrize("zero", ["weight", "edge_attr"])
@pytest.mark.parametrize("kw", [dict(), dict(beta=True), dict(concat=False), dict(root_weight=False)], ids=str)
def test_without_an_edge_term_it_is_the_edge_free_restatement_bit_for_bit(zero, kw):
    case = SPARSE_CASES[0]
    x, ei, ea = sparse_case(*case)
    ref = _ref(case, **kw)
    with torch.no_grad():
        if zero == "weight":
            ref.lin_edge.weight.zero_()
        else:
            ea = torch.zeros_like(ea)
    ops = ref.operands()
    w_e = ops.pop("w_e")
    assert torch.equal(transformer_edge(x, ei, ea, w_e=w_e, **ops), TR.transformer(x, ei, **ops))
    B, N = 2, 12
    xd, adj, ead = dense_case(B, N, *case[2:6], pattern="lower")
    ead = ead if zero == "weight" else torch.zeros_like(ead)
    for add_loop in (False, True):
        assert torch.equal(dense_transformer_edge(xd, adj, ead, w_e=w_e, add_loop=add_loop, **ops),
                           TR.dense_transformer(xd, adj, add_loop=add_loop, **ops))


def test_it_is_the_layer_written_on_message_passing():
    case = SPARSE_CASES[0]
    M, E, Fi, H, C, D, _ = case
    x, ei, ea = sparse_case(*case)
    for concat in (True, False):
        ref = _ref(case, concat=concat)
        mp = mp_layer(MP.RefMessagePassing, MP.softmax)(Fi, C, heads=H, concat=concat, edge_dim=D).double()
        mp.load_state_dict(ref.state_dict())
        want, got = ref(x, ei, ea).detach(), mp(x, ei, ea).detach()
        assert float((want - got).abs().max()) <= 1e-12 * float(want.abs().max())


def _identity(F, D, H=1, **kw):
    """q = k = v = x (C = F, one head unless told), no biases, no skip, lin_edge.weight = ones."""
    ref = TransformerEdgeRef(F, F // H, heads=H, edge_dim=D, root_weight=False, **kw).double()
    with torch.no_grad():
        for lin in (ref.lin_query, ref.lin_key, ref.lin_value):
            lin.weight.copy_(torch.eye(F))
            lin.bias.zero_()
        ref.lin_edge.weight.fill_(1.0)
    return ref


def test_one_sink_two_sources_by_hand():
    """C = 1, D = 1, W_e = [1]: node 2 attends to 0 (a = 1) and 1 (a = -1).  s = x2 (x_j + a), alpha its softmax,
    o = sum alpha (x_j + a)."""
    x = torch.tensor([[1.0], [2.0], [0.5]], dtype=torch.float64)
    ei, ea = torch.tensor([[0, 1], [2, 2]]), torch.tensor([[1.0], [-1.0]], dtype=torch.float64)
    out = _identity(1, 1)(x, ei, ea)
    s0, s1 = 0.5 * (1 + 1), 0.5 * (2 - 1)
    a0 = math.exp(s0) / (math.exp(s0) + math.exp(s1))
    assert abs(float(out[2, 0]) - (a0 * 2 + (1 - a0) * 1)) < 1e-15
    assert float(out[0, 0]) == 0 and float(out[1, 0]) == 0           # no in-edge, no skip: exactly 0


def test_an_isolated_node_gives_exactly_the_skip_and_a_duplicate_is_two_terms():
    torch.manual_seed(3)
    ref = TransformerEdgeRef(4, 3, heads=2, edge_dim=2).double()
    x = torch.randn(5, 4, dtype=torch.float64)
    ei = torch.tensor([[0, 1, 1], [2, 2, 2]])
    ea = torch.randn(3, 2, dtype=torch.float64)
    ea[2] = ea[1]                                                     # edge 1 twice
    out = ref(x, ei, ea)
    assert torch.equal(out[4], ref.lin_skip(x)[4])
    # a duplicate weighs twice: the same as one term with its probability doubled
    H, C = 2, 3
    q, k, v = (lin(x).view(5, H, C) for lin in (ref.lin_query, ref.lin_key, ref.lin_value))
    e = ref.lin_edge(ea).view(3, H, C)
    s = ((q[2] * (k[ei[0]] + e)).sum(-1) / math.sqrt(C)).exp()          # [3, H]
    w = s / (s[0] + 2 * s[1])
    want = (w[0, :, None] * (v[0] + e[0]) + 2 * w[1, :, None] * (v[1] + e[1])).reshape(-1) + ref.lin_skip(x)[2]
    assert float((out[2] - want).abs().max()) < 1e-14


@pytest.mark.parametrize("kw", [dict(), dict(beta=True), dict(concat=False)], ids=str)
def test_dense_equals_sparse_on_the_same_edge_set(kw):
    case = (0, 0, 6, 2, 4, 3, {})
    B, N = 2, 9
    x, adj, ea = dense_case(B, N, *case[2:6], pattern="lower")
    dref, sref = _ref(case, dense=True, **kw), _ref(case, **kw)
    sref.load_state_dict(dref.state_dict())
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])
    nan_off = torch.where((adj != 0).unsqueeze(-1), ea, torch.full((), float("nan"), dtype=torch.float64))
    want = sref(x.view(B * N, -1), ei, ea[bb, ii, jj]).view(B, N, -1).detach()
    got = dref(x, adj, nan_off).detach()                              # the unset entries are not read
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_add_loop_reads_the_diagonal_feature():
    case = (0, 0, 6, 2, 4, 3, {})
    B, N = 2, 9
    x, adj, ea = dense_case(B, N, *case[2:6], pattern="band")
    ref = _ref(case, dense=True)
    idx = torch.arange(N)
    with_diag = adj.clone()
    with_diag[:, idx, idx] = 1
    assert torch.equal(ref(x, adj, ea, add_loop=True), ref(x, with_diag, ea))
    other = ea.clone()
    other[:, idx, idx] += 1.0
    assert not torch.equal(ref(x, adj, other, add_loop=True), ref(x, adj, ea, add_loop=True))
    assert not torch.equal(ref(x, adj, ea, add_loop=True)[:, 2], ref(x, adj, ea)[:, 2])      # row 2 was empty


# ---- the factored restatement (the kernels' algebra) -------------------------------------------------
_NAMES = {"wq": "lin_query.weight", "bq": "lin_query.bias", "wk": "lin_key.weight", "bk": "lin_key.bias",
          "wv": "lin_value.weight", "bv": "lin_value.bias", "w_e": "lin_edge.weight", "w_skip": "lin_skip.weight",
          "b_skip": "lin_skip.bias", "w_beta": "lin_beta.weight"}


@pytest.mark.parametrize("kw", [dict(), dict(beta=True), dict(concat=False), dict(concat=False, beta=True),
                                dict(root_weight=False), dict(bias=False)], ids=str)
@pytest.mark.parametrize("case", [SPARSE_CASES[0], SPARSE_CASES[2], SPARSE_CASES[6]], ids=lambda c: "-".join(map(str, c[:6])))
def test_factored_form_and_its_hand_written_backward(case, kw):
    """Outputs and every gradient against autograd of the per-edge form, float64: 1e-12 of the value's scale."""
    M, E, Fi, H, C, D, opts = case
    x, ei, ea = sparse_case(*case)
    ref = _ref(case, seed=4, **kw)
    g = torch.randn(M, H * C if ref.concat else C, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    xs, eas = x.clone().requires_grad_(), ea.clone().requires_grad_()
    want = ref(xs, ei, eas)
    want.backward(g)
    ops = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in ref.operands().items()}
    out, grads = factored(x, ei, ea, g, **ops)
    close = lambda a, b, what: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()) or pytest.fail(what)
    close(out, want.detach(), "out")
    close(grads.pop("x"), xs.grad, "x")
    close(grads.pop("edge_attr"), eas.grad, "edge_attr")
    params = dict(ref.named_parameters())
    assert {_NAMES[k] for k in grads} == set(params)
    for k, v in grads.items():
        want_g = params[_NAMES[k]].grad
        if k == "bk":                                                 # exactly 0 in exact arithmetic
            assert float(v.abs().max()) <= 1e-12 * float(params["lin_key.weight"].grad.abs().max())
            assert float(want_g.abs().max()) <= 1e-12 * float(params["lin_key.weight"].grad.abs().max())
        else:
            close(v, want_g, k)
