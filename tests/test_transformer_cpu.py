"""DenseTransformerConv / TransformerConv host side: parameters, argument checks, the C ABI's validation and the
restatement the GPU tests compare against, pinned by hand-computed answers.  No kernel runs."""
import itertools
import math

import pytest
import torch

from _transformer_restate import DenseTransformerRef, TransformerRef, dense_transformer, transformer


# ---- parameters -----------------------------------------------------------------------------------
@pytest.mark.parametrize("concat,beta,root_weight,bias", list(itertools.product([True, False], repeat=4)))
def test_parameters(concat, beta, root_weight, bias):
    from gcm import nn as G
    F, C, H = 6, 5, 3
    D = H * C if concat else C
    want = {"lin_key.weight": (H * C, F), "lin_key.bias": (H * C,), "lin_query.weight": (H * C, F),
            "lin_query.bias": (H * C,), "lin_value.weight": (H * C, F), "lin_value.bias": (H * C,)}
    if root_weight:
        want["lin_skip.weight"] = (D, F)
        if bias:
            want["lin_skip.bias"] = (D,)
        if beta:
            want["lin_beta.weight"] = (1, 3 * D)
    d = G.DenseTransformerConv(F, C, heads=H, concat=concat, beta=beta, root_weight=root_weight, bias=bias)
    s = G.TransformerConv(F, C, heads=H, concat=concat, beta=beta, root_weight=root_weight, bias=bias)
    r = TransformerRef(F, C, heads=H, concat=concat, beta=beta, root_weight=root_weight, bias=bias)
    for m in (d, s, r):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert d.beta == s.beta == (beta and root_weight)         # beta is dropped without root_weight
    bound = 1 / math.sqrt(F)                                  # torch.nn.Linear's default init
    sd = s.state_dict()
    assert 0 < float(sd["lin_query.weight"].abs().max()) <= bound and 0 < float(sd["lin_key.bias"].abs().max()) <= bound
    d.load_state_dict(s.state_dict())                         # one loads the other's state_dict unchanged
    s.load_state_dict(G.DenseTransformerConv(F, C, heads=H, concat=concat, beta=beta, root_weight=root_weight,
                                             bias=bias).state_dict())
    DenseTransformerRef(F, C, heads=H, concat=concat, beta=beta, root_weight=root_weight,
                        bias=bias).load_state_dict(d.state_dict())
    for m in (d, s):
        assert not isinstance(m, (G.DenseGraphConv, G.GraphConv))


def test_stacks_take_the_layered_and_generic_paths():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    dense = G.Sequential("x, adj, weights, B, N", [(G.DenseTransformerConv(4, 8), "x, adj -> x"), torch.nn.Tanh(),
                                                   (G.DenseTransformerConv(8, 8), "x, adj -> x"), torch.nn.Tanh()])
    assert DenseGCM(dense, edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is None
    sparse = G.Sequential("x, edges, weights", [(G.TransformerConv(4, 8), "x, edges, weights -> x"), torch.nn.Tanh(),
                                                (G.TransformerConv(8, 8), "x, edges, weights -> x")])
    mem = SparseGCM(sparse, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()


# ---- argument errors --------------------------------------------------------------------------------
def test_argument_errors():
    from gcm import nn as G, _hip
    x, ei = torch.zeros(3, 2), torch.tensor([[0, 1], [1, 2]])
    for conv, args in ((G.TransformerConv(2, 2, dropout=0.5), (x, ei)),
                       (G.DenseTransformerConv(2, 2, dropout=0.5), (x, torch.ones(3, 3)))):
        with pytest.raises(NotImplementedError, match="dropout"):
            conv(*args)
        conv.eval()                                   # dropout is a no-op in eval mode: the call reaches the kernels
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            conv(*args)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.TransformerConv(2, 2, dropout=0.0)(x, ei, torch.zeros(2, 3))
    with pytest.raises(NotImplementedError, match="edge_dim"):
        G.TransformerConv(2, 2, edge_dim=3)
    with pytest.raises(NotImplementedError, match="return_attention_weights"):
        G.TransformerConv(2, 2)(x, ei, return_attention_weights=True)
    for cls in (G.TransformerConv, G.DenseTransformerConv):
        with pytest.raises(NotImplementedError, match="tuple"):
            cls((2, 3), 2)
    with pytest.raises(TypeError):
        G.DenseTransformerConv(2, 2)(torch.zeros(1, 3, 2), torch.zeros(1, 3, 3, dtype=torch.float64))


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {
    "gcm_dense_transformerconv_fwd_workspace_bytes", "gcm_dense_transformerconv_fwd",
    "gcm_dense_transformerconv_bwd_workspace_bytes", "gcm_dense_transformerconv_bwd",
    "gcm_csr_transformerconv_fwd_workspace_bytes", "gcm_csr_transformerconv_fwd",
    "gcm_csr_transformerconv_bwd_workspace_bytes", "gcm_csr_transformerconv_bwd"}


def test_library_exports_every_symbol_of_the_transformer_header():
    """include/gcm_hip_transformer.h is a section gcm_hip.h includes: every function it declares is exported and
    bound."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_transformer.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_transformer.h")))
    assert declared == set(_hip.TRANSFORMER_PROTOTYPES) == _FUNCTIONS
    assert not declared & (set(_hip.PROTOTYPES) | set(_hip.AGGR_PROTOTYPES) | set(_hip.LEARNED_DET_PROTOTYPES))
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == _hip.TRANSFORMER_PROTOTYPES[name][1]
    assert lib.gcm_abi_version() == 8                         # the section is additive


def test_c_abi_rejects_null_pointers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_transformerconv_fwd(*([None] * 7), 0, 1, 1, 1, 1, 1, 1, 1, 0, None) == -1
    assert lib.gcm_dense_transformerconv_bwd(*([None] * 10), 0, 1, 1, 1, 1, 1, 1, 1, None) == -1
    assert lib.gcm_csr_transformerconv_fwd(*([None] * 8), 0, 1, 0, 1, 1, 1, 1, 1, None) == -1
    assert lib.gcm_csr_transformerconv_bwd(*([None] * 15), 0, 1, 0, 1, 1, 1, 1, 1, None) == -1


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    for concat, root in itertools.product((0, 1), repeat=2):
        for H, C in ((1, 32), (4, 8)):
            # cfg2's dense shape (B 256, N 128, F 32) and cfg4's sparse one (512 graphs x 512 nodes, one edge each)
            fwd = lib.gcm_dense_transformerconv_fwd_workspace_bytes(256, 128, 32, H, C, concat, root)
            bwd = lib.gcm_dense_transformerconv_bwd_workspace_bytes(256, 128, 32, H, C, concat, root)
            P = 3 * H * C + ((H * C if concat else C) if root else 0)
            assert fwd >= 256 * 128 * 4 * (P + H * C + 2 * H + 1 + 4) and bwd >= 256 * 128 * 4 * (P + H * C)
            M, E = 512 * 512, 512 * 511
            fwd = lib.gcm_csr_transformerconv_fwd_workspace_bytes(M, E, 32, H, C, concat, root)
            bwd = lib.gcm_csr_transformerconv_bwd_workspace_bytes(M, E, 32, H, C, concat, root)
            assert fwd >= M * 4 * (P + H * C + 2 * H) and bwd >= 4 * (M * (P + H * C) + 2 * E * H)
    assert lib.gcm_csr_transformerconv_bwd_workspace_bytes(1000, 0, 32, 2, 16, 1, 1) > 0     # no edges: still rows
    assert lib.gcm_dense_transformerconv_fwd_workspace_bytes(0, 128, 32, 1, 32, 1, 1) == 0
    assert lib.gcm_dense_transformerconv_bwd_workspace_bytes(0, 128, 32, 1, 32, 1, 1) == 0
    assert lib.gcm_csr_transformerconv_fwd_workspace_bytes(0, 0, 32, 1, 32, 1, 1) == 0
    assert lib.gcm_csr_transformerconv_bwd_workspace_bytes(0, 0, 32, 1, 32, 1, 1) == 0


# ---- the restatement against hand-computed answers (identity projections, no biases) ----------------
def _d(v):
    return torch.tensor(v, dtype=torch.float64)


def _softmax_sum(es, vs):
    w = [math.exp(e) for e in es]
    return sum(a * v for a, v in zip(w, vs)) / sum(w)


def _eye(n):
    I = torch.eye(n, dtype=torch.float64)
    return I, None, I, None, I, None                  # wq, bq, wk, bk, wv, bv


def test_restatement_two_heads():
    # heads 2, C = 1, identity projections: q = k = v = x, s_ijh = x_ih x_jh.  Edges 0 -> 2, 1 -> 2, 0 -> 1.
    x = _d([[1.0, 0.5], [0.0, 1.0], [-1.0, 2.0]])
    ei = torch.tensor([[0, 1, 0], [2, 2, 1]])
    out = transformer(x, ei, *_eye(2), heads=2)
    want = [[0.0, 0.0],                                                   # no in-edge: aggregates nothing
            [1.0, 0.5],                                                   # one neighbour: its value
            [_softmax_sum([-1.0 * 1.0, -1.0 * 0.0], [1.0, 0.0]), _softmax_sum([2.0 * 0.5, 2.0 * 1.0], [0.5, 1.0])]]
    assert torch.allclose(out, _d(want))
    adj = _d([[0, 0, 0], [1, 0, 0], [1, 1, 0]])
    assert torch.allclose(dense_transformer(x, adj, *_eye(2), heads=2)[0], out)


def test_restatement_scores_are_scaled_by_sqrt_c():
    # one head, C = 4: s = <q, k> / 2
    x = _d([[1.0, 1.0, 1.0, 1.0], [2.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 3.0]])
    ei = torch.tensor([[0, 1], [2, 2]])
    out = transformer(x, ei, *_eye(4))
    w0, w1 = math.exp(3.0 / 2), math.exp(0.0)
    assert torch.allclose(out[2], (w0 * x[0] + w1 * x[1]) / (w0 + w1))


def test_restatement_duplicates_and_loops_are_ordinary_terms():
    # node 1: a loop twice and 0 -> 1: three terms; no loop is added for node 0, which has no in-edge
    x = _d([[2.0], [-1.0]])
    ei = torch.tensor([[1, 1, 0], [1, 1, 1]])
    out = transformer(x, ei, *_eye(1))
    assert torch.allclose(out[1], _d([_softmax_sum([1.0, 1.0, -2.0], [-1.0, -1.0, 2.0])]))
    assert torch.equal(out[0], _d([0.0]))


def test_restatement_isolated_node_gives_exactly_the_skip():
    x = _d([[1.0, -2.0], [2.0, 0.5], [3.0, 1.0]])
    w_skip, b_skip = _d([[0.5, 1.0], [-1.0, 0.25]]), _d([0.25, -0.5])
    out = transformer(x, torch.tensor([[0], [1]]), *_eye(2), w_skip, b_skip)
    r = x @ w_skip.t() + b_skip
    assert torch.equal(out[0], r[0]) and torch.equal(out[2], r[2])
    assert torch.allclose(out[1], x[0] + r[1])
    adj = _d([[0, 0, 0], [1, 0, 0], [0, 0, 0]])
    dense = dense_transformer(x, adj, *_eye(2), w_skip, b_skip)[0]
    assert torch.equal(dense, out) and not torch.isnan(dense).any()
    assert torch.equal(transformer(x, torch.tensor([[0], [1]]), *_eye(2))[0], _d([0.0, 0.0]))   # no root: 0


def test_restatement_beta_gate_on_one_node():
    # one node with a loop: o = v = 2, r = 0.5 * 2 = 1, logit = 0.3 o - 0.2 r + 0.7 (o - r) = 1.1
    x = _d([[2.0]])
    out = transformer(x, torch.tensor([[0], [0]]), *_eye(1), _d([[0.5]]), None, _d([[0.3, -0.2, 0.7]]))
    b = 1 / (1 + math.exp(-1.1))
    assert torch.allclose(out, _d([[b * 1.0 + (1 - b) * 2.0]]))
    # an isolated node under the gate: o = 0, logit = -0.2 r - 0.7 r
    out = transformer(x, torch.zeros(2, 0, dtype=torch.long), *_eye(1), _d([[0.5]]), None, _d([[0.3, -0.2, 0.7]]))
    assert torch.allclose(out, _d([[1 / (1 + math.exp(0.9))]]))


@pytest.mark.parametrize("heads,concat,beta,root", [(2, True, False, True), (3, False, True, True),
                                                    (2, True, True, True), (2, False, False, False)])
def test_dense_equals_sparse_on_the_same_edge_set(heads, concat, beta, root):
    torch.manual_seed(1)
    B, N, F, C = 2, 7, 3, 4
    ref = DenseTransformerRef(F, C, heads=heads, concat=concat, beta=beta, root_weight=root).double()
    sref = TransformerRef(F, C, heads=heads, concat=concat, beta=beta, root_weight=root).double()
    sref.load_state_dict(ref.state_dict())
    adj = (torch.rand(B, N, N) < 0.4).double() * (torch.rand(B, N, N).double() - 0.5)    # pattern only
    adj[:, 2] = 0                                                                         # an empty row
    x = torch.randn(B, N, F, dtype=torch.float64)
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])
    d = ref(x, adj)
    s = sref(x.view(B * N, F), ei).view(B, N, -1)
    assert torch.allclose(d, s) and not torch.isnan(d).any()
    mask = torch.rand(B, N) < 0.5
    assert torch.equal(ref(x, adj, mask), d * mask.unsqueeze(-1))


def test_restatement_add_loop_overwrites_weighted_diagonal():
    torch.manual_seed(2)
    x = torch.randn(3, 2, dtype=torch.float64)
    weighted = _d([[5.0, 0.0, 2.5], [0.1, -7.0, 0.0], [0.0, 3.0, 0.0]])
    pattern = _d([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])
    got = dense_transformer(x, weighted, *_eye(2), add_loop=True)
    assert torch.equal(got, dense_transformer(x, pattern, *_eye(2)))
    # node 2 has a zero diagonal: without add_loop it attends to node 1 only
    assert torch.allclose(dense_transformer(x, weighted, *_eye(2))[0, 2], x[1])
    s21, s22 = float(x[2] @ x[1]) / math.sqrt(2), float(x[2] @ x[2]) / math.sqrt(2)
    want = [_softmax_sum([s21, s22], [float(x[1, c]), float(x[2, c])]) for c in range(2)]
    assert torch.allclose(got[0, 2], _d(want))


def test_restatement_concat_false_is_the_mean_over_heads():
    torch.manual_seed(3)
    x = torch.randn(5, 6, dtype=torch.float64)
    ei = torch.tensor([[0, 1, 2, 3, 3], [4, 4, 4, 0, 0]])
    cat = transformer(x, ei, *_eye(6), heads=3)
    mean = transformer(x, ei, *_eye(6), heads=3, concat=False)
    assert torch.allclose(mean, cat.view(5, 3, 2).mean(1))
    # heads 2, C = 1 by hand: node 2 attends to 0 and 1
    x = _d([[1.0, 0.5], [0.0, 1.0], [-1.0, 2.0]])
    out = transformer(x, torch.tensor([[0, 1], [2, 2]]), *_eye(2), heads=2, concat=False)
    want = (_softmax_sum([-1.0, 0.0], [1.0, 0.0]) + _softmax_sum([1.0, 2.0], [0.5, 1.0])) / 2
    assert torch.allclose(out[2], _d([want]))
