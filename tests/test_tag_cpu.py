"""DenseTAGConv / TAGConv host side: parameters, argument checks, the C ABI's validation, the restatement the GPU
tests compare against, checked against hand-computed answers in float64, and the conditioning of the small cases of
the GPU table.  No kernel runs."""
import pytest
import torch

import _tag_cases as cases
from _tag_restate import DenseTagRef, TagRef, dense_tag, inv_sqrt_degree, tag
from gcm.nn import DenseTAGConv, TAGConv     # noqa: F401  (without the layers nothing here is worth running)

_CLASSES = ["DenseTAGConv", "TAGConv"]
F64 = torch.float64


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def _keys(K, cin=4, cout=6, bias=True):
    keys = {f"lins.{k}.weight": (cout, cin) for k in range(K + 1)}
    if bias:
        keys["bias"] = (cout,)
    return keys


# ---- parameters -----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 3])
def test_parameters_and_state_dict_keys(K):
    from gcm import nn as G
    d, s = G.DenseTAGConv(4, 6, K), G.TAGConv(4, 6, K=K)
    for m in (d, s, DenseTagRef(4, 6, K), TagRef(4, 6, K)):
        assert _shapes(m) == _keys(K)
    for m in (d, s):
        assert (m.in_channels, m.out_channels, m.K, m.normalize) == (4, 6, K, True)
        assert len(m.lins) == K + 1 and all(type(lin) is torch.nn.Linear and lin.bias is None for lin in m.lins)
        assert float(m.bias.detach().abs().max()) == 0.0            # PyG: zeros
        assert not isinstance(m, (G.DenseGraphConv, G.GraphConv))
    assert repr(s) == f"TAGConv(4, 6, K={K})" and repr(d) == f"DenseTAGConv(4, 6, K={K})"


def test_default_K_is_three_and_arguments_go_by_position():
    from gcm import nn as G
    for cls in _CLASSES:
        assert getattr(G, cls)(4, 6).K == 3
        m = getattr(G, cls)(4, 6, 2, False, False)                  # in, out, K, bias, normalize
        assert (m.K, m.bias, m.normalize) == (2, None, False)


@pytest.mark.parametrize("cls", _CLASSES)
def test_bias_false_drops_the_key(cls):
    from gcm import nn as G
    assert _shapes(getattr(G, cls)(4, 6, 3, bias=False)) == _keys(3, bias=False)
    assert _shapes(DenseTagRef(4, 6, 3, bias=False)) == _keys(3, bias=False)


def test_dense_and_sparse_load_each_other():
    from gcm import nn as G
    d, s = G.DenseTAGConv(4, 6, 2), G.TAGConv(4, 6, 2)
    with torch.no_grad():
        d.bias.uniform_(-1, 1)
    s.load_state_dict(d.state_dict())
    for k, v in d.state_dict().items():
        assert torch.equal(s.state_dict()[k], v)
    d2 = G.DenseTAGConv(4, 6, 2)
    d2.load_state_dict(s.state_dict())
    assert torch.equal(d2.lins[2].weight, d.lins[2].weight) and torch.equal(d2.bias, d.bias)
    DenseTagRef(4, 6, 2).load_state_dict(d.state_dict())
    TagRef(4, 6, 2).load_state_dict(s.state_dict())


@pytest.mark.parametrize("cls", _CLASSES)
def test_reset_parameters(cls):
    from gcm import nn as G
    conv = getattr(G, cls)(16, 8, 2)
    with torch.no_grad():
        for p in conv.parameters():
            p.fill_(9.0)
    conv.reset_parameters()
    assert float(conv.bias.detach().abs().max()) == 0.0
    for lin in conv.lins:                                           # torch.nn.Linear's own init: U(-1/4, 1/4) at 16 in
        assert 0.1 < float(lin.weight.detach().abs().max()) <= 0.25
    getattr(G, cls)(4, 4, 0, bias=False).reset_parameters()


def test_stacks_take_the_layered_and_generic_paths():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    dense = G.Sequential("x, adj, weights, B, N", [(G.DenseTAGConv(8, 8, 2), "x, adj -> x"), torch.nn.Tanh(),
                                                   (G.DenseTAGConv(8, 8, 1), "x, adj -> x")])
    assert DenseGCM(dense, edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is None
    sparse = G.Sequential("x, edges, weights", [(G.TAGConv(8, 8, 2), "x, edges, weights -> x"), torch.nn.Tanh(),
                                                (G.TAGConv(8, 8, 1), "x, edges, weights -> x")])
    mem = SparseGCM(sparse, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()


# ---- argument errors --------------------------------------------------------------------------------
def test_argument_errors():
    from gcm import nn as G, _hip
    x, ei = torch.zeros(3, 4), torch.tensor([[0, 1], [1, 2]])
    for cls in _CLASSES:
        with pytest.raises(ValueError, match="K must be at least 0"):
            getattr(G, cls)(4, 4, K=-1)
    with pytest.raises(TypeError, match="adj must be float32"):
        G.DenseTAGConv(4, 4, 1)(torch.zeros(1, 3, 4), torch.zeros(1, 3, 3, dtype=torch.float64))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.DenseTAGConv(4, 4, 1)(x, torch.ones(3, 3))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.TAGConv(4, 4, 1)(x, ei)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.TAGConv(4, 4, 0)(x, ei, torch.ones(2))
    with pytest.raises(NotImplementedError, match="GATv2Conv is not implemented"):
        G.GATv2Conv(3, 4)                                           # the placeholder stays


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_dense_tagconv_fwd", "gcm_dense_tagconv_fwd_workspace_bytes", "gcm_dense_tagconv_bwd",
              "gcm_dense_tagconv_bwd_workspace_bytes", "gcm_csr_tagconv_fwd", "gcm_csr_tagconv_fwd_workspace_bytes",
              "gcm_csr_tagconv_bwd", "gcm_csr_tagconv_bwd_workspace_bytes"}


def test_library_exports_every_symbol_of_the_tag_header():
    """include/gcm_hip_tag.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_tag.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_tag.h"))) - {"gcm_gcn_norm"}
    assert declared == set(_hip.TAG_PROTOTYPES) == _FUNCTIONS
    assert not declared & (set(_hip.PROTOTYPES) | set(_hip.GATED_PROTOTYPES) | set(_hip.RESGATED_PROTOTYPES))
    lib = _hip.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == _hip.TAG_PROTOTYPES[name][1]
    assert lib.gcm_abi_version() == 8                               # the section is additive


def test_c_abi_rejects_null_pointers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_tagconv_fwd(*([None] * 6), 0, 1, 1, 1, 1, 1, 1, 0, None) == -1
    assert lib.gcm_dense_tagconv_bwd(*([None] * 10), 0, 1, 1, 1, 1, 1, 1, 0, None) == -1
    assert lib.gcm_csr_tagconv_fwd(*([None] * 8), 0, 1, 0, 1, 1, 1, None) == -1
    assert lib.gcm_csr_tagconv_bwd(*([None] * 17), 0, 1, 0, 1, 1, 1, 1, None) == -1


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    for K in (1, 3):
        assert lib.gcm_dense_tagconv_fwd_workspace_bytes(256, 128, 32, K) > 0           # cfg2's dense shape
        assert lib.gcm_dense_tagconv_bwd_workspace_bytes(256, 128, 32, 32, K) > 0
        assert lib.gcm_csr_tagconv_fwd_workspace_bytes(512 * 512, 32, K) > 0            # cfg4's sparse graph
        assert lib.gcm_csr_tagconv_bwd_workspace_bytes(512 * 512, 512 * 511, 32, 32, K) > 0
    assert lib.gcm_csr_tagconv_bwd_workspace_bytes(1000, 0, 32, 32, 2) > 0              # no edges: still rows
    assert lib.gcm_dense_tagconv_bwd_workspace_bytes(4, 16, 8, 8, 0) > 0                # K = 0: the linear layer
    # what is saved: h_1 .. h_K and, dense, d
    for B, N, Fi, K in ((256, 128, 32, 3), (3, 50, 33, 2), (2, 130, 128, 1), (2, 9, 5, 0)):
        R = B * N
        assert lib.gcm_dense_tagconv_fwd_workspace_bytes(B, N, Fi, K) == 4 * (K * R * Fi + R)
        assert lib.gcm_csr_tagconv_fwd_workspace_bytes(R, Fi, K) == max(4 * K * R * Fi, 256)
    for dims in ((0, 128, 32, 2), (4, 0, 32, 2), (4, 128, 0, 2), (4, 128, 32, -1)):     # an empty problem
        assert lib.gcm_dense_tagconv_fwd_workspace_bytes(*dims) == 0
        assert lib.gcm_dense_tagconv_bwd_workspace_bytes(*dims[:3], 32, dims[3]) == 0
    assert lib.gcm_csr_tagconv_fwd_workspace_bytes(0, 32, 2) == 0
    assert lib.gcm_csr_tagconv_bwd_workspace_bytes(0, 0, 32, 32, 2) == 0


# ---- the restatement against hand-computed answers, in float64 ---------------------------------------
def _w(*values):
    """1 x 1 hop matrices."""
    return [torch.tensor([[v]], dtype=F64) for v in values]


_PATH = torch.tensor([[0, 1], [1, 2]])                              # 0 -> 1 -> 2


def _dense_of(ei, M, w=None):
    adj = torch.zeros(M, M, dtype=F64)
    w = torch.ones(ei.shape[1], dtype=F64) if w is None else w
    adj.index_put_((ei[1], ei[0]), w, accumulate=True)              # adj[i, j]: j -> i, duplicates summed
    return adj


def test_restatement_path_by_hand():
    """K = 2 on 0 -> 1 -> 2 with x = (1, 2, 4) and W = (1, 10, 100).  Plain: h_1 = (0, 1, 2), h_2 = (0, 0, 1).
    Normalised: deg = (0, 1, 1), d = (0, 1, 1), so the edge out of node 0 has coefficient 0: the source without
    in-edges contributes nothing; h_1 = (0, 0, 2), h_2 = 0."""
    x = torch.tensor([[1.0], [2.0], [4.0]], dtype=F64)
    W = _w(1, 10, 100)
    plain, normed = [[1.0], [12.0], [124.0]], [[1.0], [2.0], [24.0]]
    assert torch.equal(tag(x, _PATH, W, normalize=False), torch.tensor(plain, dtype=F64))
    assert torch.equal(tag(x, _PATH, W, normalize=True), torch.tensor(normed, dtype=F64))
    adj = _dense_of(_PATH, 3)
    assert torch.equal(dense_tag(x, adj, W, normalize=False)[0], torch.tensor(plain, dtype=F64))
    assert torch.equal(dense_tag(x, adj, W, normalize=True)[0], torch.tensor(normed, dtype=F64))
    bias = torch.tensor([0.5], dtype=F64)
    assert torch.equal(tag(x, _PATH, W, bias), torch.tensor(normed, dtype=F64) + 0.5)
    assert torch.equal(tag(x, _PATH, W[:1], bias), x + 0.5)         # K = 0: the linear layer


def test_restatement_duplicates_and_a_kept_self_loop_by_hand():
    """Edges 0 -> 0 (weight 4), 0 -> 1 twice (weight 1 each), x = (2, 0), W = (1, 1), K = 1.  deg = (4, 2), d = (1/2,
    1/sqrt 2); the loop is an ordinary edge with coefficient 1/2 * 4 * 1/2 = 1, each duplicate has 1 / (2 sqrt 2) and
    both count: h_1 = (2, sqrt 2), out = (4, sqrt 2).  Plain: h_1 = (8, 4), out = (10, 4)."""
    ei = torch.tensor([[0, 0, 0], [0, 1, 1]])
    w = torch.tensor([4.0, 1.0, 1.0], dtype=F64)
    x = torch.tensor([[2.0], [0.0]], dtype=F64)
    want = torch.tensor([[4.0], [2.0 ** 0.5]], dtype=F64)
    torch.testing.assert_close(tag(x, ei, _w(1, 1), edge_weight=w), want, rtol=0, atol=1e-15)
    torch.testing.assert_close(dense_tag(x, _dense_of(ei, 2, w), _w(1, 1))[0], want, rtol=0, atol=1e-15)
    assert torch.equal(tag(x, ei, _w(1, 1), edge_weight=w, normalize=False), torch.tensor([[10.0], [4.0]], dtype=F64))
    # a weight vector of the wrong length is ignored: unit weights, deg = (1, 2), h_1 = (2, 2 * 2 / sqrt 2)
    got = tag(x, ei, _w(1, 1), edge_weight=torch.ones(5, dtype=F64))
    torch.testing.assert_close(got, torch.tensor([[4.0], [2.0 * 2.0 ** 0.5]], dtype=F64), rtol=0, atol=1e-15)


def test_restatement_add_loop_overwrites_a_weighted_diagonal_by_hand():
    """adj = [[5, 0], [3, 7]] with add_loop is [[1, 0], [3, 1]]: deg = (1, 4), d = (1, 1/2), A^ = [[1, 0], [3/2, 1/4]].
    x = (1, 2), W = (1, 10), K = 1: h_1 = (1, 2), out = (11, 22).  mask drops row 1."""
    adj = torch.tensor([[5.0, 0.0], [3.0, 7.0]], dtype=F64)
    x = torch.tensor([[1.0], [2.0]], dtype=F64)
    assert torch.equal(dense_tag(x, adj, _w(1, 10), add_loop=True)[0], torch.tensor([[11.0], [22.0]], dtype=F64))
    mask = torch.tensor([[True, False]])
    assert torch.equal(dense_tag(x, adj, _w(1, 10), mask=mask, add_loop=True)[0],
                       torch.tensor([[11.0], [0.0]], dtype=F64))
    # without add_loop the diagonal is an ordinary weighted entry: deg = (5, 10)
    d = torch.tensor([5.0, 10.0], dtype=F64) ** -0.5
    want = x + 10 * ((d[:, None] * adj * d[None, :]) @ x)
    torch.testing.assert_close(dense_tag(x, adj, _w(1, 10))[0], want, rtol=0, atol=1e-14)


def test_restatement_degree_zero():
    assert torch.equal(inv_sqrt_degree(torch.tensor([0.0, 4.0, 0.25], dtype=F64)),
                       torch.tensor([0.0, 0.5, 2.0], dtype=F64))
    deg = torch.tensor([0.0, 4.0], dtype=F64, requires_grad=True)
    inv_sqrt_degree(deg).sum().backward()
    assert float(deg.grad[0]) == 0.0                                # 0 at deg == 0, not NaN
    assert abs(float(deg.grad[1]) + 0.5 * 4.0 ** -1.5) < 1e-15


def test_restatement_dense_equals_sparse_on_the_same_weighted_edge_set():
    torch.manual_seed(3)
    B, N, Fi, Fo, K = 2, 9, 3, 4, 3
    adj = (torch.rand(B, N, N) < 0.3).to(F64) * (torch.rand(B, N, N, dtype=F64) + 0.1)
    adj[:, 2] = 0                                                   # a node without in-edges
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])
    x = torch.randn(B, N, Fi, dtype=F64)
    W = [torch.randn(Fo, Fi, dtype=F64) for _ in range(K + 1)]
    bias = torch.randn(Fo, dtype=F64)
    for normalize in (True, False):
        d = dense_tag(x, adj, W, bias, normalize=normalize)
        s = tag(x.view(B * N, Fi), ei, W, bias, adj[bb, ii, jj], normalize=normalize).view(B, N, Fo)
        torch.testing.assert_close(d, s, rtol=0, atol=1e-12)
    loops = torch.arange(B * N)
    with_loops = torch.cat([ei[:, ei[0] != ei[1]], torch.stack([loops, loops])], 1)
    wl = torch.cat([adj[bb, ii, jj][ei[0] != ei[1]], torch.ones(B * N, dtype=F64)])
    torch.testing.assert_close(dense_tag(x, adj, W, bias, add_loop=True),
                               tag(x.view(B * N, Fi), with_loops, W, bias, wl).view(B, N, Fo), rtol=0, atol=1e-12)


def test_restatement_gradients_are_finite_and_zero_degree_term_is_exactly_zero():
    """Row 1 of adj is empty, so deg_1 == 0 and d_1 == 0: every entry of that row has the gradient d_1 d_j G_1j plus
    the degree term of row 1, and both are exactly 0.  Elsewhere entries equal to 0 have a gradient too."""
    torch.manual_seed(5)
    N, Fi, Fo, K = 4, 2, 3, 2
    adj = torch.tensor([[0, 1, 0, 2], [0, 0, 0, 0], [1, 1, 3, 0], [0, 0.5, 1, 0]], dtype=F64).requires_grad_()
    x = torch.randn(1, N, Fi, dtype=F64, requires_grad=True)
    W = [torch.randn(Fo, Fi, dtype=F64) for _ in range(K + 1)]
    dense_tag(x, adj, W).square().sum().backward()
    assert torch.isfinite(adj.grad).all() and torch.isfinite(x.grad).all()
    assert torch.equal(adj.grad[1], torch.zeros(N, dtype=F64))
    assert float(adj.grad[0, 0].abs()) > 0 and float(adj.grad[3, 3].abs()) > 0          # zero entries of live rows
    adj2 = adj.detach().clone().requires_grad_()
    dense_tag(x, adj2, W, add_loop=True).square().sum().backward()
    assert torch.equal(adj2.grad.diagonal(), torch.zeros(N, dtype=F64))                 # an overwritten diagonal
    ei = torch.tensor([[1, 3, 0, 1, 2, 1, 2], [0, 0, 2, 2, 2, 3, 3]])
    ew = torch.tensor([1, 2, 1, 1, 3, 0.5, 1], dtype=F64, requires_grad=True)
    xs = x.detach()[0].clone().requires_grad_()
    tag(xs, ei, W, edge_weight=ew).square().sum().backward()
    assert torch.isfinite(ew.grad).all() and torch.isfinite(xs.grad).all()
    want = adj.grad[ei[1], ei[0]]                                   # the same graph: the same gradients per edge
    torch.testing.assert_close(ew.grad, want, rtol=0, atol=1e-12)


def test_restatement_gradcheck():
    torch.manual_seed(6)
    adj = (torch.rand(2, 5, 5) < 0.5).to(F64) * (torch.rand(2, 5, 5, dtype=F64) + 0.2)
    adj[:, :, 0] = 0.7                                              # every degree positive: differentiable around adj
    adj.requires_grad_()
    x = torch.randn(2, 5, 3, dtype=F64, requires_grad=True)
    W = [torch.randn(2, 3, dtype=F64, requires_grad=True) for _ in range(3)]
    assert torch.autograd.gradcheck(lambda x, adj, *W: dense_tag(x, adj, list(W)), (x, adj, *W))


# ---- the GPU table -----------------------------------------------------------------------------------
def test_case_table_holds_the_required_shapes():
    dense = {c[:5] for c in cases.DENSE_CASES}
    assert {(3, 7, 3, 5, 1), (3, 7, 3, 5, 3), (5, 1, 4, 3, 2), (2, 33, 8, 8, 2), (2, 40, 16, 12, 3), (2, 40, 6, 9, 0),
            (4, 128, 32, 32, 3), (2, 129, 32, 32, 3), (2, 70, 128, 128, 2), (2, 64, 64, 96, 4)} <= dense
    sparse = {c[:5] for c in cases.SPARSE_CASES}
    assert {(10, 30, 3, 5, 1), (40, 90, 8, 6, 3), (300, 900, 64, 32, 2), (50, 0, 4, 4, 2),
            (70, 400, 128, 128, 2)} <= sparse
    inp, _ = cases.dense_reference(6)                               # the band: node 0 has no in-edge
    assert float(inp["adj"][:, 0].abs().max()) == 0 and float(inp["adj"][0, 5, [4, 3, 1]].min()) == 1
    for case in cases.DENSE_CASES:
        assert float(cases.dense_inputs(case)["adj"].min()) >= 0    # non-negative weights


@pytest.mark.parametrize("index", [i for i, c in enumerate(cases.DENSE_CASES) if c[1] <= 64],
                         ids=lambda i: cases.case_id(cases.DENSE_CASES[i]))
def test_small_dense_cases_are_well_conditioned(index):
    _, res = cases.dense_reference(index)
    for k, v in cases.conditioning(res).items():
        assert v <= 1e-4, (k, v)


@pytest.mark.parametrize("index", [i for i, c in enumerate(cases.SPARSE_CASES) if c[0] <= 70],
                         ids=lambda i: cases.case_id(cases.SPARSE_CASES[i]))
def test_small_sparse_cases_are_well_conditioned(index):
    _, res = cases.sparse_reference(index)
    for k, v in cases.conditioning(res).items():
        assert v <= 1e-4, (k, v)
