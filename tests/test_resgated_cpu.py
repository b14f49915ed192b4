"""DenseResGatedGraphConv / ResGatedGraphConv host side: parameters, argument checks, the C ABI's validation and the
restatement the GPU tests compare against, checked against itself in float64.  No kernel runs."""
import pytest
import torch

from _resgated_restate import (DenseResGatedRef, ResGatedRef, dense_resgated, dense_resgated_adj_grad, resgated)

_CLASSES = ["DenseResGatedGraphConv", "ResGatedGraphConv"]
_KEYS = {"lin_key.weight": (4, 3), "lin_key.bias": (4,), "lin_query.weight": (4, 3), "lin_query.bias": (4,),
         "lin_value.weight": (4, 3), "lin_value.bias": (4,), "lin_skip.weight": (4, 3), "bias": (4,)}


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


# ---- parameters -----------------------------------------------------------------------------------
def test_parameters_and_state_dict_keys():
    from gcm import nn as G
    d, s = G.DenseResGatedGraphConv(3, 4), G.ResGatedGraphConv(3, 4)
    for m in (d, s, DenseResGatedRef(3, 4), ResGatedRef(3, 4)):
        assert _shapes(m) == _KEYS
    assert set(d.state_dict()) == set(s.state_dict())
    for m in (d, s):
        assert (m.in_channels, m.out_channels, m.root_weight) == (3, 4, True)
        assert isinstance(m.act, torch.nn.Sigmoid)
        assert float(m.bias.detach().abs().max()) == 0.0                 # zeroed by reset_parameters()
        assert not isinstance(m, (G.DenseGraphConv, G.GraphConv))
    assert s.edge_dim is None
    assert repr(d) == "DenseResGatedGraphConv(3, 4)" and repr(s) == "ResGatedGraphConv(3, 4)"


def test_constructor_arguments_by_position():
    from gcm import nn as G
    s = G.ResGatedGraphConv(3, 4, torch.nn.Sigmoid(), None, False, False)     # act, edge_dim, root_weight, bias
    assert not s.root_weight and s.bias is None and s.lin_skip is None
    d = G.DenseResGatedGraphConv(3, 4, None, False, False)                    # act, root_weight, bias
    assert not d.root_weight and d.bias is None and d.lin_skip is None


@pytest.mark.parametrize("cls", _CLASSES)
def test_root_weight_and_bias_drop_their_keys(cls):
    from gcm import nn as G
    conv = getattr(G, cls)
    assert set(conv(3, 4, root_weight=False).state_dict()) == set(_KEYS) - {"lin_skip.weight"}
    assert set(conv(3, 4, bias=False).state_dict()) == set(_KEYS) - {"bias"}
    assert set(conv(3, 4, root_weight=False, bias=False).state_dict()) == set(_KEYS) - {"lin_skip.weight", "bias"}
    assert set(DenseResGatedRef(3, 4, root_weight=False, bias=False).state_dict()) == \
        set(_KEYS) - {"lin_skip.weight", "bias"}


def test_dense_and_sparse_load_each_other():
    from gcm import nn as G
    d, s = G.DenseResGatedGraphConv(3, 4), G.ResGatedGraphConv(3, 4)
    with torch.no_grad():
        d.bias.fill_(0.5)
    s.load_state_dict(d.state_dict())
    for k, v in d.state_dict().items():
        assert torch.equal(s.state_dict()[k], v)
    d2 = G.DenseResGatedGraphConv(3, 4)
    d2.load_state_dict(s.state_dict())
    assert torch.equal(d2.lin_skip.weight, d.lin_skip.weight) and float(d2.bias[0].detach()) == 0.5
    DenseResGatedRef(3, 4).load_state_dict(d.state_dict())
    ResGatedRef(3, 4).load_state_dict(s.state_dict())


@pytest.mark.parametrize("cls", _CLASSES)
def test_reset_parameters(cls):
    from gcm import nn as G
    conv = getattr(G, cls)(3, 4)
    with torch.no_grad():
        for p in conv.parameters():
            p.fill_(9.0)
    conv.reset_parameters()
    assert float(conv.bias.detach().abs().max()) == 0.0
    for lin in (conv.lin_key, conv.lin_query, conv.lin_value, conv.lin_skip):
        for p in lin.parameters():
            assert float(p.detach().abs().max()) < 1.0            # torch.nn.Linear's init: within 1 / sqrt(fan_in)
    getattr(G, cls)(3, 4, root_weight=False, bias=False).reset_parameters()


def test_stacks_take_the_layered_and_generic_paths():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    dense = G.Sequential("x, adj, weights, B, N", [(G.DenseResGatedGraphConv(4, 8), "x, adj -> x"), torch.nn.Tanh(),
                                                   (G.DenseResGatedGraphConv(8, 8), "x, adj -> x"), torch.nn.Tanh()])
    assert DenseGCM(dense, edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is None
    sparse = G.Sequential("x, edges, weights", [(G.ResGatedGraphConv(4, 8), "x, edges, weights -> x"),
                                                torch.nn.Tanh(),
                                                (G.ResGatedGraphConv(8, 8), "x, edges, weights -> x")])
    mem = SparseGCM(sparse, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()


# ---- argument errors --------------------------------------------------------------------------------
def test_not_implemented_arguments_are_named():
    from gcm import nn as G
    with pytest.raises(NotImplementedError, match="edge_dim"):
        G.ResGatedGraphConv(3, 4, edge_dim=2)
    for cls in _CLASSES:
        with pytest.raises(NotImplementedError, match="in_channels"):
            getattr(G, cls)((3, 3), 4)
        for act in (torch.nn.ReLU(), torch.nn.Tanh(), torch.sigmoid, "sigmoid"):
            with pytest.raises(NotImplementedError, match="act"):
                getattr(G, cls)(3, 4, act=act)
        getattr(G, cls)(3, 4, act=torch.nn.Sigmoid())
    with pytest.raises(TypeError):
        G.DenseResGatedGraphConv(3, 4, edge_dim=None)             # the dense twin has no edge_dim
    with pytest.raises(NotImplementedError, match="GATv2Conv is not implemented"):
        G.GATv2Conv(3, 4)                                         # the placeholder stays


def test_argument_errors_of_a_call():
    from gcm import nn as G, _hip
    x, ei = torch.zeros(3, 3), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(TypeError, match="adj must be float32"):
        G.DenseResGatedGraphConv(3, 4)(torch.zeros(1, 3, 3), torch.zeros(1, 3, 3, dtype=torch.float64))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.DenseResGatedGraphConv(3, 4)(x, torch.ones(3, 3))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.ResGatedGraphConv(3, 4)(x, ei)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.ResGatedGraphConv(3, 4)(x, ei, torch.ones(2))           # edge_attr is accepted


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_dense_resgatedconv_fwd", "gcm_dense_resgatedconv_fwd_workspace_bytes",
              "gcm_dense_resgatedconv_bwd", "gcm_dense_resgatedconv_bwd_workspace_bytes",
              "gcm_csr_resgatedconv_fwd", "gcm_csr_resgatedconv_fwd_workspace_bytes",
              "gcm_csr_resgatedconv_bwd", "gcm_csr_resgatedconv_bwd_workspace_bytes"}


def test_library_exports_every_symbol_of_the_resgated_header():
    """include/gcm_hip_resgated.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_resgated.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    assert hasattr(_hip, "RESGATED_PROTOTYPES")
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_resgated.h")))
    assert declared == set(_hip.RESGATED_PROTOTYPES) == _FUNCTIONS
    assert not declared & (set(_hip.PROTOTYPES) | set(_hip.AGGR_PROTOTYPES) | set(_hip.LEARNED_DET_PROTOTYPES)
                           | set(_hip.TRANSFORMER_PROTOTYPES) | set(_hip.RESET_PROTOTYPES) | set(_hip.GIN_PROTOTYPES)
                           | set(_hip.BPTT_HOPS_PROTOTYPES))
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == _hip.RESGATED_PROTOTYPES[name][1]
    assert lib.gcm_abi_version() == 8                         # the section is additive
    assert len(_hip.PROTOTYPES) == 150


def test_c_abi_rejects_null_pointers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_resgatedconv_fwd(*([None] * 7), 0, 1, 1, 1, 1, 1, 0, None) == -1
    assert lib.gcm_dense_resgatedconv_bwd(*([None] * 11), 0, 1, 1, 1, 1, 1, 0, None) == -1
    assert lib.gcm_csr_resgatedconv_fwd(*([None] * 8), 0, 1, 0, 1, 1, 1, None) == -1
    assert lib.gcm_csr_resgatedconv_bwd(*([None] * 13), 0, 1, 0, 1, 1, 1, None) == -1


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    for root in (0, 1):
        assert lib.gcm_dense_resgatedconv_fwd_workspace_bytes(256, 128, 32, 32, root) > 0     # cfg2's dense shape
        assert lib.gcm_dense_resgatedconv_bwd_workspace_bytes(256, 128, 32, 32, root) > 0
        assert lib.gcm_csr_resgatedconv_fwd_workspace_bytes(512 * 512, 512 * 511, 32, 32, root) > 0   # cfg4's sparse
        assert lib.gcm_csr_resgatedconv_bwd_workspace_bytes(512 * 512, 512 * 511, 32, 32, root) > 0
    assert lib.gcm_csr_resgatedconv_bwd_workspace_bytes(1000, 0, 32, 32, 1) > 0               # no edges: still rows
    # what is saved is the projections and the bit image, nothing per gate: [R, 4 C] floats + [R, N / 32] words
    R = 256 * 128
    assert lib.gcm_dense_resgatedconv_fwd_workspace_bytes(256, 128, 32, 32, 1) == R * 128 * 4 + R * 4 * 4
    assert lib.gcm_dense_resgatedconv_fwd_workspace_bytes(0, 128, 32, 32, 1) == 0
    assert lib.gcm_csr_resgatedconv_bwd_workspace_bytes(0, 0, 32, 32, 1) == 0


# ---- the restatement against itself, in float64 -----------------------------------------------------
def _operands(Fi, C, seed):
    gen = torch.Generator().manual_seed(seed)

    def r(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64)
    return [r(C, Fi), r(C), r(C, Fi), r(C), r(C, Fi), r(C), r(C, Fi), r(C)]     # key, query, value (w, b), skip, bias


def test_restatement_by_hand():
    # one channel, identity weights: 0 -> 1 twice and the loop 1 -> 1; node 0 has no in-edge
    one, zero = torch.ones(1, 1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    x = torch.tensor([[2.0], [-1.0]], dtype=torch.float64)
    ei = torch.tensor([[0, 0, 1], [1, 1, 1]])
    got = resgated(x, ei, one, zero, one, zero, one, zero, 3 * one, zero + 0.5)
    sig = torch.sigmoid(torch.tensor([-1.0 + 2.0, -1.0 - 1.0], dtype=torch.float64))
    want = torch.stack([3 * x[0] + 0.5, 3 * x[1] + 0.5 + 2 * sig[0] * 2.0 + sig[1] * -1.0])
    assert torch.allclose(got, want, rtol=0, atol=1e-15)
    adj = torch.tensor([[0.0, 0.0], [2.0, 1.0]], dtype=torch.float64)        # the duplicate as a weight of 2
    assert torch.allclose(dense_resgated(x, adj, one, zero, one, zero, one, zero, 3 * one, zero + 0.5)[0], want,
                          rtol=0, atol=1e-15)


def test_restatement_dense_equals_sparse_on_the_same_edge_set():
    torch.manual_seed(1)
    B, N, Fi, C = 2, 9, 3, 4
    ops = _operands(Fi, C, 1)
    adj = (torch.rand(B, N, N) < 0.4).double()                # 0/1 with loops on the diagonal here and there
    adj[:, 2] = 0                                             # an empty row
    x = torch.randn(B, N, Fi, dtype=torch.float64)
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])              # adj[b, i, j]: edge j -> i
    d = dense_resgated(x, adj, *ops)
    s = resgated(x.view(B * N, Fi), ei, *ops).view(B, N, C)
    assert float((d - s).abs().max()) <= 1e-12
    skip_bias = x @ ops[6].t() + ops[7]
    assert float((d[:, 2] - skip_bias[:, 2]).abs().max()) <= 1e-12          # no in-edge: skip + bias


def test_restatement_add_loop_and_mask():
    torch.manual_seed(2)
    B, N, Fi, C = 2, 5, 3, 4
    ops = _operands(Fi, C, 2)
    x = torch.randn(B, N, Fi, dtype=torch.float64)
    adj = torch.rand(B, N, N, dtype=torch.float64)
    looped = adj.clone()
    looped[:, torch.arange(N), torch.arange(N)] = 1.0
    assert torch.equal(dense_resgated(x, adj, *ops, add_loop=True), dense_resgated(x, looped, *ops))
    mask = torch.tensor([[True, False, True, True, False], [False, True, True, True, True]])
    got = dense_resgated(x, adj, *ops, mask=mask)
    assert torch.equal(got, dense_resgated(x, adj, *ops) * mask.unsqueeze(-1))
    assert torch.equal(dense_resgated(x[0], adj[0], *ops), dense_resgated(x[:1], adj[:1], *ops))   # 2-D inputs


def test_restatement_gradcheck():
    torch.manual_seed(3)
    B, N, Fi, C = 2, 5, 3, 4
    ops = [t.requires_grad_() for t in _operands(Fi, C, 3)]
    x = torch.randn(B, N, Fi, dtype=torch.float64, requires_grad=True)
    adj = ((torch.rand(B, N, N) < 0.5).double() * torch.randn(B, N, N, dtype=torch.float64)).requires_grad_()
    for add_loop in (False, True):
        assert torch.autograd.gradcheck(lambda x_, a_, *o: dense_resgated(x_, a_, *o, add_loop=add_loop),
                                        (x, adj, *ops))
    ei = torch.tensor([[0, 1, 1, 3, 3, 9, 4, 4], [1, 2, 2, 3, 3, 0, 8, 7]])      # duplicates and loops
    xs = torch.randn(B * N, Fi, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x_, *o: resgated(x_, ei, *o), (xs, *ops))


@pytest.mark.parametrize("add_loop", [False, True])
def test_restatement_adjacency_gradient_is_the_stated_formula(add_loop):
    torch.manual_seed(4)
    B, N, Fi, C = 2, 5, 3, 4
    ops = _operands(Fi, C, 4)
    x = torch.randn(B, N, Fi, dtype=torch.float64)
    adj = ((torch.rand(B, N, N) < 0.5).double() * torch.randn(B, N, N, dtype=torch.float64)).requires_grad_()
    g = torch.randn(B, N, C, dtype=torch.float64)
    dense_resgated(x, adj, *ops, add_loop=add_loop).backward(g)
    want = dense_resgated_adj_grad(x, g, *ops[:6], add_loop=add_loop)
    assert float((adj.grad - want).abs().max()) <= 1e-12
    if add_loop:
        assert float(adj.grad.diagonal(dim1=1, dim2=2).abs().max()) == 0.0
    assert float(adj.grad[adj == 0].abs().max()) > 0          # the derivative exists where adj is 0 too
