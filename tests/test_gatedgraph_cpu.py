"""DenseGatedGraphConv / GatedGraphConv host side: parameters, argument checks, the C ABI's validation, the
restatement the GPU tests compare against, checked against itself in float64, and the conditioning of every case of
the GPU table.  No kernel runs."""
import pytest
import torch

import _gatedgraph_cases as cases
from _gatedgraph_restate import (WIDTH_ERROR, DenseGatedRef, GatedRef, dense_gatedgraph, dense_gatedgraph_adj_grad,
                                 gatedgraph, gru, pad)

_CLASSES = ["DenseGatedGraphConv", "GatedGraphConv"]
_KEYS = {"weight": (3, 4, 4), "rnn.weight_ih": (12, 4), "rnn.weight_hh": (12, 4), "rnn.bias_ih": (12,),
         "rnn.bias_hh": (12,)}


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


# ---- parameters -----------------------------------------------------------------------------------
def test_parameters_and_state_dict_keys():
    from gcm import nn as G
    d, s = G.DenseGatedGraphConv(4, 3), G.GatedGraphConv(4, 3)
    for m in (d, s, DenseGatedRef(4, 3), GatedRef(4, 3)):
        assert _shapes(m) == _KEYS
    for m in (d, s):
        assert (m.out_channels, m.num_layers) == (4, 3)
        assert type(m.rnn) is torch.nn.GRUCell and (m.rnn.input_size, m.rnn.hidden_size) == (4, 4)
        assert not isinstance(m, (G.DenseGraphConv, G.GraphConv))
    assert s.aggr == "add"
    assert repr(d) == "DenseGatedGraphConv(4, num_layers=3)" and repr(s) == "GatedGraphConv(4, num_layers=3)"


def test_constructor_arguments_by_position():
    from gcm import nn as G
    s = G.GatedGraphConv(4, 2, "add", False)                    # out_channels, num_layers, aggr, bias
    assert set(s.state_dict()) == {"weight", "rnn.weight_ih", "rnn.weight_hh"}
    d = G.DenseGatedGraphConv(4, 2, False)                      # out_channels, num_layers, bias
    assert set(d.state_dict()) == {"weight", "rnn.weight_ih", "rnn.weight_hh"}
    assert s.weight.shape == d.weight.shape == (2, 4, 4)


@pytest.mark.parametrize("cls", _CLASSES)
def test_bias_false_drops_the_two_bias_keys(cls):
    from gcm import nn as G
    assert set(getattr(G, cls)(4, 3, bias=False).state_dict()) == set(_KEYS) - {"rnn.bias_ih", "rnn.bias_hh"}
    assert set(DenseGatedRef(4, 3, bias=False).state_dict()) == set(_KEYS) - {"rnn.bias_ih", "rnn.bias_hh"}


def test_dense_and_sparse_load_each_other():
    from gcm import nn as G
    d, s = G.DenseGatedGraphConv(4, 3), G.GatedGraphConv(4, 3)
    s.load_state_dict(d.state_dict())
    for k, v in d.state_dict().items():
        assert torch.equal(s.state_dict()[k], v)
    d2 = G.DenseGatedGraphConv(4, 3)
    d2.load_state_dict(s.state_dict())
    assert torch.equal(d2.weight, d.weight) and torch.equal(d2.rnn.bias_hh, d.rnn.bias_hh)
    DenseGatedRef(4, 3).load_state_dict(d.state_dict())
    GatedRef(4, 3).load_state_dict(s.state_dict())


@pytest.mark.parametrize("cls", _CLASSES)
def test_reset_parameters(cls):
    from gcm import nn as G
    conv = getattr(G, cls)(16, 2)
    with torch.no_grad():
        for p in conv.parameters():
            p.fill_(9.0)
    conv.reset_parameters()
    for p in conv.parameters():                                 # U(-1 / sqrt(C), 1 / sqrt(C)): weight and the cell alike
        assert float(p.detach().abs().max()) <= 0.25
    assert float(conv.weight.detach().abs().max()) > 0.2        # 512 draws: the range is used
    getattr(G, cls)(4, 1, bias=False).reset_parameters()


def test_stacks_take_the_layered_and_generic_paths():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    dense = G.Sequential("x, adj, weights, B, N", [(G.DenseGatedGraphConv(8, 2), "x, adj -> x"), torch.nn.Tanh(),
                                                   (G.DenseGatedGraphConv(8, 1), "x, adj -> x")])
    assert DenseGCM(dense, edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is None
    sparse = G.Sequential("x, edges, weights", [(G.GatedGraphConv(8, 2), "x, edges, weights -> x"), torch.nn.Tanh(),
                                                (G.GatedGraphConv(8, 1), "x, edges, weights -> x")])
    mem = SparseGCM(sparse, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()


# ---- argument errors --------------------------------------------------------------------------------
def test_argument_errors():
    from gcm import nn as G, _hip
    x, ei = torch.zeros(3, 3), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(ValueError, match=WIDTH_ERROR):
        G.DenseGatedGraphConv(2, 1)(torch.zeros(1, 3, 3), torch.zeros(1, 3, 3))
    with pytest.raises(ValueError, match=WIDTH_ERROR):
        G.GatedGraphConv(2, 1)(x, ei)
    with pytest.raises(ValueError, match=WIDTH_ERROR):
        pad(x, 2)
    for aggr in ("mean", "max"):
        with pytest.raises(NotImplementedError, match="aggr"):
            G.GatedGraphConv(4, 1, aggr=aggr)
    with pytest.raises(TypeError):
        G.DenseGatedGraphConv(4, 1, aggr="add")                 # the dense twin takes no aggr
    with pytest.raises(TypeError, match="adj must be float32"):
        G.DenseGatedGraphConv(4, 1)(torch.zeros(1, 3, 3), torch.zeros(1, 3, 3, dtype=torch.float64))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.DenseGatedGraphConv(4, 1)(x, torch.ones(3, 3))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.GatedGraphConv(4, 1)(x, ei)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.GatedGraphConv(4, 1)(x, ei, torch.ones(2))
    with pytest.raises(NotImplementedError, match="GATv2Conv is not implemented"):
        G.GATv2Conv(3, 4)                                       # the placeholder stays


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_dense_gatedgraphconv_fwd", "gcm_dense_gatedgraphconv_fwd_workspace_bytes",
              "gcm_dense_gatedgraphconv_bwd", "gcm_dense_gatedgraphconv_bwd_workspace_bytes",
              "gcm_csr_gatedgraphconv_fwd", "gcm_csr_gatedgraphconv_fwd_workspace_bytes",
              "gcm_csr_gatedgraphconv_bwd", "gcm_csr_gatedgraphconv_bwd_workspace_bytes"}


def test_library_exports_every_symbol_of_the_gated_header():
    """include/gcm_hip_gated.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_gated.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_gated.h")))
    assert declared == set(_hip.GATED_PROTOTYPES) == _FUNCTIONS
    assert not declared & (set(_hip.PROTOTYPES) | set(_hip.AGGR_PROTOTYPES) | set(_hip.LEARNED_DET_PROTOTYPES)
                           | set(_hip.TRANSFORMER_PROTOTYPES) | set(_hip.RESET_PROTOTYPES) | set(_hip.GIN_PROTOTYPES)
                           | set(_hip.BPTT_HOPS_PROTOTYPES) | set(_hip.RESGATED_PROTOTYPES))
    lib = _hip.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == _hip.GATED_PROTOTYPES[name][1]
    assert lib.gcm_abi_version() == 8                           # the section is additive
    assert len(_hip.PROTOTYPES) == 150


def test_c_abi_rejects_null_pointers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_gatedgraphconv_fwd(*([None] * 9), 0, 1, 1, 1, 1, 1, 0, None) == -1
    assert lib.gcm_dense_gatedgraphconv_bwd(*([None] * 14), 0, 1, 1, 1, 1, 1, 0, None) == -1
    assert lib.gcm_csr_gatedgraphconv_fwd(*([None] * 11), 0, 1, 0, 1, 1, 1, None) == -1
    assert lib.gcm_csr_gatedgraphconv_bwd(*([None] * 19), 0, 1, 0, 1, 1, 1, None) == -1


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    for L in (1, 3):
        assert lib.gcm_dense_gatedgraphconv_fwd_workspace_bytes(256, 128, 32, L) > 0          # cfg2's dense shape
        assert lib.gcm_dense_gatedgraphconv_bwd_workspace_bytes(256, 128, 32, L) > 0
        assert lib.gcm_csr_gatedgraphconv_fwd_workspace_bytes(512 * 512, 512 * 511, 32, L) > 0   # cfg4's sparse
        assert lib.gcm_csr_gatedgraphconv_bwd_workspace_bytes(512 * 512, 512 * 511, 32, L) > 0
    assert lib.gcm_csr_gatedgraphconv_bwd_workspace_bytes(1000, 0, 32, 2) > 0                 # no edges: still rows
    # what is saved: h_l, m_l and four gate tensors per round, 6 L R C floats, and the bit image [R, ceil(N / 32)]
    for B, N, C, L in ((256, 128, 32, 3), (3, 50, 33, 2), (2, 130, 128, 1)):
        R = B * N
        assert lib.gcm_dense_gatedgraphconv_fwd_workspace_bytes(B, N, C, L) == 4 * (6 * L * R * C + R * ((N + 31) // 32))
        assert lib.gcm_csr_gatedgraphconv_fwd_workspace_bytes(R, 5 * R, C, L) == 4 * 6 * L * R * C
    for dims in ((0, 128, 32, 2), (4, 0, 32, 2), (4, 128, 0, 2), (4, 128, 32, 0)):            # an empty batch
        assert lib.gcm_dense_gatedgraphconv_fwd_workspace_bytes(*dims) == 0
        assert lib.gcm_dense_gatedgraphconv_bwd_workspace_bytes(*dims) == 0
    assert lib.gcm_csr_gatedgraphconv_fwd_workspace_bytes(0, 0, 32, 2) == 0
    assert lib.gcm_csr_gatedgraphconv_bwd_workspace_bytes(0, 0, 32, 2) == 0


# ---- the restatement against itself, in float64 -----------------------------------------------------
def _operands(C, L, seed, bias=True):
    gen = torch.Generator().manual_seed(seed)

    def r(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64) * 0.5
    return [r(L, C, C), r(3 * C, C), r(3 * C, C)] + ([r(3 * C), r(3 * C)] if bias else [None, None])


def test_restatement_equals_a_loop_over_torch_grucell():
    torch.manual_seed(0)
    B, N, Fi, C, L = 2, 6, 3, 5, 4
    ops = _operands(C, L, 0)
    cell = torch.nn.GRUCell(C, C).double()
    with torch.no_grad():
        for p, v in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), ops[1:]):
            p.copy_(v)
    x = torch.randn(B, N, Fi, dtype=torch.float64)
    adj = (torch.rand(B, N, N) < 0.5).double() * torch.randn(B, N, N, dtype=torch.float64)
    h = torch.cat([x, x.new_zeros(B, N, C - Fi)], -1)
    for l in range(L):
        m = adj @ (h @ ops[0][l])
        h = cell(m.view(B * N, C), h.view(B * N, C)).view(B, N, C)
    assert float((dense_gatedgraph(x, adj, *ops) - h).detach().abs().max()) <= 1e-12
    nb = torch.nn.GRUCell(C, C, bias=False).double()
    with torch.no_grad():
        nb.weight_ih.copy_(ops[1])
        nb.weight_hh.copy_(ops[2])
    h0 = torch.randn(7, C, dtype=torch.float64)
    m0 = torch.randn(7, C, dtype=torch.float64)
    assert float((gru(m0, h0, ops[1], ops[2]) - nb(m0, h0)).detach().abs().max()) <= 1e-12


def test_restatement_by_hand():
    # one channel, one round, every parameter 1 except b_hh_n = 0.5: the edges 0 -> 1 twice and the loop 1 -> 1;
    # node 0 has no in-edge and still updates through the cell with m = 0
    one = torch.ones(1, 1, 1, dtype=torch.float64)
    w = torch.ones(3, 1, dtype=torch.float64)
    b_ih = torch.zeros(3, dtype=torch.float64)
    b_hh = torch.tensor([0.0, 0.0, 0.5], dtype=torch.float64)
    x = torch.tensor([[2.0], [-1.0]], dtype=torch.float64)
    ei = torch.tensor([[0, 0, 1], [1, 1, 1]])

    def cell(m, h):
        r = torch.sigmoid(torch.tensor(m + h, dtype=torch.float64))
        z = r.clone()
        n = torch.tanh(m + r * (h + 0.5))
        return (1 - z) * n + z * h
    want = torch.stack([cell(0.0, 2.0), cell(2.0 + 2.0 - 1.0, -1.0)]).view(2, 1)
    assert torch.allclose(gatedgraph(x, ei, one, w, w, b_ih, b_hh), want, rtol=0, atol=1e-15)
    adj = torch.tensor([[0.0, 0.0], [2.0, 1.0]], dtype=torch.float64)        # the duplicate as a weight of 2
    assert torch.allclose(dense_gatedgraph(x, adj, one, w, w, b_ih, b_hh)[0], want, rtol=0, atol=1e-15)


def test_restatement_dense_equals_sparse_on_the_same_weighted_edge_set():
    torch.manual_seed(1)
    B, N, Fi, C, L = 2, 9, 3, 4, 3
    ops = _operands(C, L, 1)
    adj = (torch.rand(B, N, N) < 0.4).double() * torch.randn(B, N, N, dtype=torch.float64)
    adj[:, 2] = 0                                               # an empty row
    x = torch.randn(B, N, Fi, dtype=torch.float64)
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])                # adj[b, i, j]: edge j -> i
    d = dense_gatedgraph(x, adj, *ops)
    s = gatedgraph(x.view(B * N, Fi), ei, *ops, edge_weight=adj[bb, ii, jj]).view(B, N, C)
    assert float((d - s).abs().max()) <= 1e-12
    h = pad(x, C)                                               # no in-edge: the cell with m = 0, round after round
    for _ in range(L):
        h = gru(torch.zeros_like(h), h, *ops[1:])
    assert float((d[:, 2] - h[:, 2]).abs().max()) <= 1e-12
    # a weight vector of the wrong length is ignored
    assert torch.equal(gatedgraph(x.view(B * N, Fi), ei, *ops, edge_weight=torch.ones(3, dtype=torch.float64)),
                       gatedgraph(x.view(B * N, Fi), ei, *ops))


def test_restatement_add_loop_mask_two_d_and_padding():
    torch.manual_seed(2)
    B, N, Fi, C, L = 2, 5, 3, 4, 2
    ops = _operands(C, L, 2)
    x = torch.randn(B, N, Fi, dtype=torch.float64)
    adj = torch.rand(B, N, N, dtype=torch.float64)
    looped = adj.clone()
    looped[:, torch.arange(N), torch.arange(N)] = 1.0
    assert torch.equal(dense_gatedgraph(x, adj, *ops, add_loop=True), dense_gatedgraph(x, looped, *ops))
    mask = torch.tensor([[True, False, True, True, False], [False, True, True, True, True]])
    assert torch.equal(dense_gatedgraph(x, adj, *ops, mask=mask), dense_gatedgraph(x, adj, *ops) * mask.unsqueeze(-1))
    assert torch.equal(dense_gatedgraph(x[0], adj[0], *ops), dense_gatedgraph(x[:1], adj[:1], *ops))   # 2-D inputs
    assert torch.equal(dense_gatedgraph(x, adj[0], *ops), dense_gatedgraph(x, adj[:1].expand(B, N, N), *ops))
    padded = torch.cat([x, x.new_zeros(B, N, C - Fi)], -1)      # Fi < C: explicit zero-padding
    assert torch.equal(dense_gatedgraph(x, adj, *ops), dense_gatedgraph(padded, adj, *ops))


def test_restatement_gradcheck():
    torch.manual_seed(3)
    B, N, Fi, C, L = 2, 4, 2, 3, 2
    ops = [t.requires_grad_() for t in _operands(C, L, 3)]
    x = torch.randn(B, N, Fi, dtype=torch.float64, requires_grad=True)
    adj = ((torch.rand(B, N, N) < 0.5).double() * torch.randn(B, N, N, dtype=torch.float64)).requires_grad_()
    for add_loop in (False, True):
        assert torch.autograd.gradcheck(lambda x_, a_, *o: dense_gatedgraph(x_, a_, *o, add_loop=add_loop),
                                        (x, adj, *ops))
    ei = torch.tensor([[0, 1, 1, 3, 3, 7, 4, 4], [1, 2, 2, 3, 3, 0, 6, 5]])      # duplicates and loops
    xs = torch.randn(B * N, Fi, dtype=torch.float64, requires_grad=True)
    ew = torch.randn(ei.shape[1], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x_, w_, *o: gatedgraph(x_, ei, *o, edge_weight=w_), (xs, ew, *ops))


@pytest.mark.parametrize("add_loop", [False, True])
def test_restatement_adjacency_gradient_is_the_stated_formula(add_loop):
    torch.manual_seed(4)
    B, N, Fi, C, L = 2, 5, 3, 4, 3
    ops = _operands(C, L, 4)
    x = torch.randn(B, N, Fi, dtype=torch.float64)
    adj = ((torch.rand(B, N, N) < 0.5).double() * torch.randn(B, N, N, dtype=torch.float64)).requires_grad_()
    g = torch.randn(B, N, C, dtype=torch.float64)
    dense_gatedgraph(x, adj, *ops, add_loop=add_loop).backward(g)
    want = dense_gatedgraph_adj_grad(x, adj, g, *ops, add_loop=add_loop)
    assert float((adj.grad - want).abs().max()) <= 1e-12
    if add_loop:
        assert float(adj.grad.diagonal(dim1=1, dim2=2).abs().max()) == 0.0
    assert float(adj.grad[adj == 0].abs().max()) > 0            # the derivative exists where adj is 0 too


# ---- the precondition of the GPU table --------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(cases.DENSE_CASES)), ids=[cases.case_id(c) for c in cases.DENSE_CASES])
def test_dense_cases_are_well_conditioned(index):
    _, res = cases.dense_reference(index)
    cond = cases.conditioning(res)
    print(cases.case_id(cases.DENSE_CASES[index]), {k: f"{v:.1e}" for k, v in cond.items()})
    assert set(cond) >= {"out", "x", "weight", "rnn.weight_ih", "rnn.weight_hh"}
    for k, v in cond.items():
        assert v <= 1e-4, (k, v)


@pytest.mark.parametrize("index", range(len(cases.SPARSE_CASES)), ids=[cases.case_id(c) for c in cases.SPARSE_CASES])
def test_sparse_cases_are_well_conditioned(index):
    inp, res = cases.sparse_reference(index)
    cond = cases.conditioning(res)
    print(cases.case_id(cases.SPARSE_CASES[index]), {k: f"{v:.1e}" for k, v in cond.items()})
    assert ("edge_weight" in cond) == (inp["edge_weight"] is not None and inp["edge_weight"].numel() > 0)
    for k, v in cond.items():
        assert v <= 1e-4, (k, v)
