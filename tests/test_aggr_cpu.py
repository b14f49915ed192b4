"""Mean / max aggregation (GraphConv(aggr=...), DenseGraphConv(aggr=...), SAGEConv, DenseSAGEConv) host side:
parameters, argument checks, the fused-path guards, the C ABI's validation and the restatement the GPU tests compare
against, pinned by hand-computed answers.  No kernel runs."""
import pytest
import torch

from _aggr_restate import (dense_aggr_conv, dense_max_agg, dense_mean_agg, sparse_aggr_conv, sparse_max_agg,
                           sparse_max_margin, sparse_mean_agg, weighted_max_case)


# ---- constructors and parameters ---------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["add", "mean", "max"])
def test_graphconv_accepts_aggr_and_keeps_its_layout(aggr):
    from gcm import nn as G
    for cls in (G.DenseGraphConv, G.GraphConv):
        m = cls(3, 5, aggr=aggr)
        assert m.aggr == aggr
        sd = m.state_dict()
        assert set(sd) == {"lin_rel.weight", "lin_rel.bias", "lin_root.weight"}
        assert sd["lin_rel.weight"].shape == (5, 3) and sd["lin_root.weight"].shape == (5, 3)
        assert sd["lin_rel.bias"].shape == (5,)
        assert set(cls(3, 5, aggr=aggr, bias=False).state_dict()) == {"lin_rel.weight", "lin_root.weight"}


@pytest.mark.parametrize("aggr", ["min", "sum", "lstm", None])
def test_unknown_aggr_raises(aggr):
    from gcm import nn as G
    for cls in (G.DenseGraphConv, G.GraphConv, G.SAGEConv):
        with pytest.raises(NotImplementedError):
            cls(3, 5, aggr=aggr)


def test_sage_parameters():
    from gcm import nn as G
    s = G.SAGEConv(3, 5)
    assert s.aggr == "mean" and G.SAGEConv(3, 5, aggr="max").aggr == "max"
    sd = s.state_dict()
    assert set(sd) == {"lin_l.weight", "lin_l.bias", "lin_r.weight"}
    assert sd["lin_l.weight"].shape == (5, 3) and sd["lin_l.bias"].shape == (5,) and sd["lin_r.weight"].shape == (5, 3)
    assert set(G.SAGEConv(3, 5, root_weight=False).state_dict()) == {"lin_l.weight", "lin_l.bias"}
    assert set(G.SAGEConv(3, 5, bias=False).state_dict()) == {"lin_l.weight", "lin_r.weight"}
    assert set(G.SAGEConv(3, 5, root_weight=False, bias=False).state_dict()) == {"lin_l.weight"}
    d = G.DenseSAGEConv(3, 5)
    sd = d.state_dict()
    assert set(sd) == {"lin_rel.weight", "lin_root.weight", "lin_root.bias"}
    assert sd["lin_rel.weight"].shape == (5, 3) and sd["lin_root.weight"].shape == (5, 3)
    assert sd["lin_root.bias"].shape == (5,)
    assert set(G.DenseSAGEConv(3, 5, bias=False).state_dict()) == {"lin_rel.weight", "lin_root.weight"}
    assert not isinstance(s, (G.DenseGraphConv, G.GraphConv)) and not isinstance(d, (G.DenseGraphConv, G.GraphConv))


def test_sage_not_implemented_options():
    from gcm import nn as G
    with pytest.raises(NotImplementedError, match="normalize"):
        G.SAGEConv(3, 5, normalize=True)
    with pytest.raises(NotImplementedError, match="project"):
        G.SAGEConv(3, 5, project=True)
    with pytest.raises(NotImplementedError, match="aggr"):
        G.SAGEConv(3, 5, aggr="add")
    with pytest.raises(NotImplementedError, match="normalize"):
        G.DenseSAGEConv(3, 5, normalize=True)


def test_no_cpu_fallback():
    from gcm import nn as G, _hip
    x, ei, adj = torch.zeros(3, 2), torch.tensor([[0, 1], [1, 2]]), torch.ones(3, 3)
    calls = [(G.GraphConv(2, 2, aggr="mean"), (x, ei)), (G.GraphConv(2, 2, aggr="max"), (x, ei, torch.ones(2))),
             (G.SAGEConv(2, 2), (x, ei)), (G.SAGEConv(2, 2, aggr="max", root_weight=False), (x, ei)),
             (G.DenseGraphConv(2, 2, aggr="mean"), (x, adj)), (G.DenseGraphConv(2, 2, aggr="max"), (x, adj)),
             (G.DenseSAGEConv(2, 2), (x, adj))]
    for conv, args in calls:
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            conv(*args)
    with pytest.raises(TypeError):
        G.DenseGraphConv(2, 2, aggr="mean")(torch.zeros(1, 3, 2), torch.zeros(1, 3, 3, dtype=torch.float64))


def test_activation_fusion_is_refused_not_ignored():
    from gcm import nn as G, _hip
    x, ei, adj = torch.zeros(3, 2), torch.tensor([[0, 1], [1, 2]]), torch.ones(3, 3)
    for aggr in ("mean", "max"):
        with pytest.raises(ValueError, match="fusion"):
            G.DenseGraphConv(2, 2, aggr=aggr)(x, adj, _act=_hip.ACT_TANH)
        with pytest.raises(ValueError, match="fusion"):
            G.GraphConv(2, 2, aggr=aggr)(x, ei, _act=_hip.ACT_RELU)


# ---- the fused paths take aggr="add" stacks only ----------------------------------------------
def _dense_stack(make):
    from gcm import nn as G
    return G.Sequential("x, adj, weights, B, N", [(make(4, 8), "x, adj -> x"), torch.nn.Tanh(),
                                                  (make(8, 8), "x, adj -> x"), torch.nn.Tanh()])


def _sparse_stack(make, sig="x, edges, weights -> x"):
    from gcm import nn as G
    return G.Sequential("x, edges, weights", [(make(4, 8), sig), torch.nn.Tanh(), (make(8, 8), sig)])


def test_dense_structure_is_none_for_mean_max_and_sage():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    sel = TemporalBackedge([1])
    assert DenseGCM(_dense_stack(G.DenseGraphConv), edge_selectors=sel, graph_size=8)._structure() is not None
    for make in (lambda a, b: G.DenseGraphConv(a, b, aggr="mean"), lambda a, b: G.DenseGraphConv(a, b, aggr="max"),
                 G.DenseSAGEConv):
        assert DenseGCM(_dense_stack(make), edge_selectors=sel, graph_size=8)._structure() is None
    mixed = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(4, 8), "x, adj -> x"), torch.nn.Tanh(),
                                                   (G.DenseGraphConv(8, 8, aggr="mean"), "x, adj -> x")])
    assert DenseGCM(mixed, edge_selectors=sel, graph_size=8)._structure() is None


def test_sparse_canonical_is_none_for_mean_max_and_sage():
    from gcm import nn as G
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    mem = SparseGCM(_sparse_stack(G.GraphConv), edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._native_gnn()
    for make in (lambda a, b: G.GraphConv(a, b, aggr="mean"), lambda a, b: G.GraphConv(a, b, aggr="max")):
        mem = SparseGCM(_sparse_stack(make), edge_selectors=TemporalEdge([1]), graph_size=8)
        assert mem._canonical() is None and not mem._native_gnn()
    mem = SparseGCM(_sparse_stack(G.SAGEConv, "x, edges -> x"), edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()


# ---- the C ABI ----------------------------------------------------------------------------------
def test_library_exports_every_symbol_of_the_aggregation_header():
    """include/gcm_hip_aggr.h is the section gcm_hip.h includes: every function it declares is exported and bound."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_aggr.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_aggr.h")))
    assert declared == set(_hip.AGGR_PROTOTYPES) == {
        "gcm_dense_aggrconv_fwd", "gcm_dense_aggrconv_bwd_workspace_bytes", "gcm_dense_aggrconv_bwd",
        "gcm_csr_aggrconv_fwd", "gcm_csr_aggrconv_bwd_workspace_bytes", "gcm_csr_aggrconv_bwd"}
    assert not declared & set(_hip.PROTOTYPES)
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == _hip.AGGR_PROTOTYPES[name][1]


def test_c_abi_rejects_null_pointers():
    from gcm import _hip
    lib = _hip.lib()
    for aggr in (_hip.AGGR_MEAN, _hip.AGGR_MAX):
        assert lib.gcm_dense_aggrconv_fwd(*([None] * 10), 1, 1, 1, 1, aggr, None) == -1
        assert lib.gcm_dense_aggrconv_bwd(*([None] * 15), 0, 1, 1, 1, 1, aggr, None) == -1
        assert lib.gcm_csr_aggrconv_fwd(*([None] * 10), 1, 0, 1, 1, aggr, None) == -1
        assert lib.gcm_csr_aggrconv_bwd(*([None] * 19), 0, 1, 0, 1, 1, aggr, None) == -1
    assert (_hip.AGGR_MEAN, _hip.AGGR_MAX) == (1, 2)
    assert lib.gcm_dense_aggrconv_bwd_workspace_bytes(256, 128, 32, 32) > 0
    assert lib.gcm_csr_aggrconv_bwd_workspace_bytes(1000, 900, 32, 16) > 0
    assert lib.gcm_csr_aggrconv_bwd_workspace_bytes(1000, 0, 32, 16) > 0
    assert lib.gcm_dense_aggrconv_bwd_workspace_bytes(0, 128, 32, 32) == 0
    assert lib.gcm_csr_aggrconv_bwd_workspace_bytes(0, 0, 32, 16) == 0


# ---- the restatement against hand-computed answers ----------------------------------------------
def _d(v):
    return torch.tensor(v, dtype=torch.float64)


def test_dense_mean_zero_degree_row_and_clamp():
    x = _d([[[2.0, -4.0], [6.0, 8.0], [1.0, 1.0]]])
    adj = _d([[[0.0, 1.0, 1.0],      # degree 2: the plain mean of rows 1 and 2
               [0.0, 0.0, 0.0],      # degree 0: aggregates 0 (0 / clamp(0) = 0)
               [0.25, 0.25, 0.0]]])  # rowsum 0.5 < 1: the clamp divides by 1, not by 0.5
    agg = dense_mean_agg(x, adj)
    assert torch.equal(agg, _d([[[3.5, 4.5], [0.0, 0.0], [2.0, 1.0]]]))
    # weights: rowsum 4 -> (3 * x0 + 1 * x1) / 4
    assert torch.equal(dense_mean_agg(x, _d([[[3.0, 1.0, 0.0]] * 3]))[0, 0], _d([3.0, -1.0]))
    # the clamp passes the gradient at rowsum == 1 and blocks it below
    a = _d([[[0.5, 0.5, 0.0], [0.25, 0.25, 0.0], [0.0, 0.0, 0.0]]]).requires_grad_()
    dense_mean_agg(x, a)[..., 0].sum().backward()
    # row 0 (rowsum 1): g_adj_0j = x_j0 / 1 - (S_0 / 1^2) with S_0 = 0.5 * 2 + 0.5 * 6 = 4
    assert torch.equal(a.grad[0, 0], _d([2.0 - 4.0, 6.0 - 4.0, 1.0 - 4.0]))
    assert torch.equal(a.grad[0, 1], _d([2.0, 6.0, 1.0]))                       # below the bound: no degree term


def test_dense_max_isolated_negative_and_ties():
    x = _d([[[-3.0, 5.0], [-1.0, 5.0], [-2.0, -7.0], [9.0, 9.0]]])
    adj = _d([[[0.0, 0.0, 0.0, 0.0],        # isolated: 0
               [1.0, 0.0, 1.0, 0.0],        # neighbours 0, 2: channel 0 negative only -> -2, not 0
               [-0.5, 2.0, 0.0, 0.0],       # pattern only: the values (and their signs) do not matter
               [1.0, 1.0, 0.0, 0.0]]])      # channel 1 ties between 0 and 1: the lowest j gets the gradient
    xr = x.clone().requires_grad_()
    agg = dense_max_agg(xr, adj)
    assert torch.equal(agg.detach(), _d([[[0.0, 0.0], [-2.0, 5.0], [-1.0, 5.0], [-1.0, 5.0]]]))
    agg[0, 3, 1].backward()
    assert torch.equal(xr.grad[0, :, 1], _d([1.0, 0.0, 0.0, 0.0]))
    out = dense_aggr_conv(x, adj, _d([[1.0, 0.0], [0.0, 2.0]]), _d([[1.0, 1.0], [0.0, 0.0]]), _d([0.5, 0.0]), "max",
                          mask=torch.tensor([[True, True, False, True]]))
    assert torch.equal(out[0], _d([[2.5, 0.0], [2.5, 10.0], [0.0, 0.0], [17.5, 10.0]]))


def test_sparse_mean_divides_by_count_not_weight_sum():
    x = _d([[2.0], [4.0], [10.0], [1.0]])
    ei = torch.tensor([[0, 1, 1], [2, 2, 3]])
    w = _d([0.5, 0.25, 3.0])
    agg = sparse_mean_agg(x, ei, w)
    assert torch.equal(agg.flatten(), _d([0.0, 0.0, (0.5 * 2 + 0.25 * 4) / 2, 12.0]))    # not / 0.75
    assert torch.equal(sparse_mean_agg(x, ei).flatten(), _d([0.0, 0.0, 3.0, 4.0]))
    # a weight vector of the wrong length is ignored
    out = sparse_aggr_conv(x, ei, _d([[1.0]]), _d([[1.0]]), _d([0.5]), _d([1.0, 2.0]), "mean")
    assert torch.equal(out.flatten(), _d([2.5, 4.5, 13.5, 5.5]))


def test_sparse_max_isolated_negative_duplicates_and_first_edge_wins():
    x = _d([[-3.0, 1.0], [-1.0, 1.0], [4.0, 4.0]])
    # edges into 2: 0 -> 2 twice (duplicate), 1 -> 2; node 0 and 1 without in-edges
    ei = torch.tensor([[0, 1, 0], [2, 2, 2]])
    agg = sparse_max_agg(x, ei)
    assert torch.equal(agg, _d([[0.0, 0.0], [0.0, 0.0], [-1.0, 1.0]]))              # negative only: -1, not 0
    w = _d([1.0, 1.0, 1.0]).requires_grad_()
    xr = x.clone().requires_grad_()
    sparse_max_agg(xr, ei, w)[2, 1].backward()                                       # a three-way tie at 1
    assert torch.equal(w.grad, _d([1.0, 0.0, 0.0])) and torch.equal(xr.grad[:, 1], _d([1.0, 0.0, 0.0]))
    # weights: candidates of channel 0 are 2 * -3, 0.5 * -1, -1 * -3 -> the duplicate with weight -1 wins
    w2 = _d([2.0, 0.5, -1.0]).requires_grad_()
    agg = sparse_max_agg(x, ei, w2)
    assert torch.equal(agg[2].detach(), _d([3.0, 2.0]))
    agg[2, 0].backward()
    assert torch.equal(w2.grad, _d([0.0, 0.0, -3.0]))
    margin = sparse_max_margin(x, ei, w2.detach())
    assert torch.isinf(margin[0]).all() and float(margin[2, 0]) == pytest.approx((3.0 + 0.5) / 3.0)


def test_dense_and_sparse_agree_on_the_same_graph():
    torch.manual_seed(0)
    B, N, Fi, Fo = 2, 7, 3, 4
    adj = (torch.rand(B, N, N) < 0.4).double() * (torch.rand(B, N, N).double() + 0.5)
    adj[:, 2] = 0                                                                    # an empty row
    x = torch.randn(B, N, Fi, dtype=torch.float64)
    w_rel, w_root, b = (torch.randn(Fo, Fi, dtype=torch.float64), torch.randn(Fo, Fi, dtype=torch.float64),
                        torch.randn(Fo, dtype=torch.float64))
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])
    pattern = (adj != 0).double()
    # max: the dense layer reads the pattern, the sparse one with unit weights does the same
    d = dense_aggr_conv(x, adj, w_rel, w_root, b, "max")
    s = sparse_aggr_conv(x.view(B * N, Fi), ei, w_rel, w_root, b, None, "max").view(B, N, Fo)
    assert torch.allclose(d, s)
    # mean: on a 0/1 adjacency with full rows (rowsum >= 1) the weight sum is the edge count
    d = dense_aggr_conv(x, pattern, w_rel, w_root, b, "mean")
    s = sparse_aggr_conv(x.view(B * N, Fi), ei, w_rel, w_root, b, None, "mean").view(B, N, Fo)
    assert torch.allclose(d, s)


@pytest.mark.parametrize("M,E,Fi,seed", [(40, 90, 8, 130), (50, 120, 8, 170), (300, 1500, 32, 1832), (129, 700, 128, 957), (64, 2000, 16, 77)])
def test_weighted_sparse_max_near_ties_stay_under_the_cap(M, E, Fi, seed):
    """The cases test_aggr_gpu.py uses for weighted sparse max.  The products w_e x_src can nearly tie, and a tie
    closer than fp32 resolves may go to another edge than in float64; entries whose two best candidates are within
    1e-5 relative in float64 may be at most 0.1 % of all.  These seeds have none, so the GPU test compares every
    gradient entry."""
    x, ei, w = weighted_max_case(M, E, Fi, seed)
    near = sparse_max_margin(x, ei, w) < 1e-5
    assert int(near.sum()) <= 1e-3 * near.numel()
    assert int(near.sum()) == 0
