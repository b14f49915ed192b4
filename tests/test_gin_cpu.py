"""DenseGINConv / GINConv host side: parameters, argument checks, the C ABI's validation and the restatement the GPU
tests compare against, pinned by hand-computed answers.  No kernel runs."""
import pytest
import torch

from _gin_restate import DenseGINRef, GINRef, dense_gin, gin


def _mlp(cin=3, hid=5, cout=4):
    return torch.nn.Sequential(torch.nn.Linear(cin, hid), torch.nn.Tanh(), torch.nn.Linear(hid, cout))


# ---- parameters -----------------------------------------------------------------------------------
@pytest.mark.parametrize("train_eps", [False, True])
def test_parameters(train_eps):
    from gcm import nn as G
    want = {"eps": (1,), "nn.0.weight": (5, 3), "nn.0.bias": (5,), "nn.2.weight": (4, 5), "nn.2.bias": (4,)}
    d = G.DenseGINConv(_mlp(), eps=0.25, train_eps=train_eps)
    s = G.GINConv(_mlp(), eps=0.25, train_eps=train_eps)
    for m in (d, s, DenseGINRef(_mlp(), 0.25, train_eps), GINRef(_mlp(), 0.25, train_eps)):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
        assert m.initial_eps == 0.25 and float(m.eps.detach()) == 0.25 and m.eps.dtype == torch.float32
        assert isinstance(m.eps, torch.nn.Parameter) == train_eps
        assert ("eps" in dict(m.named_parameters())) == train_eps
        assert ("eps" in dict(m.named_buffers())) == (not train_eps)
    for m in (d, s):
        assert not isinstance(m, (G.DenseGraphConv, G.GraphConv))
    assert repr(s) == f"GINConv(nn={s.nn})" and repr(d) == f"DenseGINConv(nn={d.nn})"


def test_dense_and_sparse_load_each_other():
    from gcm import nn as G
    d, s = G.DenseGINConv(_mlp(), eps=0.5, train_eps=True), G.GINConv(_mlp(), eps=-0.5)
    s.load_state_dict(d.state_dict())
    assert float(s.eps.detach()) == 0.5
    for k, v in d.state_dict().items():
        assert torch.equal(s.state_dict()[k], v)
    d2 = G.DenseGINConv(_mlp())
    d2.load_state_dict(s.state_dict())
    assert float(d2.eps.detach()) == 0.5 and torch.equal(d2.nn[2].weight, d.nn[2].weight)
    DenseGINRef(_mlp()).load_state_dict(d.state_dict())
    GINRef(_mlp(), train_eps=True).load_state_dict(s.state_dict())


@pytest.mark.parametrize("cls", ["DenseGINConv", "GINConv"])
@pytest.mark.parametrize("train_eps", [False, True])
def test_reset_parameters(cls, train_eps):
    from gcm import nn as G
    conv = getattr(G, cls)(_mlp(), eps=0.3, train_eps=train_eps)
    with torch.no_grad():
        conv.eps.fill_(7.0)
        for p in conv.nn.parameters():
            p.fill_(9.0)
    conv.reset_parameters()
    assert float(conv.eps.detach()) == pytest.approx(0.3)
    for p in conv.nn.parameters():
        assert float(p.detach().abs().max()) < 1.0            # torch.nn.Linear's init: within 1 / sqrt(fan_in)
    # nested containers are walked down to the modules that have a reset_parameters()
    deep = torch.nn.Sequential(torch.nn.Sequential(torch.nn.Linear(3, 3)), torch.nn.Tanh())
    conv = getattr(G, cls)(deep)
    with torch.no_grad():
        deep[0][0].weight.fill_(9.0)
    conv.reset_parameters()
    assert float(deep[0][0].weight.detach().abs().max()) < 1.0


def test_stacks_take_the_layered_and_generic_paths():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    dense = G.Sequential("x, adj, weights, B, N", [(G.DenseGINConv(_mlp(4, 8, 8)), "x, adj -> x"), torch.nn.Tanh(),
                                                   (G.DenseGINConv(_mlp(8, 8, 8)), "x, adj -> x"), torch.nn.Tanh()])
    assert DenseGCM(dense, edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is None
    sparse = G.Sequential("x, edges, weights", [(G.GINConv(_mlp(4, 8, 8)), "x, edges -> x"), torch.nn.Tanh(),
                                                (G.GINConv(_mlp(8, 8, 8)), "x, edges -> x")])
    mem = SparseGCM(sparse, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()


# ---- argument errors --------------------------------------------------------------------------------
def test_argument_errors():
    from gcm import nn as G, _hip
    x, ei = torch.zeros(3, 3), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(TypeError):
        G.DenseGINConv(_mlp())(torch.zeros(1, 3, 3), torch.zeros(1, 3, 3, dtype=torch.float64))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.DenseGINConv(_mlp())(x, torch.ones(3, 3))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.GINConv(_mlp())(x, ei)
    assert not hasattr(G, "GINEConv")                         # edge features are not implemented
    with pytest.raises(TypeError):
        G.GINConv(_mlp())(x, ei, torch.ones(2))               # no edge weights, as PyG


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_dense_gin_fwd", "gcm_dense_gin_bwd", "gcm_dense_gin_bwd_workspace_bytes",
              "gcm_csr_gin_fwd", "gcm_csr_gin_bwd", "gcm_csr_gin_bwd_workspace_bytes"}


def test_library_exports_every_symbol_of_the_gin_header():
    """include/gcm_hip_gin.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_gin.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    assert hasattr(_hip, "GIN_PROTOTYPES")
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_gin.h")))
    assert declared == set(_hip.GIN_PROTOTYPES) == _FUNCTIONS
    assert not declared & (set(_hip.PROTOTYPES) | set(_hip.AGGR_PROTOTYPES) | set(_hip.LEARNED_DET_PROTOTYPES)
                           | set(_hip.TRANSFORMER_PROTOTYPES) | set(_hip.RESET_PROTOTYPES))
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == _hip.GIN_PROTOTYPES[name][1]
    assert lib.gcm_abi_version() == 8                         # the section is additive


def test_c_abi_rejects_null_pointers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_gin_fwd(None, None, None, None, 1, 1, 1, 1, None) == -1
    assert lib.gcm_dense_gin_bwd(*([None] * 8), 0, 1, 1, 1, 1, None) == -1
    assert lib.gcm_csr_gin_fwd(None, None, None, None, None, 1, 0, 1, None) == -1
    assert lib.gcm_csr_gin_bwd(*([None] * 8), 0, 1, 0, 1, None) == -1


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_gin_bwd_workspace_bytes(256, 128, 32) > 0           # cfg2's dense shape
    assert lib.gcm_csr_gin_bwd_workspace_bytes(512 * 512, 512 * 511, 32) > 0  # cfg4's sparse one
    assert lib.gcm_csr_gin_bwd_workspace_bytes(1000, 0, 32) > 0              # no edges: still rows
    assert lib.gcm_dense_gin_bwd_workspace_bytes(0, 128, 32) == 0
    assert lib.gcm_csr_gin_bwd_workspace_bytes(0, 0, 32) == 0


# ---- the restatement against hand-computed answers (nn = Identity unless said) ----------------------
def _d(v):
    return torch.tensor(v, dtype=torch.float64)


_ID = torch.nn.Identity()


def test_restatement_path_of_three_nodes():
    # 0 -> 1 -> 2, eps = 0.5: h_0 = 1.5 x_0, h_1 = 1.5 x_1 + x_0, h_2 = 1.5 x_2 + x_1
    x = _d([[1.0, 2.0], [3.0, -1.0], [0.5, 4.0]])
    ei = torch.tensor([[0, 1], [1, 2]])
    want = _d([[1.5, 3.0], [5.5, 0.5], [3.75, 5.0]])
    assert torch.equal(gin(x, ei, 0.5, _ID), want)
    adj = _d([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert torch.equal(dense_gin(x, adj, 0.5, _ID)[0], want)


def test_restatement_eps_minus_one_removes_the_self_term():
    x = _d([[1.0, 2.0], [3.0, -1.0], [0.5, 4.0]])
    ei = torch.tensor([[0, 1], [1, 2]])
    want = _d([[0.0, 0.0], [1.0, 2.0], [3.0, -1.0]])
    assert torch.equal(gin(x, ei, -1.0, _ID), want)
    adj = _d([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert torch.equal(dense_gin(x, adj, -1.0, _ID)[0], want)
    assert torch.equal(dense_gin(x, adj, 0.5, _ID, add_loop=False)[0], want)     # no self term at all


def test_restatement_duplicates_and_loops_count_once_per_occurrence():
    # node 1: the loop 1 -> 1 twice and 0 -> 1 twice; node 0: nothing.  eps = 0
    x = _d([[2.0], [-1.0]])
    ei = torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1]])
    assert torch.equal(gin(x, ei, 0.0, _ID), _d([[2.0], [-1.0 + 2 * -1.0 + 2 * 2.0]]))


def test_restatement_dense_diagonal_is_kept_and_counted():
    # adj values are weights; the diagonal 3 of node 0 is an ordinary entry on top of the self term
    x = _d([[2.0], [-1.0]])
    adj = _d([[3.0, 0.5], [0.0, 0.0]])
    assert torch.equal(dense_gin(x, adj, 0.25, _ID)[0], _d([[1.25 * 2.0 + 3.0 * 2.0 + 0.5 * -1.0], [-1.25]]))
    assert torch.equal(dense_gin(x, adj, 0.25, _ID, add_loop=False)[0], _d([[3.0 * 2.0 - 0.5], [0.0]]))


def test_restatement_without_edges_is_nn_of_the_scaled_input():
    torch.manual_seed(0)
    nn = _mlp().double()
    x = torch.randn(4, 3, dtype=torch.float64)
    assert torch.equal(gin(x, torch.zeros(2, 0, dtype=torch.long), 0.5, nn), nn(1.5 * x))
    assert torch.equal(dense_gin(x, torch.zeros(4, 4, dtype=torch.float64), 0.5, nn)[0], nn(1.5 * x))


def test_restatement_mask():
    x = _d([[[1.0], [2.0]]])
    adj = _d([[[0.0, 1.0], [1.0, 0.0]]])
    mask = torch.tensor([[True, False]])
    assert torch.equal(dense_gin(x, adj, 0.0, _ID, mask), _d([[[3.0], [0.0]]]))


def test_dense_equals_sparse_on_the_same_edge_set():
    torch.manual_seed(1)
    B, N, F = 2, 9, 3
    ref = DenseGINRef(_mlp(), eps=0.3, train_eps=True).double()
    sref = GINRef(_mlp(), train_eps=True).double()
    sref.load_state_dict(ref.state_dict())
    adj = (torch.rand(B, N, N) < 0.4).double()                # 0/1 with loops on the diagonal here and there
    adj[:, 2] = 0                                             # an empty row
    x = torch.randn(B, N, F, dtype=torch.float64)
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])              # adj[b, i, j]: edge j -> i
    d = ref(x, adj)
    s = sref(x.view(B * N, F), ei).view(B, N, -1)
    assert float((d - s).detach().abs().max()) <= 1e-12
