"""EdgeConv / DenseEdgeConv without a GPU: the restatement (tests/_edgeconv_restate.py) against hand-computed answers,
its gradients, the decomposition of the first Linear, the constructor contract of gcm.nn's layers, the C ABI section,
and the conditions under which the GPU cases (tests/_edgeconv_cases.py) have one winner in every precision."""
import pytest
import torch

import _edgeconv_cases as cases
from _edgeconv_restate import (DenseEdgeConvRef, EdgeConvRef, csr_margins, decomposed_pre, dense_edgeconv,
                               dense_margins, dense_messages, edgeconv, make_nn)


def _d(v):
    return torch.tensor(v, dtype=torch.float64)


def _hand_nn():
    """F = 1, H = 2, C = 1, no biases: m_ij = relu(x_i) + relu(x_j - x_i)."""
    nn = torch.nn.Sequential(torch.nn.Linear(2, 2, bias=False), torch.nn.ReLU(), torch.nn.Linear(2, 1, bias=False))
    with torch.no_grad():
        nn[0].weight.copy_(torch.eye(2))
        nn[2].weight.fill_(1.0)
    return nn.double()


# x = [1, 3, 2, 3].  Node 0 receives from 1, 2, 3 and itself: messages 1 + 2, 1 + 1, 1 + 2, 1 + 0 - nodes 1 and 3 tie
# exactly and the first wins.  Node 1 receives nothing.  Node 2 has its self edge only: 2 + 0.  Node 3 receives from 0,
# sparse: twice: 3 + relu(1 - 3) = 3.
_X = [[1.0], [3.0], [2.0], [3.0]]
_EI = torch.tensor([[1, 2, 3, 0, 2, 0, 0], [0, 0, 0, 0, 2, 3, 3]])
_ADJ = [[1, 1, 1, 1], [0, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0]]


def test_restatement_hand_computed_sparse():
    x = _d(_X).requires_grad_()
    out, win = edgeconv(x, _EI, _hand_nn(), with_winner=True)
    assert out.flatten().tolist() == [3.0, 0.0, 2.0, 3.0]      # the empty row gives 0, the self edge counts
    assert win.flatten().tolist() == [0, -1, 4, 5]             # tie 1 / 3 -> the first entry; duplicates -> the first
    out.sum().backward()
    # node 0's winner is node 1: d/dx0 = relu'(x0) - relu'(x1 - x0) = 0, d/dx1 = 1 and nothing for its twin, node 3;
    # node 2: relu'(x2) = 1 (relu'(0) = 0 for the difference); node 3: relu'(x3) = 1, relu'(x0 - x3) = 0
    assert x.grad.flatten().tolist() == [0.0, 1.0, 1.0, 1.0]


def test_restatement_hand_computed_dense():
    x = _d(_X).unsqueeze(0).requires_grad_()
    out, win = dense_edgeconv(x, _d(_ADJ).unsqueeze(0), _hand_nn(), with_winner=True)
    assert out.flatten().tolist() == [3.0, 0.0, 2.0, 3.0]
    assert win.flatten().tolist() == [1, -1, 2, 0]             # tie 1 / 3 -> the lower index
    out.sum().backward()
    assert x.grad.flatten().tolist() == [0.0, 1.0, 1.0, 1.0]
    # the values of adj do not matter
    again = dense_edgeconv(x.detach(), _d(_ADJ).unsqueeze(0) * -2.5, _hand_nn())
    assert torch.equal(again, out.detach())


def test_restatement_mask_zeroes_rows():
    ref = DenseEdgeConvRef(_hand_nn())
    out = ref(_d(_X).unsqueeze(0), _d(_ADJ).unsqueeze(0), torch.tensor([[True, True, False, True]]))
    assert out.flatten().tolist() == [3.0, 0.0, 0.0, 3.0]


@pytest.mark.parametrize("act", ["relu", "leaky"])
def test_restatement_gradcheck(act):
    torch.manual_seed(3)
    nn = make_nn(3, 4, 2, act).double()
    w = [p for p in nn.parameters()]
    x = torch.randn(2, 5, 3, dtype=torch.float64, requires_grad=True)
    adj = (torch.rand(2, 5, 5) < 0.5).double()
    ei = torch.randint(0, 7, (2, 15))
    xs = torch.randn(7, 3, dtype=torch.float64, requires_grad=True)

    def dense(x, *ps):
        return dense_edgeconv(x, adj, nn)

    def sparse(x, *ps):
        return edgeconv(x, ei, nn)

    assert torch.autograd.gradcheck(dense, (x, *w), eps=1e-7, atol=1e-6)
    assert torch.autograd.gradcheck(sparse, (xs, *w), eps=1e-7, atol=1e-6)


def test_decomposition_identity():
    """P_i + Q_j == W1 [x_i, x_j - x_i] + b1 in float64, for every pair."""
    torch.manual_seed(4)
    for bias in (True, False):
        nn = make_nn(5, 7, 3, "relu", bias).double()
        x = torch.randn(2, 6, 5, dtype=torch.float64)
        P, Q = decomposed_pre(x, nn)
        xi, xj = x.unsqueeze(2).expand(2, 6, 6, 5), x.unsqueeze(1).expand(2, 6, 6, 5)
        literal = nn[0](torch.cat([xi, xj - xi], -1))
        assert float((P.unsqueeze(2) + Q.unsqueeze(1) - literal).detach().abs().max()) < 1e-13


def test_dense_equals_sparse_restatement():
    c = cases.dense_case("D2")
    s = cases.csr_case("D2")
    nn = c["nn"].double()
    d = dense_edgeconv(c["x"].double(), c["adj"], nn)
    assert torch.equal(edgeconv(s["x"].double(), s["ei"], nn).view_as(d), d)


# ---- the constructor contract -----------------------------------------------------------------------
def _lin(i, o, **kw):
    return torch.nn.Linear(i, o, **kw)


@pytest.mark.parametrize("cls", ["DenseEdgeConv", "EdgeConv"])
def test_accepted_forms_and_state_dict_keys(cls):
    from gcm import nn as G
    conv = getattr(G, cls)(torch.nn.Sequential(_lin(12, 8), torch.nn.ReLU(), _lin(8, 5)))
    assert list(conv.state_dict()) == ["nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"]
    assert (conv.in_channels, conv.out_channels, conv.aggr) == (6, 5, "max")
    conv = getattr(G, cls)(torch.nn.Sequential(_lin(12, 8, bias=False), torch.nn.LeakyReLU(0.2), _lin(8, 5, bias=False)))
    assert list(conv.state_dict()) == ["nn.0.weight", "nn.2.weight"]
    skinny = torch.nn.Sequential(G.SkinnyLinear(12, 8), torch.nn.ReLU(), G.SkinnyLinear(8, 5))
    assert isinstance(skinny[0], torch.nn.Linear)
    getattr(G, cls)(skinny)
    before = conv.nn[0].weight.clone()
    conv.reset_parameters()
    assert not torch.equal(before, conv.nn[0].weight)


def test_dense_and_sparse_load_each_other():
    from gcm import nn as G
    torch.manual_seed(5)
    a = G.DenseEdgeConv(make_nn(3, 4, 2))
    b = G.EdgeConv(make_nn(3, 4, 2))
    b.load_state_dict(a.state_dict())
    a.load_state_dict(b.state_dict())
    ref = EdgeConvRef(make_nn(3, 4, 2))
    ref.load_state_dict(a.state_dict())
    assert torch.equal(ref.nn[2].bias, b.nn[2].bias)


@pytest.mark.parametrize("cls", ["DenseEdgeConv", "EdgeConv"])
def test_not_implemented(cls):
    from gcm import nn as G
    make = getattr(G, cls)
    S, R = torch.nn.Sequential, torch.nn.ReLU
    bad = [
        _lin(12, 8),                                                       # not a Sequential
        S(_lin(12, 8)),                                                    # a single Linear
        S(_lin(12, 8), R()),                                               # Linear + act
        S(_lin(12, 8), R(), _lin(8, 5), R()),                              # a trailing activation
        S(_lin(12, 8), torch.nn.BatchNorm1d(8), R(), _lin(8, 5)),          # a norm inside
        S(_lin(12, 8), torch.nn.LayerNorm(8), _lin(8, 5)),
        S(_lin(12, 8), torch.nn.Tanh(), _lin(8, 5)),                       # another activation
        S(_lin(12, 8), R(), _lin(8, 8), R(), _lin(8, 5)),                  # a deeper MLP
        S(_lin(12, 8), R(), _lin(9, 5)),                                   # widths that do not chain
    ]
    for nn in bad:
        with pytest.raises(NotImplementedError, match=r"Linear\(2 \* F, H\), ReLU\(\) or LeakyReLU\(s\), Linear\(H, C\)"):
            make(nn)
    with pytest.raises(NotImplementedError, match="monotone activation .* commutes with the max"):
        make(S(_lin(12, 8), R(), _lin(8, 5), R()))
    for aggr in ("add", "mean", "sum"):
        with pytest.raises(NotImplementedError, match="'max' only"):
            make(S(_lin(12, 8), R(), _lin(8, 5)), aggr=aggr)


def test_width_mismatch_is_a_value_error_at_the_call():
    from gcm import nn as G
    nn = torch.nn.Sequential(_lin(12, 8), torch.nn.ReLU(), _lin(8, 5))
    with pytest.raises(ValueError, match="2 \\* 5"):
        G.DenseEdgeConv(nn)(torch.randn(2, 4, 5), torch.ones(2, 4, 4))
    with pytest.raises(ValueError, match="2 \\* 7"):
        G.EdgeConv(nn)(torch.randn(4, 7), torch.tensor([[0, 1], [1, 2]]))


def test_gatv2_placeholder_still_raises():
    from gcm import nn as G
    with pytest.raises(NotImplementedError, match="GATv2Conv is not implemented"):
        G.GATv2Conv(4, 4)


def test_docstrings_state_the_contract():
    from gcm import nn as G
    for cls, path in ((G.DenseEdgeConv, "layered path"), (G.EdgeConv, "generic path")):
        doc = " ".join(cls.__doc__.split())
        for phrase in ("x_j - x_i", "gets 0", "first wins", "Not implemented", path):
            assert phrase in doc, (cls.__name__, phrase)


def test_stacks_take_the_layered_and_generic_paths():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    n1, n2 = cases.memory_nns()
    dense = G.Sequential("x, adj, weights, B, N", [(G.DenseEdgeConv(n1), "x, adj -> x"), torch.nn.Tanh(),
                                                   (G.DenseEdgeConv(n2), "x, adj -> x"), torch.nn.Tanh()])
    assert DenseGCM(dense, edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is None
    n1, n2 = cases.memory_nns()
    sparse = G.Sequential("x, edges, weights", [(G.EdgeConv(n1), "x, edges -> x"), torch.nn.Tanh(),
                                                (G.EdgeConv(n2), "x, edges -> x"), torch.nn.Tanh()])
    mem = SparseGCM(sparse, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_dense_edgemax_fwd", "gcm_dense_edgemax_bwd", "gcm_dense_edgemax_bwd_workspace_bytes",
              "gcm_csr_edgemax_fwd", "gcm_csr_edgemax_bwd", "gcm_csr_edgemax_bwd_workspace_bytes"}


def test_library_exports_every_symbol_of_the_edgeconv_header():
    """include/gcm_hip_edgeconv.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_edgeconv.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_edgeconv.h")))
    assert declared == set(_hip.EDGECONV_PROTOTYPES) == _FUNCTIONS
    assert not declared & set(_hip.PROTOTYPES)
    assert not declared & (set(_hip.GEN_PROTOTYPES) | set(_hip.AGGR_PROTOTYPES) | set(_hip.PNA_PROTOTYPES))
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == _hip.EDGECONV_PROTOTYPES[name]
    assert lib.gcm_abi_version() == 8                         # the section is additive


def test_c_abi_rejects_null_pointers_and_wide_layers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_edgemax_fwd(None, None, None, None, None, 0.0, None, None, 1, 1, 1, 1, None) == -1
    assert lib.gcm_dense_edgemax_bwd(*([None] * 5), 0.0, *([None] * 5), 0, 1, 1, 1, 1, None) == -1
    assert lib.gcm_csr_edgemax_fwd(*([None] * 6), 0.0, None, None, 1, 0, 1, 1, None) == -1
    assert lib.gcm_csr_edgemax_bwd(*([None] * 9), 0.0, *([None] * 5), 0, 1, 0, 1, 1, None) == -1
    one = 1                                                   # any non-null value: the widths are checked first
    assert lib.gcm_dense_edgemax_fwd(one, one, one, one, None, 0.0, one, one, 1, 1, 129, 4, None) == -2
    assert lib.gcm_csr_edgemax_fwd(one, one, one, one, one, None, 0.0, one, one, 1, 0, 4, 129, None) == -2


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_edgemax_bwd_workspace_bytes(256, 128, 32, 32) >= 32 * 33 * 4     # cfg2's dense shape
    assert lib.gcm_csr_edgemax_bwd_workspace_bytes(512 * 512, 512 * 511, 32, 32) >= 32 * 33 * 4
    assert lib.gcm_csr_edgemax_bwd_workspace_bytes(1000, 0, 32, 32) > 0                   # no edges: still rows
    assert lib.gcm_dense_edgemax_bwd_workspace_bytes(0, 128, 32, 32) == 0
    assert lib.gcm_csr_edgemax_bwd_workspace_bytes(0, 0, 32, 32) == 0


# ---- the conditions of the GPU cases ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.DENSE))
def test_dense_case_has_one_winner_in_every_precision(name):
    c = cases.dense_case(name)
    gap, kink = dense_margins(c["x"], c["adj"], c["nn"])
    assert gap >= cases.GAP, f"two messages of a (sink, channel) are {gap:.3e} apart"
    assert kink >= cases.KINK, f"a pre-activation is {kink:.3e} from the kink"
    (B, N, F, H, C), kind = cases.DENSE[name][0], cases.DENSE[name][1]
    assert c["x"].shape == (B, N, F) and c["nn"][0].out_features == H and c["nn"][2].out_features == C
    rows = (c["adj"] != 0).sum(-1)
    if kind == "random40":
        assert int(rows[:, 3].max()) == 0 and bool((c["adj"][:, 5, 5] != 0).all())
    if kind == "lower":
        assert rows[0].tolist() == list(range(N))
    if kind.startswith("hops"):
        assert int(rows[0, 0]) == 0 and int(rows.max()) >= 3


@pytest.mark.parametrize("name", cases.CSR)
def test_csr_case_has_one_winner_in_every_precision(name):
    c = cases.csr_case(name)
    gap, kink = csr_margins(c["x"], c["ei"], c["nn"])
    assert gap >= cases.GAP and kink >= cases.KINK, (gap, kink)
    if name == cases.CSR_EXTRA:
        ei, M = c["ei"], c["x"].shape[0]
        assert torch.unique(ei, dim=1).shape[1] < ei.shape[1]                    # duplicate edges
        assert bool((ei[0] == ei[1]).any())                                      # self edges
        assert int(ei.max()) < M - 3                                             # isolated nodes
    else:
        d = cases.dense_case(name)
        assert c["ei"].shape[1] == int((d["adj"] != 0).sum())                    # the same edge set
