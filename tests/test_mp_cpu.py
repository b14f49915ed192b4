"""gcm.nn.MessagePassing and gcm.graph_utils, host side: how propagate collects arguments, what it refuses, the plain
torch utilities, the C ABI's section and its validation, and the restatement the GPU tests compare against
(tests/_mp_restate.py) pinned by hand-computed answers and gradcheck.  No kernel runs."""
import math

import pytest
import torch

import _mp_cases as cases
import _mp_restate as R


def _i(v):
    return torch.tensor(v, dtype=torch.int64)


def _d(v):
    return torch.tensor(v, dtype=torch.float64)


_EI = _i([[0, 1, 0, 2], [2, 2, 1, 2]])          # 0 -> 2, 1 -> 2, 0 -> 1, 2 -> 2


# ---- argument collection --------------------------------------------------------------------------
def _recorder(base, **init):
    class Recorder(base):
        """Records what each stage receives; the aggregate is its own (aggr=None), so no kernel is needed."""

        def __init__(self):
            super().__init__(aggr=None, **init)
            self.seen = {}

        def message(self, x_j, x_i, pair_j, pair_i, edge_weight, tag, index, ptr, size, size_i, size_j, dim_size,
                    edge_index, edge_index_i, edge_index_j, opt=7, opt_j=None):
            self.seen["message"] = dict(locals())
            return x_j

        def aggregate(self, inputs, index, dim_size, norm, ptr=None):
            self.seen["aggregate"] = dict(locals())
            return torch.zeros(dim_size, dtype=inputs.dtype).index_add_(0, index, inputs)

        def update(self, inputs, x, tag):
            self.seen["update"] = dict(locals())
            return inputs + x

    return Recorder()


@pytest.mark.parametrize("which", ["gcm", "restatement"])
def test_propagate_collects_arguments_by_pygs_rules(which):
    from gcm import nn as G
    rec = _recorder(G.MessagePassing if which == "gcm" else R.RefMessagePassing, node_dim=0)
    x = _i([10, 20, 30])                                       # int64: gathered with plain indexing, no kernel
    a, b = _d([1.0, 2.0, 3.0]), _d([5.0, 6.0, 7.0])            # a (src, dst) pair in float64
    w = _d([0.1, 0.2, 0.3, 0.4])
    out = rec.propagate(_EI, x=x, pair=(a, b), edge_weight=w, tag="hello", norm=None, unused=1)
    m = rec.seen["message"]
    assert torch.equal(m["x_j"], _i([10, 20, 10, 30])) and torch.equal(m["x_i"], _i([30, 30, 20, 30]))
    assert torch.equal(m["pair_j"], _d([1.0, 2.0, 1.0, 3.0]))              # _j reads element 0 by source
    assert torch.equal(m["pair_i"], _d([7.0, 7.0, 6.0, 7.0]))              # _i reads element 1 by sink
    assert m["edge_weight"] is w and m["tag"] == "hello"                   # passed through as given
    assert torch.equal(m["index"], _EI[1]) and m["ptr"] is None
    assert m["size"] == (3, 3) and m["size_i"] == 3 and m["size_j"] == 3 and m["dim_size"] == 3
    assert m["edge_index"] is _EI
    assert torch.equal(m["edge_index_i"], _EI[1]) and torch.equal(m["edge_index_j"], _EI[0])
    assert m["opt"] == 7 and m["opt_j"] is None                            # defaults stand in for missing keys
    g = rec.seen["aggregate"]
    assert torch.equal(g["index"], _EI[1]) and g["dim_size"] == 3 and g["norm"] is None and g["ptr"] is None
    u = rec.seen["update"]
    assert u["x"] is x and u["tag"] == "hello"
    assert torch.equal(out, _i([0, 10, 60]) + x)


def test_pair_with_no_destination_and_size_argument():
    from gcm import nn as G

    class P(G.MessagePassing):
        def __init__(self):
            super().__init__(aggr=None)

        def message(self, x_j, x_i=None):
            self.x_i = x_i
            return x_j

        def aggregate(self, inputs, dim_size, size):
            return inputs, dim_size, size

    p = P()
    x = torch.arange(6).view(3, 2)
    out, dim_size, size = p.propagate(_EI, x=(x, None))
    assert torch.equal(out, x[_EI[0]]) and p.x_i is None and dim_size == 3 and size == (3, 3)
    out, dim_size, size = p.propagate(_EI, size=(3, 3), x=(x, x))
    assert dim_size == 3 and torch.equal(p.x_i, x[_EI[1]])
    _, dim_size, _ = p.propagate(_EI, size=(3, None), x=x)
    assert dim_size == 3


def test_gathers_of_other_dtypes_carry_no_gradient():
    from gcm import nn as G

    class P(G.MessagePassing):
        def __init__(self):
            super().__init__(aggr=None, node_dim=0)

        def aggregate(self, inputs):
            return inputs

    x = _d([1.0, 2.0, 3.0]).requires_grad_()
    out = P().propagate(_EI, x=x)
    assert torch.equal(out, x.detach()[_EI[0]]) and not out.requires_grad


def test_defaults():
    from gcm import nn as G
    mp = G.MessagePassing()
    assert mp.aggr == "add" and mp.flow == "source_to_target" and mp.node_dim == -2
    x = torch.ones(2)
    assert mp.message(x) is x and mp.update(x) is x
    assert G.MessagePassing("sum").aggr == "sum" and G.MessagePassing(aggr=None).aggr is None
    assert repr(mp) == "MessagePassing()"
    for absent in ("message_and_aggregate", "edge_update", "register_propagate_forward_hook", "explain", "jittable",
                   "decomposed_layers"):
        assert not hasattr(mp, absent), absent


# ---- what is refused --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(aggr=["add", "max"]), dict(aggr=torch.nn.Identity()), dict(aggr="mul"), dict(aggr="std"), dict(aggr="var"),
    dict(aggr="median"), dict(aggr="softmax"), dict(aggr_kwargs={}), dict(flow="target_to_source"),
    dict(decomposed_layers=2), dict(node_dim=1), dict(node_dim=-1)])
def test_constructor_refuses_what_is_not_implemented(kw):
    from gcm import nn as G
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        G.MessagePassing(**kw)


def test_propagate_errors():
    from gcm import nn as G, _hip

    class P(G.MessagePassing):
        def __init__(self, **kw):
            super().__init__(aggr=None, **kw)

        def message(self, x_j, norm):
            return x_j

        def aggregate(self, inputs):
            return inputs

    x = torch.arange(6).view(3, 2)
    with pytest.raises(TypeError, match="norm"):
        P().propagate(_EI, x=x)                                # a missing key without a default
    with pytest.raises(TypeError, match="x"):
        P().propagate(_EI, norm=1, size=(3, 3))
    with pytest.raises(ValueError, match="node_dim"):
        P().propagate(_EI, x=torch.arange(3), norm=1)          # node_dim=-2 gathers 2-D tensors only
    with pytest.raises(ValueError, match="node_dim"):
        P().propagate(_EI, x=torch.zeros(3, 2, 2, dtype=torch.int64), norm=1)
    assert P(node_dim=0).propagate(_EI, x=torch.arange(3), norm=1).shape == (4,)
    with pytest.raises(ValueError, match="rows"):
        P().propagate(_EI, x=x, norm=1, size=(4, 4))
    with pytest.raises(ValueError, match="size"):
        P().propagate(_EI, norm=1, x_unrelated=x)              # nothing tells M
    with pytest.raises(NotImplementedError, match="bipartite"):
        P().propagate(_EI, x=x, norm=1, size=(3, 4))
    with pytest.raises(NotImplementedError, match="bipartite"):
        P().propagate(_EI, x=(x, torch.arange(8).view(4, 2)), norm=1)
    with pytest.raises(NotImplementedError, match="SparseTensor"):
        P().propagate(torch.eye(3).to_sparse(), x=x, norm=1)
    with pytest.raises(ValueError, match="int64"):
        P().propagate(_EI.int(), x=x, norm=1)
    with pytest.raises(NotImplementedError):
        P().edge_updater(_EI)
    with pytest.raises(NotImplementedError, match="aggregate"):
        G.MessagePassing(aggr=None).propagate(_EI, x=x)
    # float32 tensors go through the kernels: no CPU fallback, and the refusal comes before any index is built
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        P().propagate(_EI, x=torch.zeros(3, 2), norm=1)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.MessagePassing().propagate(_EI, x=torch.zeros(3, 2))


def test_segment_utilities_refuse_cpu_and_other_forms():
    from gcm import nn as G, _hip
    src, index = torch.zeros(4, 2), _EI[1]
    for fn in (G.softmax, G.scatter):
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            fn(src, index)
        with pytest.raises(NotImplementedError, match="dim"):
            fn(src, index, dim=1)
        with pytest.raises(TypeError, match="float32"):
            fn(src.double(), index)
        with pytest.raises(ValueError, match="rows"):
            fn(torch.zeros(3, 2), index)
        with pytest.raises(TypeError, match="int64"):
            fn(src, index.int())
    with pytest.raises(NotImplementedError, match="reduce"):
        G.scatter(src, index, reduce="mul")
    with pytest.raises(NotImplementedError, match="ptr"):
        G.softmax(src, index, ptr=torch.tensor([0, 4]))


# ---- the plain torch utilities, both versions, against hand-computed answers ------------------------------
def _utils():
    from gcm import nn as G
    return [G, R.UTILS]


def test_degree():
    for U in _utils():
        d = U.degree(_EI[1], 4)
        assert torch.equal(d, torch.tensor([0.0, 1.0, 3.0, 0.0])) and d.dtype == torch.float32
        assert torch.equal(U.degree(_EI[0]), torch.tensor([2.0, 1.0, 1.0]))           # num_nodes from the index
        assert torch.equal(U.degree(_EI[1], 3, dtype=torch.int64), _i([0, 1, 3]))
        assert U.degree(_i([]), 2).tolist() == [0.0, 0.0]


def test_add_self_loops():
    for U in _utils():
        ei, attr = U.add_self_loops(_EI, num_nodes=4)
        assert torch.equal(ei, _i([[0, 1, 0, 2, 0, 1, 2, 3], [2, 2, 1, 2, 0, 1, 2, 3]])) and attr is None
        assert not hasattr(ei, "gcm_graph")                                          # a new tensor: no index attached
        ei, attr = U.add_self_loops(_EI, _d([1.0, 2.0, 3.0, 4.0]))                   # N from the list, fill 1.0
        assert ei.shape == (2, 7) and torch.equal(attr, _d([1, 2, 3, 4, 1, 1, 1]))
        ei, attr = U.add_self_loops(_EI, torch.ones(4, 2), fill_value=2.5, num_nodes=3)
        assert torch.equal(attr[4:], torch.full((3, 2), 2.5))
    from gcm import nn as G
    for fill in ("mean", "add", torch.ones(1)):
        with pytest.raises(NotImplementedError, match="fill_value"):
            G.add_self_loops(_EI, torch.ones(4), fill_value=fill)


def test_remove_self_loops():
    for U in _utils():
        ei, attr = U.remove_self_loops(_EI, _d([1.0, 2.0, 3.0, 4.0]))
        assert torch.equal(ei, _i([[0, 1, 0], [2, 2, 1]])) and torch.equal(attr, _d([1.0, 2.0, 3.0]))
        assert U.remove_self_loops(_EI)[1] is None


# ---- the restatement against closed forms: node 2 aggregates from 0 and 1, node 1 from 0, node 0 from nothing ---
_X = _d([[1.0, 4.0], [3.0, 0.0], [0.5, 2.0]])
_E3 = _i([[0, 1, 0], [2, 2, 1]])


@pytest.mark.parametrize("aggr,want", [
    ("add", [[0, 0], [1, 4], [4, 4]]), ("sum", [[0, 0], [1, 4], [4, 4]]), ("mean", [[0, 0], [1, 4], [2, 2]]),
    ("max", [[0, 0], [1, 4], [3, 4]]), ("min", [[0, 0], [1, 4], [1, 0]])])
def test_restatement_aggregations(aggr, want):
    got = R.RefMessagePassing(aggr).propagate(_E3, x=_X)
    assert torch.equal(got, _d(want))                          # the empty segment is 0 for every aggr
    assert torch.equal(R.scatter(_X[_E3[0]], _E3[1], dim_size=3, reduce=aggr), _d(want))


def test_restatement_duplicates_and_loops_are_ordinary_terms():
    ei = _i([[0, 2, 0, 1], [1, 1, 1, 1]])                      # 0 -> 1 twice, 2 -> 1, and the loop 1 -> 1
    x = _d([[1.0], [5.0], [4.0]])
    assert R.RefMessagePassing("add").propagate(ei, x=x).flatten().tolist() == [0.0, 11.0, 0.0]
    assert R.RefMessagePassing("mean").propagate(ei, x=x).flatten().tolist() == [0.0, 2.75, 0.0]


def test_restatement_tie_rule():
    c = cases.tie_case()
    x = c["x"].double().requires_grad_()
    msgs = x[c["ei"][0]]
    msgs.retain_grad()
    out = R.scatter(msgs, c["ei"][1], dim_size=c["M"], reduce="max")
    assert out[3].tolist() == [2.0, 5.0] and out[1].tolist() == [0.5, 0.5]
    out.sum().backward()
    want = torch.zeros(6, 2, dtype=torch.float64)
    want[1, 0] = want[0, 1] = 1.0                              # node 3: edge 1 (not 4) in channel 0, edge 0 in channel 1
    want[2] = 1.0                                              # node 1: edge 2 (not 5)
    assert torch.equal(msgs.grad, want)
    msgs = x.detach()[c["ei"][0]].requires_grad_()
    R.scatter(msgs, c["ei"][1], dim_size=c["M"], reduce="min").sum().backward()
    want = torch.zeros(6, 2, dtype=torch.float64)
    want[3, 0] = want[1, 1] = 1.0                              # node 3: edge 3 holds -1; -3 is tied, edge 1 (not 4)
    want[2] = 1.0
    assert torch.equal(msgs.grad, want)


def test_restatement_softmax():
    src = _d([[1.0, 400.0], [3.0, 0.0], [-2.0, 7.0]])
    got = R.softmax(src, _E3[1], None, 3)
    w = math.exp(1.0) + math.exp(3.0)
    assert float(got[0, 0]) == pytest.approx(math.exp(1.0) / w, abs=1e-15)
    assert float(got[1, 0]) == pytest.approx(math.exp(3.0) / w, abs=1e-15)
    assert float(got[0, 1]) == 1.0 and float(got[1, 1]) == pytest.approx(math.exp(-400.0), abs=1e-300)
    assert got[2].tolist() == [1.0, 1.0]                       # a one-entry segment
    assert R.softmax(src[:0], _E3[1][:0], None, 3).shape == (0, 2)
    # trailing dimensions are independent
    s3 = torch.stack([src, 2 * src], 1)
    assert torch.equal(R.softmax(s3, _E3[1], None, 3)[:, 0], got)


def test_restatement_layers_closed_forms():
    L = R.layers(R.RefMessagePassing)
    # GCN on the 3-node graph: loops added, deg = (1, 2, 3)
    torch.manual_seed(0)
    gcn = L.GCN(2, 2).double()
    h = gcn.lin(_X)
    want = torch.stack([h[0], h[1] / 2 + h[0] / math.sqrt(2), h[2] / 3 + h[0] / math.sqrt(3) + h[1] / math.sqrt(6)])
    assert torch.allclose(gcn(_X, _E3), want + gcn.bias, rtol=0, atol=1e-14)
    # GIN: nn((1 + eps) x + sum)
    gin = L.GIN(torch.nn.Identity(), eps=0.5)
    assert torch.allclose(gin(_X, _E3), 1.5 * _X + _d([[0, 0], [1, 4], [4, 4]]), rtol=0, atol=1e-14)
    # EdgeConv with nn = identity: max over [x_i, x_j - x_i]
    ec = L.EdgeConv(torch.nn.Identity())
    assert torch.equal(ec(_X, _E3), _d([[0, 0, 0, 0], [3, 0, -2, 4], [0.5, 2, 2.5, 2]]))
    # GraphConv: edge_weight reaches message in the caller's order
    gc = L.GraphConv(2, 2, aggr="add").double()
    w = _d([2.0, 0.0, -1.0])
    agg = _d([[0, 0], [-1, -4], [2, 8]])
    assert torch.allclose(gc(_X, _E3, w), gc.lin_rel(agg) + gc.lin_root(_X), rtol=0, atol=1e-14)
    # GATv2 with one in-edge: alpha = 1, so node 1 gets lin_l(x_0); node 0 gets the bias alone
    gat = L.GATv2(2, 3, heads=2).double()
    out = gat(_X, _E3)
    assert torch.allclose(out[1], gat.lin_l(_X)[0] + gat.bias, rtol=0, atol=1e-14)
    assert torch.equal(out[0], gat.bias.detach())


def test_restatement_gradcheck():
    torch.manual_seed(5)
    M, C = 7, 3
    ei = cases.edges(M, 14, seed=4)                            # duplicate loops and a duplicate edge: exact ties
    x = torch.randn(M, C, dtype=torch.float64, requires_grad=True)
    for aggr in ("add", "mean", "max", "min"):
        mp = R.RefMessagePassing(aggr)
        assert torch.autograd.gradcheck(lambda x_: mp.propagate(ei, x=x_), (x,)), aggr
    src = torch.randn(ei.shape[1], 2, C, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda s: R.softmax(s, ei[1], None, M), (src,))
    # a tie between two DIFFERENT rows is a kink: the one-sided rule is checked by test_restatement_tie_rule; here the
    # duplicate edges tie with themselves, where giving the gradient to one copy is the exact derivative w.r.t. x
    L = R.layers(R.RefMessagePassing)
    gat = L.GATv2(C, 2, heads=2).double()
    assert torch.autograd.gradcheck(lambda x_: gat(x_, ei), (x,))
    ec = L.EdgeConv(torch.nn.Sequential(torch.nn.Linear(2 * C, 4), torch.nn.Tanh(), torch.nn.Linear(4, 2))).double()
    assert torch.autograd.gradcheck(lambda x_: ec(x_, ei), (x,))


# ---- the C ABI --------------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_mp_gather", "gcm_mp_reduce", "gcm_mp_select_bwd", "gcm_mp_softmax_fwd", "gcm_mp_softmax_bwd"}


def test_library_exports_every_symbol_of_the_mp_header():
    """include/gcm_hip_mp.h is a section gcm_hip.h includes: declared == bound == exported, disjoint from the rest."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_mp.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_mp.h")))
    assert declared == set(_hip.MP_PROTOTYPES) == _FUNCTIONS
    others = [v for k, v in vars(_hip).items() if k.endswith("PROTOTYPES") and k != "MP_PROTOTYPES"]
    assert len(others) >= 17
    for section in others:
        assert not declared & set(section)
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == _hip.MP_PROTOTYPES[name]
    assert lib.gcm_abi_version() == 8                         # the section is additive
    assert (_hip.MP_SUM, _hip.MP_MEAN, _hip.MP_MAX, _hip.MP_MIN) == (0, 1, 2, 3)


def test_c_abi_rejects_null_pointers_and_bad_arguments():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_mp_gather(None, None, None, None, 1, 1, 1, None) == -1
    assert lib.gcm_mp_reduce(None, None, None, 0, None, None, 1, 1, 1, None) == -1
    assert lib.gcm_mp_reduce(None, None, None, 0, None, None, 1, 0, 1, None) == -1        # out is written even at E = 0
    assert lib.gcm_mp_select_bwd(None, None, None, None, 1, 1, 1, None) == -1
    assert lib.gcm_mp_softmax_fwd(None, None, None, None, 1, 1, 1, None) == -1
    assert lib.gcm_mp_softmax_bwd(None, None, None, None, None, 1, 1, 1, None) == -1
    assert lib.gcm_mp_reduce(None, None, None, 4, None, None, 0, 0, 1, None) == -1        # no such op
    assert lib.gcm_mp_gather(None, None, None, None, 1, 1, 0, None) == -1                 # C >= 1
    assert lib.gcm_mp_gather(None, None, None, None, 1, -1, 1, None) == -1
    # nothing to do: nothing is launched and empty tensors may come as NULL
    assert lib.gcm_mp_gather(None, None, None, None, 5, 0, 4, None) == 0
    assert lib.gcm_mp_reduce(None, None, None, 2, None, None, 0, 0, 4, None) == 0
    assert lib.gcm_mp_softmax_fwd(None, None, None, None, 5, 0, 4, None) == 0


# ---- SparseGCM takes a subclassed stack through its generic path ------------------------------------------
def test_subclassed_stack_takes_the_generic_path():
    from gcm import nn as G
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    l1, l2 = cases.memory_stack(R.layers(G.MessagePassing, G))
    assert isinstance(l1, G.MessagePassing) and isinstance(l2, G.MessagePassing)
    gnn = G.Sequential("x, edges, weights", [(l1, "x, edges, weights -> x"), torch.nn.Tanh(), (l2, "x, edges -> x"),
                                             torch.nn.Tanh()])
    mem = SparseGCM(gnn, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()
