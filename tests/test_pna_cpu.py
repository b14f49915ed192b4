"""PNAConv / DensePNAConv host side: parameters and buffers, argument checks, the degree histogram helper, the C ABI's
validation, the restatement the GPU tests compare against (tests/_pna_restate.py) checked against hand-computed
answers in float64, and the conditions of the two input families for every case of the GPU table.  No kernel runs."""
import ctypes
import math

import pytest
import torch

import _pna_restate as R
from _pna_restate import DensePNARef, PNARef
from gcm.nn import DensePNAConv, PNAConv     # noqa: F401  (without the layers nothing here is worth running)

F64 = torch.float64
_CLASSES = ["DensePNAConv", "PNAConv"]
_DEG = torch.tensor([1, 4, 3, 2])            # 10 nodes: one without in-edges, four with one, ...


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def _keys(cin, cout, A, S, towers, divide_input, post_layers):
    Fi = cin // towers if divide_input else cin
    Fo = cout // towers
    keys = {"aggr_module.avg_deg_lin": (1,), "aggr_module.avg_deg_log": (1,), "lin.weight": (cout, cout),
            "lin.bias": (cout,)}
    for t in range(towers):
        keys[f"pre_nns.{t}.0.weight"], keys[f"pre_nns.{t}.0.bias"] = (Fi, 2 * Fi), (Fi,)
        keys[f"post_nns.{t}.0.weight"], keys[f"post_nns.{t}.0.bias"] = (Fo, (A * S + 1) * Fi), (Fo,)
        for layer in range(1, post_layers):
            keys[f"post_nns.{t}.{2 * layer}.weight"], keys[f"post_nns.{t}.{2 * layer}.bias"] = (Fo, Fo), (Fo,)
    return keys


# ---- parameters -----------------------------------------------------------------------------------
@pytest.mark.parametrize("post_layers", [1, 2])
@pytest.mark.parametrize("divide_input", [False, True])
@pytest.mark.parametrize("towers", [1, 2])
def test_state_dict_keys_and_shapes(towers, divide_input, post_layers):
    from gcm import nn as G
    aggregators, scalers = R.PAPER
    want = _keys(8, 6, 4, 3, towers, divide_input, post_layers)
    kw = dict(towers=towers, divide_input=divide_input, post_layers=post_layers)
    d = G.DensePNAConv(8, 6, aggregators, scalers, _DEG, **kw)
    s = G.PNAConv(8, 6, aggregators, scalers, _DEG, **kw)
    for m in (d, s, DensePNARef(8, 6, aggregators, scalers, _DEG, **kw), PNARef(8, 6, aggregators, scalers, _DEG, **kw)):
        assert _shapes(m) == want
    assert {k for k, _ in d.named_buffers()} == {"aggr_module.avg_deg_lin", "aggr_module.avg_deg_log"}
    s.load_state_dict(d.state_dict())                               # the twins interchange
    for k, v in d.state_dict().items():
        assert torch.equal(s.state_dict()[k], v)
    DensePNARef(8, 6, aggregators, scalers, [1], **kw).load_state_dict(s.state_dict())
    for m in (d, s):
        assert (m.F_in, m.F_out) == (8 // towers if divide_input else 8, 6 // towers)
        assert not isinstance(m, (G.DenseGraphConv, G.GraphConv))
        assert type(m.pre_nns[0][0]) is torch.nn.Linear and type(m.lin) is torch.nn.Linear
    assert repr(s) == f"PNAConv(8, 6, towers={towers})"


@pytest.mark.parametrize("cls", _CLASSES)
def test_reset_parameters_is_linear_default(cls):
    from gcm import nn as G
    conv = getattr(G, cls)(16, 8, ["mean"], ["identity"], _DEG, post_layers=2)
    with torch.no_grad():
        for p in conv.parameters():
            p.fill_(9.0)
    conv.reset_parameters()
    assert 0.05 < float(conv.pre_nns[0][0].weight.detach().abs().max()) <= 1 / math.sqrt(32)     # U(-1/sqrt(fan_in), ..)
    assert float(conv.lin.weight.detach().abs().max()) <= 1 / math.sqrt(8)
    assert float(conv.post_nns[0][2].weight.detach().abs().max()) <= 1 / math.sqrt(8)


def test_degree_statistics_by_hand():
    """deg = [1, 4, 3, 2]: n = 10, sum d deg[d] = 0 + 4 + 6 + 6 = 16, sum log(d+1) deg[d] = 4 log 2 + 3 log 3 + 2 log 4."""
    from gcm import nn as G
    for m in (G.PNAConv(4, 4, ["sum"], ["linear"], _DEG), G.DensePNAConv(4, 4, ["sum"], ["linear"], _DEG.tolist()),
              PNARef(4, 4, ["sum"], ["linear"], _DEG)):
        am = m.aggr_module
        assert am.avg_deg_lin.shape == am.avg_deg_log.shape == (1,) and am.avg_deg_lin.dtype == torch.float32
        assert abs(float(am.avg_deg_lin) - 1.6) < 1e-6
        assert abs(float(am.avg_deg_log) - (4 * math.log(2) + 3 * math.log(3) + 2 * math.log(4)) / 10) < 1e-6


def test_degree_histogram_by_hand():
    from gcm.nn import degree_histogram
    adj = torch.tensor([[0, 0, 0, 0], [2.0, 0, 0, 0], [1, 0.5, 0, 0], [1, 1, -1, 0]])   # in-degrees 0, 1, 2, 3
    assert degree_histogram(adj).tolist() == [1, 1, 1, 1] and degree_histogram(adj).dtype == torch.int64
    assert degree_histogram(torch.stack([adj, torch.zeros(4, 4)])).tolist() == [5, 1, 1, 1]
    ei = torch.tensor([[0, 0, 1, 0, 0, 3], [1, 2, 2, 2, 0, 3]])     # into 0: 1, 1: 1, 2: 3 (a duplicate), 3: 1 (a loop)
    assert degree_histogram(ei).tolist() == [0, 3, 0, 1]
    assert degree_histogram(ei, num_nodes=6).tolist() == [2, 3, 0, 1]
    assert degree_histogram(torch.zeros(2, 0, dtype=torch.long), num_nodes=3).tolist() == [3]


# ---- argument errors --------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", _CLASSES)
def test_argument_errors(cls):
    from gcm import nn as G
    make = getattr(G, cls)
    with pytest.raises(ValueError, match="unknown aggregator 'median'"):
        make(4, 4, ["mean", "median"], ["identity"], _DEG)
    with pytest.raises(ValueError, match="unknown scaler 'exp'"):
        make(4, 4, ["mean"], ["exp"], _DEG)
    with pytest.raises(NotImplementedError, match="pre_layers"):
        make(4, 4, ["mean"], ["identity"], _DEG, pre_layers=2)
    with pytest.raises(NotImplementedError, match="train_norm"):
        make(4, 4, ["mean"], ["identity"], _DEG, train_norm=True)
    with pytest.raises(NotImplementedError, match="in_channels"):
        make((4, 4), 4, ["mean"], ["identity"], _DEG)
    with pytest.raises(AssertionError):
        make(4, 5, ["mean"], ["identity"], _DEG, towers=2)          # out_channels % towers, as PyG asserts
    with pytest.raises(AssertionError):
        make(5, 4, ["mean"], ["identity"], _DEG, towers=2, divide_input=True)
    make(5, 4, ["mean"], ["identity"], _DEG, towers=2)              # without divide_input any in_channels will do


def test_edge_dim_and_the_placeholder():
    from gcm import nn as G
    with pytest.raises(NotImplementedError, match="edge_dim"):
        G.PNAConv(4, 4, ["mean"], ["identity"], _DEG, edge_dim=3)
    with pytest.raises(TypeError):
        G.DensePNAConv(4, 4, ["mean"], ["identity"], _DEG, edge_dim=3)      # the dense twin has no such argument
    with pytest.raises(NotImplementedError, match="GATv2Conv is not implemented"):
        G.GATv2Conv(3, 4)                                           # the placeholder stays
    with pytest.raises(NotImplementedError):
        G.GraphConv(4, 4, aggr="min")                               # and so does GraphConv's


def test_no_cpu_fallback():
    """A CPU module fails before any index is built."""
    from gcm import nn as G, _hip, _ops
    x, ei = torch.zeros(3, 4), torch.tensor([[0, 1], [1, 2]])
    built = []
    orig = _ops.GraphIndex.from_edge_index
    _ops.GraphIndex.from_edge_index = staticmethod(lambda *a: built.append(a))
    try:
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            G.PNAConv(4, 4, ["mean"], ["identity"], _DEG)(x, ei)
    finally:
        _ops.GraphIndex.from_edge_index = staticmethod(orig)
    assert not built
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.DensePNAConv(4, 4, ["mean"], ["identity"], _DEG)(x, torch.ones(3, 3))
    with pytest.raises(TypeError, match="adj must be float32"):
        G.DensePNAConv(4, 4, ["mean"], ["identity"], _DEG)(torch.zeros(1, 3, 4), torch.zeros(1, 3, 3, dtype=F64))


def test_stacks_take_the_layered_and_generic_paths():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    a, s = R.PAPER
    dense = G.Sequential("x, adj, weights, B, N", [(G.DensePNAConv(8, 8, a, s, _DEG), "x, adj -> x"), torch.nn.Tanh(),
                                                   (G.DensePNAConv(8, 8, ["mean", "max"], s, _DEG), "x, adj -> x")])
    assert DenseGCM(dense, edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is None
    canonical = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(8, 8), "x, adj -> x"), torch.nn.Tanh(),
                                                       (G.DenseGraphConv(8, 8), "x, adj -> x"), torch.nn.Tanh()])
    assert DenseGCM(canonical, edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is not None
    sparse = G.Sequential("x, edges, weights", [(G.PNAConv(8, 8, a, s, _DEG), "x, edges, weights -> x"),
                                                torch.nn.Tanh(),
                                                (G.PNAConv(8, 8, ["sum"], s, _DEG), "x, edges, weights -> x")])
    mem = SparseGCM(sparse, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_dense_pnaconv_fwd", "gcm_dense_pnaconv_bwd", "gcm_dense_pnaconv_bwd_workspace_bytes",
              "gcm_csr_pnaconv_fwd", "gcm_csr_pnaconv_bwd", "gcm_csr_pnaconv_bwd_workspace_bytes"}


def test_library_exports_every_symbol_of_the_pna_header():
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_pna.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_pna.h"))) - {"gcm_csr_graphconv_bwd"}
    assert declared == set(_hip.PNA_PROTOTYPES) == _FUNCTIONS
    assert not declared & (set(_hip.PROTOTYPES) | set(_hip.AGGR_PROTOTYPES) | set(_hip.TAG_PROTOTYPES))
    lib = _hip.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == _hip.PNA_PROTOTYPES[name][1]
    assert lib.gcm_abi_version() == 8                               # the section is additive
    assert (_hip.PNA_SUM, _hip.PNA_STD, _hip.PNA_INVERSE_LINEAR) == (0, 5, 4)


def _codes(names, table):
    from gcm import _ops
    return _ops._pna_codes(names, table)


def test_c_abi_validates_without_a_device():
    """Null pointers: GCM_EINVAL.  Widths > 128: GCM_EUNSUPPORTED, before anything is launched (the pointers here are
    host memory that no kernel may touch)."""
    from gcm import _hip, _ops
    lib = _hip.lib()
    aggrs, scalers = _codes(R.PAPER[0], _ops.PNA_AGGREGATORS), _codes(R.PAPER[1], _ops.PNA_SCALERS)
    lists = (aggrs, 4, scalers, 3)
    assert lib.gcm_dense_pnaconv_fwd(*([None] * 16), 2, 5, 8, 8, 1, 0, *lists, 0, None) == -1
    assert lib.gcm_dense_pnaconv_bwd(*([None] * 21), 0, 2, 5, 8, 8, 1, 0, *lists, 0, None) == -1
    assert lib.gcm_csr_pnaconv_fwd(*([None] * 17), 5, 3, 8, 8, 1, 0, *lists, None) == -1
    assert lib.gcm_csr_pnaconv_bwd(*([None] * 23), 0, 5, 3, 8, 8, 1, 0, *lists, None) == -1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for cin, cout in ((129, 8), (8, 129), (256, 128)):
        assert lib.gcm_dense_pnaconv_fwd(*([p] * 16), 2, 5, cin, cout, 1, 0, *lists, 0, None) == -2
        assert lib.gcm_dense_pnaconv_bwd(*([p] * 21), 1 << 40, 2, 5, cin, cout, 1, 0, *lists, 0, None) == -2
        assert lib.gcm_csr_pnaconv_fwd(*([p] * 17), 5, 3, cin, cout, 1, 0, *lists, None) == -2
        assert lib.gcm_csr_pnaconv_bwd(*([p] * 23), 1 << 40, 5, 3, cin, cout, 1, 0, *lists, None) == -2
    # invalid lists and sizes that do not divide: GCM_EINVAL
    assert lib.gcm_dense_pnaconv_fwd(*([p] * 16), 2, 5, 8, 8, 1, 0, 7, 1, scalers, 3, 0, None) == -1    # code 7
    assert lib.gcm_dense_pnaconv_fwd(*([p] * 16), 2, 5, 8, 8, 1, 0, aggrs, 9, scalers, 3, 0, None) == -1
    assert lib.gcm_dense_pnaconv_fwd(*([p] * 16), 2, 5, 8, 9, 2, 0, *lists, 0, None) == -1
    assert lib.gcm_csr_pnaconv_fwd(*([p] * 17), 5, 3, 9, 8, 2, 1, *lists, None) == -1
    assert lib.gcm_dense_pnaconv_fwd(*([p] * 16), 2, 40000, 8, 8, 1, 0, *lists, 0, None) == -2          # N > 32767


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_pnaconv_bwd_workspace_bytes(256, 128, 32, 32, 1, 0, 4, 3) > 0          # cfg2's dense shape
    assert lib.gcm_csr_pnaconv_bwd_workspace_bytes(512 * 512, 512 * 511, 32, 32, 1, 0, 4, 3) > 0
    assert lib.gcm_csr_pnaconv_bwd_workspace_bytes(1000, 0, 32, 32, 2, 1, 6, 5) > 0             # no edges: still rows
    small = lib.gcm_dense_pnaconv_bwd_workspace_bytes(2, 8, 8, 8, 1, 0, 1, 1)
    assert lib.gcm_dense_pnaconv_bwd_workspace_bytes(2, 8, 8, 8, 1, 0, 6, 5) > small            # grows with A S
    for dims in ((0, 8, 8, 8, 1, 0, 1, 1), (2, 8, 0, 8, 1, 0, 1, 1), (2, 8, 8, 9, 2, 0, 1, 1), (2, 8, 8, 8, 1, 0, 0, 1)):
        assert lib.gcm_dense_pnaconv_bwd_workspace_bytes(*dims) == 0
    assert lib.gcm_csr_pnaconv_bwd_workspace_bytes(0, 0, 8, 8, 1, 0, 1, 1) == 0


# ---- the restatement against hand-computed answers, in float64 ---------------------------------------
# Four nodes, one channel, W_pre = [1, 1], b_pre = 0: the message of j -> i is x_i + x_j.  x = (1, 2, 4, 2).
#   node 0: no in-edge.   node 1: from 0 (one message: 3).   node 2: from 0, 1, 3 (5, 6, 6).
#   node 3: from 1 and 3 - a self loop - (4, 4): a tie.
_X = torch.tensor([[1.0], [2.0], [4.0], [2.0]], dtype=F64)
_EI = torch.tensor([[0, 0, 1, 3, 1, 3], [1, 2, 2, 2, 3, 3]])
_N = [0, 1, 3, 2]
_HAND = {"sum": [0, 3, 17, 8], "mean": [0, 3, 17 / 3, 4], "min": [0, 3, 5, 4], "max": [0, 3, 6, 4],
         "var": [0, 0, 97 / 3 - (17 / 3) ** 2, 0], "std": [0, 0, math.sqrt(97 / 3 - (17 / 3) ** 2), 0]}


def _hand_ref(cls, aggregators, scalers):
    """Identity post and final linears on one channel, so that the output is x + the sum of the scaled blocks."""
    ref = cls(1, 1, aggregators, scalers, _DEG).double()
    with torch.no_grad():
        ref.pre_nns[0][0].weight.fill_(1.0)
        ref.pre_nns[0][0].bias.zero_()
        ref.post_nns[0][0].weight.fill_(1.0)
        ref.post_nns[0][0].bias.zero_()
        ref.lin.weight.fill_(1.0)
        ref.lin.bias.zero_()
    return ref


def _dense_of(ei, M):
    adj = torch.zeros(M, M, dtype=F64)
    adj[ei[1], ei[0]] = 1.0
    return adj


@pytest.mark.parametrize("aggregator", R.AGGREGATORS)
def test_restatement_aggregators_by_hand(aggregator):
    want = _X[:, 0] + torch.tensor(_HAND[aggregator], dtype=F64)
    got_s = _hand_ref(PNARef, [aggregator], ["identity"])(_X, _EI)
    got_d = _hand_ref(DensePNARef, [aggregator], ["identity"])(_X, _dense_of(_EI, 4))
    torch.testing.assert_close(got_s[:, 0], want, rtol=0, atol=1e-14)
    torch.testing.assert_close(got_d[0, :, 0], want, rtol=0, atol=1e-14)
    if aggregator in ("var", "std"):                                # one message, and a tie: exactly 0
        assert float(got_s[1, 0]) == 2.0 and float(got_s[3, 0]) == 2.0


@pytest.mark.parametrize("scaler", R.SCALERS)
def test_restatement_scalers_by_hand(scaler):
    lin, log = 1.6, (4 * math.log(2) + 3 * math.log(3) + 2 * math.log(4)) / 10
    s = {"identity": lambda n: 1.0, "amplification": lambda n: math.log(n + 1) / log,
         "attenuation": lambda n: log / math.log(max(n, 1) + 1), "linear": lambda n: n / lin,
         "inverse_linear": lambda n: lin / max(n, 1)}[scaler]
    want = _X[:, 0] + torch.tensor([s(n) * v for n, v in zip(_N, _HAND["sum"])], dtype=F64)
    got = _hand_ref(PNARef, ["sum"], [scaler])(_X, _EI)
    torch.testing.assert_close(got[:, 0], want, rtol=0, atol=1e-6)   # the buffers are float32
    assert float(got[0, 0]) == 1.0                                   # n = 0: every scaler times 0


def test_restatement_concatenation_order_is_scaler_major():
    ref = PNARef(1, 1, ["sum", "max"], ["identity", "linear"], _DEG).double()
    msg, valid = R.sparse_messages(_X, _EI, torch.ones(1, 2, dtype=F64), torch.zeros(1, dtype=F64))
    agg, n = R.aggregate(msg, valid, ref.aggregators)
    am = ref.aggr_module
    scaled = R.scale(agg, n, ref.scalers, am.avg_deg_lin, am.avg_deg_log)
    lin = float(am.avg_deg_lin)
    assert scaled[2].tolist() == pytest.approx([17, 6, 17 * 3 / lin, 6 * 3 / lin])


def test_restatement_tie_gradient_goes_to_the_first_candidate():
    """Node 3 hears 4 from node 1 and 4 from itself: CSR order puts 1 -> 3 first, the dense twin the lower j = 1."""
    for cls, graph in ((PNARef, _EI), (DensePNARef, _dense_of(_EI, 4))):
        for aggregator in ("min", "max"):
            x = _X.clone().requires_grad_()
            out = _hand_ref(cls, [aggregator], ["identity"])(x, graph).reshape(4)
            out[3].backward()
            # d out_3 / d x = 1 (the root term) + 1 (a_3) at node 3, + 1 at the winner's source, node 1
            assert x.grad[:, 0].tolist() == [0.0, 1.0, 0.0, 2.0]
    ei = torch.tensor([[3, 1], [3, 3]])                             # the loop listed first: now it wins
    x = _X.clone().requires_grad_()
    _hand_ref(PNARef, ["max"], ["identity"])(x, ei)[3, 0].backward()
    assert x.grad[:, 0].tolist() == [0.0, 0.0, 0.0, 3.0]


def test_restatement_dense_equals_sparse():
    torch.manual_seed(3)
    B, N, cin, cout = 2, 9, 4, 6
    adj = (torch.rand(B, N, N) < 0.3).to(F64)
    adj[:, 2] = 0
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])
    x = torch.randn(B, N, cin, dtype=F64)
    for towers, divide in ((1, False), (2, False), (2, True)):
        d = R.lively(DensePNARef(cin, cout, R.AGGREGATORS, R.SCALERS, _DEG, towers, 2, divide), 5, False).double()
        s = PNARef(cin, cout, R.AGGREGATORS, R.SCALERS, _DEG, towers, 2, divide).double()
        s.load_state_dict(d.state_dict())
        torch.testing.assert_close(d(x, adj), s(x.view(B * N, cin), ei).view(B, N, cout), rtol=0, atol=1e-11)
    loops = torch.arange(B * N)
    with_loops = torch.cat([ei[:, ei[0] != ei[1]], torch.stack([loops, loops])], 1)
    torch.testing.assert_close(d(x, adj, add_loop=True), s(x.view(B * N, cin), with_loops).view(B, N, cout), rtol=0,
                               atol=1e-11)
    mask = torch.rand(B, N) < 0.5
    assert torch.equal(d(x, adj, mask), d(x, adj) * mask.unsqueeze(-1))


def test_the_message_decomposes_into_a_i_plus_b_j():
    """What the kernels rely on: W_pre [x_i | x_j] + b_pre = (W_dst x_i + b_pre) + W_src x_j."""
    torch.manual_seed(4)
    B, N, Fi = 2, 7, 5
    x = torch.randn(B, N, Fi, dtype=F64)
    w, b = torch.randn(Fi, 2 * Fi, dtype=F64), torch.randn(Fi, dtype=F64)
    a_i = x @ w[:, :Fi].T + b
    b_j = x @ w[:, Fi:].T
    torch.testing.assert_close(R.dense_messages(x, w, b), a_i.unsqueeze(2) + b_j.unsqueeze(1), rtol=0, atol=1e-13)


def test_restatement_gradcheck_on_the_smooth_aggregators():
    torch.manual_seed(6)
    ref = R.lively(PNARef(3, 4, ["sum", "mean", "var"], R.SCALERS, _DEG, 2), 7, False).double()
    x = torch.randn(6, 3, dtype=F64, requires_grad=True)
    ei = torch.tensor([[0, 1, 2, 3, 4, 0, 0, 5], [1, 1, 1, 2, 2, 2, 5, 5]])
    assert torch.autograd.gradcheck(lambda x: ref(x, ei), (x,))


# ---- the GPU table -----------------------------------------------------------------------------------
def test_case_table_holds_the_required_shapes():
    shapes = {c["shape"] for c in R.DENSE_CASES}
    assert {(1, 5, 3, 4, 1, False), (3, 33, 8, 6, 2, False), (3, 33, 8, 6, 2, True), (2, 70, 33, 5, 1, False),
            (2, 128, 32, 32, 1, False), (1, 130, 4, 8, 2, False)} <= shapes
    for shape in R.DENSE_SHAPES:
        assert {c["pattern"] for c in R.DENSE_CASES if c["shape"] == shape} == set(R.PATTERNS)
    assert {(c["mask"], c["add_loop"]) for c in R.DENSE_CASES} == {(False, False), (True, False), (False, True),
                                                                   (True, True)}
    assert any(c["flat"] for c in R.DENSE_CASES)
    assert {(c["M"], c["E"]) for c in R.SPARSE_CASES} >= {(M, E) for M in (7, 70, 200) for E in (0, 12, 400, 2000)}
    for table in (R.DENSE_CASES, R.SPARSE_CASES):
        lists = {c["lists"] for c in table}
        assert {R.ALL, R.PAPER, R.PERMUTED} <= lists
        assert {((a,), ("identity",)) for a in R.AGGREGATORS} <= lists
    inp = R.dense_inputs(R.DENSE_CASES[7])                          # random: some rows are empty, some are not
    n = (inp["adj"] != 0).sum(-1)
    assert int((n == 0).sum()) > 0 and int(n.max()) > 3
    ei = R.sparse_inputs(R.SPARSE_CASES[6])["edge_index"]           # duplicates, duplicate loops, isolated nodes
    assert int(((ei[0] == 0) & (ei[1] == 0)).sum()) >= 2 and int(ei.max()) < 70 - 3


@pytest.mark.parametrize("index", range(len(R.DENSE_CASES)), ids=[R.case_id(c) for c in R.DENSE_CASES])
def test_dense_cases_meet_their_family_condition(index):
    inp, res = R.dense_reference(index)
    x = inp["x"].unsqueeze(0) if inp["x"].dim() == 2 else inp["x"]
    adj = inp["adj"].unsqueeze(0) if inp["adj"].dim() == 2 else inp["adj"]
    assert inp["dyadic"] == R.is_dyadic(inp["ref"].aggregators)
    if inp["dyadic"]:
        assert torch.equal(x, x.round()) and float(x.abs().max()) <= 2
        for seq in inp["ref"].pre_nns:
            for p in seq.parameters():
                assert torch.equal(p * 4, (p * 4).round()) and float(p.abs().max()) <= 0.5
    assert R.family_violations(inp["ref"], x, adj, inp["add_loop"]) == 0
    assert all(torch.isfinite(v).all() for v in res[torch.float64].values())


@pytest.mark.parametrize("index", range(len(R.SPARSE_CASES)), ids=[R.case_id(c) for c in R.SPARSE_CASES])
def test_sparse_cases_meet_their_family_condition(index):
    inp, res = R.sparse_reference(index)
    M = inp["x"].shape[0]
    assert inp["dyadic"] == R.is_dyadic(inp["ref"].aggregators)
    assert R.family_violations(inp["ref"], inp["x"].unsqueeze(0), R.sparse_pattern(inp["edge_index"], M)) == 0
    assert all(torch.isfinite(v).all() for v in res[torch.float64].values())


def test_dyadic_variance_is_exactly_zero_in_fp32_where_it_is_in_float64():
    """The fp32 restatement's variance is exactly 0 wherever the float64 one is, on the dyadic cases."""
    seen = 0
    for index, case in enumerate(R.DENSE_CASES):
        if not R.is_dyadic(case["lists"][0]) or case["shape"][1] > 70:
            continue
        inp = R.dense_inputs(case)
        x = inp["x"].unsqueeze(0) if inp["x"].dim() == 2 else inp["x"]
        adj = inp["adj"].unsqueeze(0) if inp["adj"].dim() == 2 else inp["adj"]
        B, N, _ = x.shape
        pat = R.dense_pattern(adj.expand(B, N, N), inp["add_loop"]).reshape(B * N, N)
        ref = inp["ref"]
        for dt_pair in [(torch.float64, torch.float32)]:
            var = []
            for dt in dt_pair:
                r = R._as(ref, dt)
                pre = r.pre_nns[0][0]
                msg = R.dense_messages(r._tower_x(x.to(dt), 0), pre.weight, pre.bias).reshape(B * N, N, ref.F_in)
                var.append(R.aggregate(msg.detach(), pat, ["var"])[0])
            zero = var[0] == 0
            seen += int(zero.sum())
            assert torch.equal(var[1][zero], torch.zeros_like(var[1][zero]))
    assert seen > 0
