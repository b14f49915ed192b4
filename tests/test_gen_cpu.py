"""GENConv / DenseGENConv host side: parameters, argument checks, the C ABI's validation, the restatement the GPU
tests compare against (tests/_gen_restate.py) pinned by hand-computed answers and gradcheck, and the kink precondition
of the GPU cases (tests/_gen_cases.py).  No kernel runs."""
import itertools
import math

import pytest
import torch

import _gen_cases as cases
from _gen_restate import DenseGENRef, GENRef, dense_softmax_agg, message_norm, softmax_agg


# ---- parameters -----------------------------------------------------------------------------------
def _want_keys(cin, cout, learn_t, msg_norm, norm, num_layers, expansion, bias):
    want = {"aggr_module.t": (1,)}
    if cin != cout:
        for lin in ("lin_src", "lin_dst"):
            want[lin + ".weight"] = (cout, cin)
            if bias:
                want[lin + ".bias"] = (cout,)
    if msg_norm:
        want["msg_norm.scale"] = (1,)
    widths = [cout] + [cout * expansion] * (num_layers - 1) + [cout]
    k = 0
    for i in range(1, len(widths)):
        want[f"mlp.{k}.weight"] = (widths[i], widths[i - 1])
        if bias:
            want[f"mlp.{k}.bias"] = (widths[i],)
        k += 1
        if i < len(widths) - 1:
            if norm is not None:
                want[f"mlp.{k}.weight"] = want[f"mlp.{k}.bias"] = (widths[i],)
                if norm == "batch":
                    want[f"mlp.{k}.running_mean"] = want[f"mlp.{k}.running_var"] = (widths[i],)
                    want[f"mlp.{k}.num_batches_tracked"] = ()
                k += 1
            k += 2                                            # ReLU, Dropout
    return want


@pytest.mark.parametrize("cin,learn_t,msg_norm,learn_scale,norm,num_layers,expansion,bias", [
    c for c in itertools.product([6, 4], [False, True], [False, True], [False, True], ["batch", "layer", None],
                                 [1, 2, 3], [2, 3], [False, True])
    if (c[2] or not c[3]) and (c[5] == 2 or (c[6] == 2 and not c[2]))])
def test_parameters(cin, learn_t, msg_norm, learn_scale, norm, num_layers, expansion, bias):
    from gcm import nn as G
    cout = 4
    kw = dict(t=0.25, learn_t=learn_t, msg_norm=msg_norm, learn_msg_scale=learn_scale, norm=norm,
              num_layers=num_layers, expansion=expansion, bias=bias)
    want = _want_keys(cin, cout, learn_t, msg_norm, norm, num_layers, expansion, bias)
    for m in (G.DenseGENConv(cin, cout, **kw), G.GENConv(cin, cout, **kw), DenseGENRef(cin, cout, **kw),
              GENRef(cin, cout, **kw)):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
        t = m.aggr_module.t
        assert m.initial_t == 0.25 and float(t.detach()) == 0.25 and t.dtype == torch.float32
        assert isinstance(t, torch.nn.Parameter) == learn_t
        assert ("aggr_module.t" in dict(m.named_parameters())) == learn_t
        assert ("aggr_module.t" in dict(m.named_buffers())) == (not learn_t)
        if msg_norm:
            assert float(m.msg_norm.scale.detach()) == 1.0 and m.msg_norm.scale.requires_grad == learn_scale
        assert isinstance(m.mlp, torch.nn.Sequential)
        assert isinstance(m.mlp[len(m.mlp) - 1], torch.nn.Linear)
    for m in (G.DenseGENConv(cin, cout, **kw), G.GENConv(cin, cout, **kw)):
        assert not isinstance(m, (G.DenseGraphConv, G.GraphConv))
        kinds = [type(l) for l in m.mlp]
        if num_layers == 2:
            mid = {"batch": [torch.nn.BatchNorm1d], "layer": [torch.nn.LayerNorm], None: []}[norm]
            assert kinds == [torch.nn.Linear] + mid + [torch.nn.ReLU, torch.nn.Dropout, torch.nn.Linear]
            assert m.mlp[len(m.mlp) - 2].p == 0.0


def test_default_keys():
    from gcm import nn as G
    for m in (G.GENConv(4, 4), G.DenseGENConv(4, 4)):
        assert set(m.state_dict()) == {"aggr_module.t", "mlp.0.weight", "mlp.1.weight", "mlp.1.bias",
                                       "mlp.1.running_mean", "mlp.1.running_var", "mlp.1.num_batches_tracked",
                                       "mlp.4.weight"}
        assert float(m.aggr_module.t) == 1.0 and m.eps == 1e-7
    assert repr(G.GENConv(3, 4)) == "GENConv(3, 4, aggr=softmax)"
    assert repr(G.DenseGENConv(3, 4)) == "DenseGENConv(3, 4, aggr=softmax)"


def test_dense_and_sparse_load_each_other():
    from gcm import nn as G
    kw = dict(learn_t=True, msg_norm=True, learn_msg_scale=True, norm="layer", bias=True)
    d, s = G.DenseGENConv(3, 4, t=0.5, **kw), G.GENConv(3, 4, t=-0.5, **kw)
    s.load_state_dict(d.state_dict())
    assert float(s.aggr_module.t.detach()) == 0.5
    for k, v in d.state_dict().items():
        assert torch.equal(s.state_dict()[k], v)
    d2 = G.DenseGENConv(3, 4, **kw)
    d2.load_state_dict(s.state_dict())
    assert float(d2.aggr_module.t.detach()) == 0.5 and torch.equal(d2.mlp[0].weight, d.mlp[0].weight)
    kw.pop("learn_t")
    DenseGENRef(3, 4, **kw).load_state_dict(d.state_dict())   # (t as a buffer loads a parameter's value)
    GENRef(3, 4, learn_t=True, **kw).load_state_dict(s.state_dict())


@pytest.mark.parametrize("cls", ["DenseGENConv", "GENConv"])
@pytest.mark.parametrize("learn_t", [False, True])
def test_reset_parameters(cls, learn_t):
    from gcm import nn as G
    conv = getattr(G, cls)(3, 4, t=0.3, learn_t=learn_t, msg_norm=True, learn_msg_scale=True, bias=True)
    with torch.no_grad():
        conv.aggr_module.t.fill_(7.0)
        for p in conv.parameters():
            p.fill_(9.0)
    conv.reset_parameters()
    assert float(conv.aggr_module.t.detach()) == pytest.approx(0.3)
    assert float(conv.msg_norm.scale.detach()) == 1.0
    for name, p in conv.named_parameters():
        if name.startswith(("lin_", "mlp.0", "mlp.4")):
            assert float(p.detach().abs().max()) < 1.0, name  # torch.nn.Linear's init: within 1 / sqrt(fan_in)
    assert float(conv.mlp[1].weight.detach().min()) == 1.0 and float(conv.mlp[1].bias.detach().abs().max()) == 0.0


def test_not_implemented():
    from gcm import nn as G
    for cls in (G.GENConv, G.DenseGENConv):
        for kw in (dict(edge_dim=3), dict(aggr="powermean"), dict(aggr="mean"), dict(aggr="max"), dict(aggr="add"),
                   dict(aggr=["softmax"]), dict(aggr=["softmax", "max"]), dict(learn_p=True), dict(norm="instance")):
            with pytest.raises(NotImplementedError):
                cls(4, 4, **kw)
        with pytest.raises(NotImplementedError):
            cls((4, 4), 4)
        with pytest.raises(ValueError):
            cls(4, 4, norm="graph")


def test_argument_errors():
    from gcm import nn as G, _hip
    x, ei = torch.zeros(3, 3), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(TypeError):
        G.DenseGENConv(3, 3)(torch.zeros(1, 3, 3), torch.zeros(1, 3, 3, dtype=torch.float64))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.DenseGENConv(3, 3)(x, torch.ones(3, 3))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.GENConv(3, 4)(x, ei)
    with pytest.raises(TypeError):
        G.GENConv(3, 3)(x, ei, torch.ones(2))                 # no edge weights


def test_stacks_take_the_layered_and_generic_paths():
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    d1, d2 = cases.memory_layers(G.DenseGENConv)
    dense = G.Sequential("x, adj, weights, B, N", [(d1, "x, adj -> x"), torch.nn.Tanh(), (d2, "x, adj -> x"),
                                                   torch.nn.Tanh()])
    assert DenseGCM(dense, edge_selectors=TemporalBackedge([1]), graph_size=8)._structure() is None
    s1, s2 = cases.memory_layers(G.GENConv)
    sparse = G.Sequential("x, edges, weights", [(s1, "x, edges -> x"), torch.nn.Tanh(), (s2, "x, edges -> x"),
                                                torch.nn.Tanh()])
    mem = SparseGCM(sparse, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert mem._canonical() is None and not mem._native_gnn()


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_dense_gen_fwd", "gcm_dense_gen_bwd", "gcm_dense_gen_bwd_workspace_bytes",
              "gcm_csr_gen_fwd", "gcm_csr_gen_bwd", "gcm_csr_gen_bwd_workspace_bytes"}


def test_library_exports_every_symbol_of_the_gen_header():
    """include/gcm_hip_gen.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_gen.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_gen.h")))
    assert declared == set(_hip.GEN_PROTOTYPES) == _FUNCTIONS
    assert not declared & set(_hip.PROTOTYPES)
    assert not declared & (set(_hip.GIN_PROTOTYPES) | set(_hip.AGGR_PROTOTYPES) | set(_hip.PNA_PROTOTYPES))
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == _hip.GEN_PROTOTYPES[name]
    assert lib.gcm_abi_version() == 8                         # the section is additive


def test_c_abi_rejects_null_pointers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_gen_fwd(None, None, None, 1e-7, None, None, None, 1, 1, 1, None) == -1
    assert lib.gcm_dense_gen_bwd(None, None, None, None, 1e-7, *([None] * 5), 0, 1, 1, 1, None) == -1
    assert lib.gcm_csr_gen_fwd(None, None, None, None, 1e-7, None, None, 1, 0, 1, None) == -1
    assert lib.gcm_csr_gen_bwd(None, None, None, 1e-7, *([None] * 9), 0, 1, 0, 1, None) == -1


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_gen_bwd_workspace_bytes(256, 128, 32) > 0           # cfg2's dense shape
    assert lib.gcm_csr_gen_bwd_workspace_bytes(512 * 512, 512 * 511, 32) > 0  # cfg4's sparse one
    assert lib.gcm_csr_gen_bwd_workspace_bytes(1000, 0, 32) > 0              # no edges: still rows
    assert lib.gcm_dense_gen_bwd_workspace_bytes(0, 128, 32) == 0
    assert lib.gcm_csr_gen_bwd_workspace_bytes(0, 0, 32) == 0


# ---- the restatement against hand-computed answers --------------------------------------------------
def _d(v):
    return torch.tensor(v, dtype=torch.float64)


# node 2 aggregates from 0 and 1, node 1 from 0, node 0 from nothing; x >= 0 so m = x + eps
_X = [[1.0, 4.0], [3.0, 0.0], [0.5, 2.0]]
_EI = torch.tensor([[0, 1, 0], [2, 2, 1]])
_ADJ = [[0, 0, 0], [1, 0, 0], [1, 1, 0]]


def _both(x, ei, adj, t, eps=0.0):
    s = softmax_agg(_d(x), ei, t, eps)
    d = dense_softmax_agg(_d(x).unsqueeze(0), _d(adj).unsqueeze(0), t, eps)[0]
    assert float((s - d).abs().max()) <= 1e-15
    return s


def test_restatement_t_zero_is_the_mean():
    got = _both(_X, _EI, _ADJ, 0.0)
    assert torch.allclose(got, _d([[0.0, 0.0], [1.0, 4.0], [2.0, 2.0]]), rtol=0, atol=1e-15)
    # relu and eps: m = relu(x) + eps
    got = softmax_agg(_d([[-1.0], [3.0], [0.0]]), _EI, 0.0, 0.5)
    assert torch.allclose(got, _d([[0.0], [0.5], [(0.5 + 3.5) / 2]]), rtol=0, atol=1e-15)


def test_restatement_softmax_weights():
    # node 2, channel 0: m = (1, 3), t = 1: weights e^1, e^3
    got = _both(_X, _EI, _ADJ, 1.0)
    w = math.exp(1.0) + math.exp(3.0)
    assert float(got[2, 0]) == pytest.approx((1.0 * math.exp(1.0) + 3.0 * math.exp(3.0)) / w, abs=1e-14)
    w = math.exp(4.0) + 1.0
    assert float(got[2, 1]) == pytest.approx(4.0 * math.exp(4.0) / w, abs=1e-14)
    assert torch.equal(got[1], _d([1.0, 4.0]))                # a single neighbour: itself, whatever t


def test_restatement_large_t_approaches_the_max_and_negative_the_min():
    got = _both(_X, _EI, _ADJ, 200.0)
    assert torch.allclose(got[2], _d([3.0, 4.0]), rtol=0, atol=1e-12)
    got = _both(_X, _EI, _ADJ, -200.0)
    assert torch.allclose(got[2], _d([1.0, 0.0]), rtol=0, atol=1e-12)
    # logits in the thousands: no overflow
    assert torch.isfinite(_both([[1000.0, 4.0], [3.0, 0.0], [0.5, 2.0]], _EI, _ADJ, 40.0)).all()


def test_restatement_isolated_node_gives_zero():
    got = _both(_X, _EI, _ADJ, 1.0, eps=0.25)
    assert torch.equal(got[0], _d([0.0, 0.0]))


def test_restatement_duplicate_edge_counts_twice():
    # node 1: 0 -> 1 twice and 2 -> 1 once, t = 0: (2 m_0 + m_2) / 3
    x = _d([[1.0], [5.0], [4.0]])
    ei = torch.tensor([[0, 2, 0], [1, 1, 1]])
    assert float(softmax_agg(x, ei, 0.0, 0.0)[1, 0]) == pytest.approx(2.0, abs=1e-15)
    got = float(softmax_agg(x, ei, 1.0, 0.0)[1, 0])
    assert got == pytest.approx((2 * math.e + 4 * math.exp(4.0)) / (2 * math.e + math.exp(4.0)), abs=1e-14)


def test_restatement_self_edge_is_counted_and_none_is_added():
    x = _d([[2.0], [6.0]])
    ei = torch.tensor([[0, 1], [1, 1]])                        # 0 -> 1 and 1 -> 1
    assert float(softmax_agg(x, ei, 0.0, 0.0)[1, 0]) == pytest.approx(4.0, abs=1e-15)
    adj = _d([[[0, 0], [1, 1]]])
    assert float(dense_softmax_agg(x.unsqueeze(0), adj, 0.0, 0.0)[0, 1, 0]) == pytest.approx(4.0, abs=1e-15)
    adj = _d([[[0, 0], [1, 0]]])                               # without the diagonal: node 0 alone, no loop added
    assert float(dense_softmax_agg(x.unsqueeze(0), adj, 0.0, 0.0)[0, 1, 0]) == pytest.approx(2.0, abs=1e-15)


def test_restatement_dense_reads_the_pattern_only():
    torch.manual_seed(2)
    x = torch.randn(2, 6, 3, dtype=torch.float64)
    pat = (torch.rand(2, 6, 6) < 0.5).double()
    a = dense_softmax_agg(x, pat, 1.3)
    b = dense_softmax_agg(x, pat * (torch.rand(2, 6, 6, dtype=torch.float64) * 4 - 2), 1.3)
    assert torch.equal(a, b)


def test_restatement_message_norm_and_layer():
    x = _d([[3.0, 4.0], [0.0, 0.0]])
    agg = _d([[0.0, 2.0], [0.0, 0.0]])
    got = message_norm(x, agg, _d([0.5]))
    assert torch.allclose(got, _d([[0.0, 2.5], [0.0, 0.0]]), rtol=0, atol=1e-15)   # a zero aggregate stays zero
    # the whole layer with in == out, no norm: mlp(agg + x)
    torch.manual_seed(3)
    ref = GENRef(2, 2, t=0.0, norm=None).double()
    xx = _d(_X)
    want = ref.mlp(_d([[0.0, 0.0], [1.0, 4.0], [2.0, 2.0]]) + 1e-7 * _d([[0, 0], [1, 1], [1, 1]]) + xx)
    assert torch.allclose(ref(xx, _EI), want, rtol=0, atol=1e-14)
    # mask
    dref = DenseGENRef(2, 2, t=0.0, norm=None).double()
    dref.load_state_dict(ref.state_dict())
    out = dref(xx, _d(_ADJ), mask=torch.tensor([[True, False, True]]))
    assert torch.allclose(out[0, 0], want[0], rtol=0, atol=1e-14) and torch.equal(out[0, 1], _d([0.0, 0.0]))


def test_restatement_gradcheck():
    torch.manual_seed(4)
    M, C = 7, 3
    ei = cases.edges(M, 14, seed=4)
    adj = torch.zeros(1, M, M, dtype=torch.float64)
    adj[0, ei[1], ei[0]] = 1
    x = (torch.randn(M, C, dtype=torch.float64) + 0.3).requires_grad_()
    assert float(x.detach().abs().min()) > 1e-3               # away from relu's kink
    t = torch.tensor([0.7], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x_, t_: softmax_agg(x_, ei, t_), (x, t))
    assert torch.autograd.gradcheck(lambda x_, t_: dense_softmax_agg(x_.unsqueeze(0), adj, t_), (x, t))


def test_dense_equals_sparse_on_one_random_graph():
    torch.manual_seed(1)
    B, N, F, C = 2, 9, 3, 5
    ref = DenseGENRef(F, C, t=0.8, learn_t=True, msg_norm=True, norm="layer", bias=True).double()
    sref = GENRef(F, C, learn_t=True, msg_norm=True, norm="layer", bias=True).double()
    sref.load_state_dict(ref.state_dict())
    adj = (torch.rand(B, N, N) < 0.4).double()                # 0/1 with loops on the diagonal here and there
    adj[:, 2] = 0                                             # an empty row
    x = torch.randn(B, N, F, dtype=torch.float64)
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])              # adj[b, i, j]: edge j -> i
    d = ref(x, adj)
    s = sref(x.view(B * N, F), ei).view(B, N, -1)
    assert float((d - s).detach().abs().max()) <= 1e-12


# ---- the kink precondition of the GPU cases ---------------------------------------------------------
def test_no_gpu_case_has_an_entry_on_relus_kink():
    """An fp32 lin_src can put xs on the other side of relu's kink than float64; the GPU tests compare every entry,
    so the seeds are chosen such that no entry of xs (float64) lies within 1e-5 of zero.  (At most 0.1 % per case
    would be tolerable if such entries were excluded; none is, so none may exist.)  With in == out, xs = x and the
    sign is exact."""
    checked = 0
    for B, N, C, opts in cases.DENSE:
        c = cases.dense_case(B, N, C, opts)
        n = cases.kink_entries(c["ref"], c["x"])
        assert n <= 0.001 * B * N * C and n == 0, (B, N, C, opts)
        checked += c["ref"].in_channels != C
    for M, E, C, opts in cases.CSR:
        c = cases.csr_case(M, E, C, opts)
        n = cases.kink_entries(c["ref"], c["x"])
        assert n <= 0.001 * M * C and n == 0, (M, E, C, opts)
        checked += c["ref"].in_channels != C
    assert checked >= 4
    first, _ = cases.memory_layers(DenseGENRef)
    obs = cases.memory_obs()
    n = cases.kink_entries(first, obs)
    assert n <= 0.001 * obs.shape[0] * obs.shape[1] * first.out_channels and n == 0
    assert first.lin_src.bias is None                         # the zero rows of a memory: xs = 0 in every precision
