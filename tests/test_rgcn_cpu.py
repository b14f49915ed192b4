"""RGCNConv / DenseRGCNConv / TypedEdge without a GPU: parameters, argument errors, the C ABI section, the restatement by
hand, and the preconditions of the GPU case tables (tests/_rgcn_cases.py, tests/_typed_cases.py)."""
import copy
import ctypes
import math
import os
import re

import pytest
import torch

import _rgcn_cases as RC
import _typed_cases as TC
from _gcn_restate import bound
from _rgcn_restate import RGCNRef, TypedEdge as TypedEdgeRef, bits, bridge_edges, dense_rgcn, sparse_rgcn

F64 = torch.float64
LAYERS = ["DenseRGCNConv", "RGCNConv"]


# ---- parameters -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", LAYERS)
def test_state_dict_keys_and_shapes(cls):
    from gcm import nn as G
    make = getattr(G, cls)
    full = {k: tuple(v.shape) for k, v in make(5, 6, 3).state_dict().items()}
    assert full == {"weight": (3, 5, 6), "root": (5, 6), "bias": (6,)}
    bases = {k: tuple(v.shape) for k, v in make(5, 6, 3, num_bases=2).state_dict().items()}
    assert bases == {"weight": (2, 5, 6), "comp": (3, 2), "root": (5, 6), "bias": (6,)}
    assert set(make(5, 6, 3, root_weight=False, bias=False).state_dict()) == {"weight"}
    assert make(5, 6, 3).num_relations == 3 and "num_relations=3" in repr(make(5, 6, 3))


@pytest.mark.parametrize("num_bases", [None, 2])
def test_dense_and_sparse_load_each_others_state_dict(num_bases):
    from gcm import nn as G
    d, s = G.DenseRGCNConv(5, 6, 3, num_bases=num_bases), G.RGCNConv(5, 6, 3, num_bases=num_bases)
    s.load_state_dict(d.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(d.state_dict().values(), s.state_dict().values()))
    d2 = G.DenseRGCNConv(5, 6, 3, num_bases=num_bases)
    d2.load_state_dict(s.state_dict())
    RGCNRef(5, 6, 3, num_bases=num_bases).load_state_dict(d.state_dict())       # and the restatement's layout


@pytest.mark.parametrize("cls", LAYERS)
def test_initialisation_is_glorot_and_zeros(cls):
    from gcm import nn as G
    torch.manual_seed(0)
    conv = getattr(G, cls)(40, 24, 6, num_bases=4)
    for p, fan in ((conv.weight, 40 + 24), (conv.root, 40 + 24), (conv.comp, 6 + 4)):
        a = math.sqrt(6.0 / fan)
        assert float(p.abs().max()) <= a and float(p.abs().max()) > 0.8 * a and abs(float(p.mean())) < 0.2 * a
    assert float(conv.bias.abs().max()) == 0.0
    with torch.no_grad():
        conv.bias.fill_(3.0)
    conv.reset_parameters()
    assert float(conv.bias.abs().max()) == 0.0


@pytest.mark.parametrize("cls", LAYERS)
def test_what_is_not_implemented_says_so(cls):
    from gcm import nn as G
    make = getattr(G, cls)
    with pytest.raises(NotImplementedError, match="num_blocks"):
        make(4, 4, 2, num_blocks=2)
    with pytest.raises(NotImplementedError, match="in_channels"):
        make((4, 4), 4, 2)
    with pytest.raises(NotImplementedError, match="in_channels"):
        make(None, 4, 2)
    with pytest.raises(NotImplementedError, match="aggr='max'"):
        make(4, 4, 2, aggr="max")
    with pytest.raises(NotImplementedError, match="num_relations=17"):
        make(4, 4, 17)
    make(4, 4, 16, aggr="sum")


def test_rgcnconv_takes_pygs_arguments():
    from gcm import nn as G
    conv = G.RGCNConv(4, 4, 2, None, None, "mean", True, True, False)       # PyG's positional order, is_sorted=True
    assert conv.is_sorted and not conv.relation_mask and conv.bias is None
    assert G.RGCNConv(4, 4, 2, relation_mask=True).relation_mask


def test_no_cpu_fallback():
    from gcm import nn as G, _hip, _ops
    x, ei = torch.zeros(3, 4), torch.tensor([[0, 1], [1, 2]])
    built = []
    orig = _ops.GraphIndex.from_edge_index
    _ops.GraphIndex.from_edge_index = staticmethod(lambda *a: built.append(a))
    try:
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            G.RGCNConv(4, 4, 2)(x, ei, torch.tensor([0, 1]))
    finally:
        _ops.GraphIndex.from_edge_index = staticmethod(orig)
    assert not built
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.DenseRGCNConv(4, 4, 2)(x, torch.ones(3, 3), torch.ones(3, 3))
    with pytest.raises(TypeError, match="adj must be float32"):
        G.DenseRGCNConv(4, 4, 2)(torch.zeros(1, 3, 4), torch.zeros(1, 3, 3, dtype=F64), torch.zeros(1, 3, 3))
    with pytest.raises(TypeError, match="rel must be float32"):
        G.DenseRGCNConv(4, 4, 2)(torch.zeros(1, 3, 4), torch.zeros(1, 3, 3), torch.zeros(1, 3, 3, dtype=torch.int32))


def test_typed_edge_arguments():
    from gcm.edge_selectors.dense import DenseEdge
    from gcm.edge_selectors.learned import LearnedEdge
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.edge_selectors.typed import TypedEdge
    from gcm.gcm import DenseGCM
    sel = TypedEdge([TemporalBackedge([1, 2]), DenseEdge(), LearnedEdge(4)])
    assert sel.num_relations == 3 and sel.relations == [0, 1, 2] and len(sel.selectors) == 3
    assert TypedEdge([TemporalBackedge([1]), DenseEdge(), DenseEdge()], relations=[0, 0, 1]).num_relations == 2
    assert TypedEdge([DenseEdge()], relations=[15]).num_relations == 16
    with pytest.raises(ValueError, match="at most 16 relations"):
        TypedEdge([DenseEdge()], relations=[16])
    with pytest.raises(ValueError, match="at most 16 relations"):
        TypedEdge([DenseEdge() for _ in range(17)], relations=[0] * 17)
    with pytest.raises(ValueError):
        TypedEdge([DenseEdge()], relations=[0, 1])
    with pytest.raises(ValueError, match=r"DenseGCM\(edge_weights=True\)"):
        sel(torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), torch.zeros(0), torch.zeros(2, dtype=torch.long), 2)
    # the children are submodules: the memory finds the flag users and the LearnedEdge among them
    mem = DenseGCM(torch.nn.Identity(), edge_selectors=sel, graph_size=4, edge_weights=True)
    assert mem._has_learned_edge() and any(isinstance(m, TemporalBackedge) for m in mem._flag_users())
    assert len(list(sel.parameters())) == len(list(sel.selectors[2].parameters())) > 0


def test_stacks_take_the_layered_and_generic_paths():
    from gcm import nn as G
    from gcm.edge_selectors.dense import DenseEdge
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.edge_selectors.typed import TypedEdge
    from gcm.gcm import DenseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    from gcm.sparse_gcm import SparseGCM
    sel = TypedEdge([TemporalBackedge([1]), DenseEdge()])
    dense = G.Sequential("x, adj, weights, B, N", [
        (G.DenseRGCNConv(8, 8, sel.num_relations), "x, adj, weights -> x"), torch.nn.Tanh(),
        (G.DenseRGCNConv(8, 8, sel.num_relations), "x, adj, weights -> x"), torch.nn.Tanh()])
    mem = DenseGCM(dense, edge_selectors=sel, graph_size=8, edge_weights=True)
    assert mem._structure() is None
    assert mem._fused_plan(torch.zeros(2, 8, 8), torch.zeros(2, 8, 8), torch.zeros(2, 8, 8), 8) is None
    sparse = G.Sequential("x, edges, types", [(G.RGCNConv(8, 8, 2), "x, edges, types -> x"), torch.nn.Tanh(),
                                              (G.RGCNConv(8, 8, 2), "x, edges, types -> x")])
    smem = SparseGCM(sparse, edge_selectors=TemporalEdge([1]), graph_size=8)
    assert smem._canonical() is None and not smem._native_gnn()


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_dense_rgcnconv_fwd", "gcm_dense_rgcnconv_fwd_workspace_bytes", "gcm_dense_rgcnconv_bwd",
              "gcm_dense_rgcnconv_bwd_workspace_bytes", "gcm_csr_rgcnconv_fwd", "gcm_csr_rgcnconv_fwd_workspace_bytes",
              "gcm_csr_rgcnconv_bwd", "gcm_csr_rgcnconv_bwd_workspace_bytes", "gcm_typed_merge"}


def test_library_exports_every_symbol_of_the_rgcn_header():
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_rgcn.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_rgcn.h")))
    assert declared == set(_hip.RGCN_PROTOTYPES) == _FUNCTIONS
    others = [v for k, v in vars(_hip).items() if k.endswith("PROTOTYPES") and k != "RGCN_PROTOTYPES"]
    assert len(others) >= 19 and not any(declared & set(t) for t in others)
    lib = _hip.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == _hip.RGCN_PROTOTYPES[name][1]
    assert _hip.RGCN_PROTOTYPES["gcm_dense_rgcnconv_fwd_workspace_bytes"][0] is ctypes.c_size_t
    assert lib.gcm_abi_version() == 8                               # the section is additive


def test_c_abi_validates_without_a_device():
    """Null pointers: GCM_EINVAL.  Widths > 128 and more than 16 relations: GCM_EUNSUPPORTED, before anything is
    launched (the pointers here are host memory that no kernel may touch)."""
    from gcm import _hip
    lib = _hip.lib()
    big = 1 << 40
    assert lib.gcm_dense_rgcnconv_fwd(*([None] * 9), 0, 2, 5, 8, 8, 2, 1, None) == -1
    assert lib.gcm_dense_rgcnconv_bwd(*([None] * 13), 0, 2, 5, 8, 8, 2, None) == -1
    assert lib.gcm_csr_rgcnconv_fwd(*([None] * 10), 0, 5, 3, 8, 8, 2, 1, 0, None) == -1
    assert lib.gcm_csr_rgcnconv_bwd(*([None] * 14), 0, 5, 3, 8, 8, 2, 0, None) == -1
    assert lib.gcm_typed_merge(None, None, None, None, 1, None, None, 4, None) == -1
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    for cin, cout, R in ((129, 8, 2), (8, 129, 2), (8, 8, 17)):
        assert lib.gcm_dense_rgcnconv_fwd(*([p] * 9), big, 2, 5, cin, cout, R, 1, None) == -2
        assert lib.gcm_dense_rgcnconv_bwd(*([p] * 13), big, 2, 5, cin, cout, R, None) == -2
        assert lib.gcm_csr_rgcnconv_fwd(*([p] * 10), big, 5, 3, cin, cout, R, 1, 0, None) == -2
        assert lib.gcm_csr_rgcnconv_bwd(*([p] * 14), big, 5, 3, cin, cout, R, 0, None) == -2
    assert lib.gcm_dense_rgcnconv_fwd(*([p] * 9), big, 2, 0, 8, 8, 2, 1, None) == -1          # N = 0
    assert lib.gcm_dense_rgcnconv_fwd(*([p] * 9), 16, 2, 5, 8, 8, 2, 1, None) == -3           # workspace too small
    assert lib.gcm_typed_merge(p, p, p, p, 17, p, p, 4, None) == -2                           # more than 16 children
    bad_bit = (ctypes.c_int * 1)(16)
    kids = (ctypes.c_void_p * 1)(p)
    assert lib.gcm_typed_merge(p, p, ctypes.addressof(kids), ctypes.addressof(bad_bit), 1, p, p, 4, None) == -2


def test_workspace_queries():
    from gcm import _hip
    lib = _hip.lib()
    B, N, F, H, R = 256, 128, 32, 32, 3                                                        # cfg2's shape
    assert lib.gcm_dense_rgcnconv_fwd_workspace_bytes(B, N, F, H, R) >= R * B * N * H * 4
    assert lib.gcm_dense_rgcnconv_bwd_workspace_bytes(B, N, F, H, R) >= 2 * R * B * N * H * 4
    assert lib.gcm_csr_rgcnconv_fwd_workspace_bytes(B * N, B * N * 8, F, H, R) >= R * B * N * H * 4
    assert lib.gcm_csr_rgcnconv_bwd_workspace_bytes(B * N, B * N * 8, F, H, R) >= R * B * N * H * 4
    assert lib.gcm_csr_rgcnconv_bwd_workspace_bytes(1000, 0, 32, 32, 2) > 0                    # no edges: still rows
    assert lib.gcm_dense_rgcnconv_fwd_workspace_bytes(0, N, F, H, R) == 0


# ---- the restatement by hand ------------------------------------------------------------------------
def _hand():
    """3 nodes, 2 relations, 1 feature, W_0 = 10, W_1 = 100, root = 1, bias = 0.5.  Node 0 hears node 1 in relation 0
    and nodes 1, 2 in relation 1; node 1 hears node 2 in both relations at once; node 2 hears nobody."""
    x = torch.tensor([[1.0], [2.0], [4.0]], dtype=F64)
    rel = torch.tensor([[0, 3, 2], [0, 0, 3], [0, 0, 0]], dtype=F64)
    W = torch.tensor([[[10.0]], [[100.0]]], dtype=F64)
    return x, rel, (rel > 0).to(F64), W, torch.ones(1, 1, dtype=F64), torch.tensor([0.5], dtype=F64)


def test_restatement_by_hand():
    x, rel, adj, W, root, bias = _hand()
    mean = dense_rgcn(x, adj, rel, W, root, bias)[0, :, 0]
    #            rel 0          rel 1 (mean of 2, 4 = 3)    root  bias
    assert mean.tolist() == [10 * 2 + 100 * 3 + 1 + 0.5, 10 * 4 + 100 * 4 + 2 + 0.5, 4 + 0.5]
    add = dense_rgcn(x, adj, rel, W, root, bias, aggr="add")[0, :, 0]
    assert add.tolist() == [10 * 2 + 100 * 6 + 1.5, 10 * 4 + 100 * 4 + 2.5, 4.5]
    weighted = dense_rgcn(x, adj * torch.tensor([[9.0, -1.0, 0.5]] * 3, dtype=F64), rel, W, root, bias)[0, :, 0]
    assert weighted[0].item() == 10 * -2 + 100 * (-2 + 2) / 2 + 1.5               # the count is of the pattern
    assert dense_rgcn(x, adj, rel, W, None, None)[0, 2, 0].item() == 0.0          # nobody to hear: nothing, no NaN
    # codes <= 0 are no edge; bits >= R are ignored
    assert torch.equal(dense_rgcn(x, adj, rel + 4 * (rel > 0), W, root, bias)[0, :, 0], mean)
    assert torch.equal(dense_rgcn(x, torch.ones(3, 3, dtype=F64), torch.where(rel > 0, rel, -rel - 1), W, root, bias)[0, :, 0],
                       mean)


def test_restatement_dense_equals_sparse_and_ids_equal_one_bit_masks():
    x, rel, adj, W, root, bias = _hand()
    ei, codes = bridge_edges(rel[None])
    assert ei.tolist() == [[1, 2, 2], [0, 0, 1]] and codes.tolist() == [3, 2, 3]
    for aggr in ("mean", "add"):
        d = dense_rgcn(x, adj, rel, W, root, bias, aggr)[0]
        s = sparse_rgcn(x, ei, codes, W, root, bias, aggr, mask_mode=True)
        assert torch.equal(d, s)
    torch.manual_seed(1)
    B, N, Fi, Fo, R = 3, 8, 5, 6, 3
    xx = torch.randn(B, N, Fi, dtype=F64)
    rr = torch.randint(0, 1 << R, (B, N, N)).to(F64) * (torch.rand(B, N, N) < 0.4)
    WW, ro, bi = torch.randn(R, Fi, Fo, dtype=F64), torch.randn(Fi, Fo, dtype=F64), torch.randn(Fo, dtype=F64)
    ei, codes = bridge_edges(rr)
    d = dense_rgcn(xx, (rr > 0).to(F64), rr, WW, ro, bi).view(B * N, Fo)
    assert float((d - sparse_rgcn(xx.view(B * N, Fi), ei, codes, WW, ro, bi, mask_mode=True)).abs().max()) < 1e-13
    # an edge list with ids against the same list with the one-bit codes; out-of-range ids against code 0
    E = 60
    ei = torch.randint(0, B * N, (2, E))
    ids = torch.randint(-1, R + 2, (E,))
    one_bit = torch.where((ids >= 0) & (ids < R), 1 << ids.clamp(0, R - 1), 0)
    a = sparse_rgcn(xx.view(B * N, Fi), ei, ids, WW, ro, bi)
    b = sparse_rgcn(xx.view(B * N, Fi), ei, one_bit, WW, ro, bi, mask_mode=True)
    assert torch.equal(a, b)
    # duplicates count separately
    twice = sparse_rgcn(xx.view(B * N, Fi), torch.cat([ei, ei], 1), torch.cat([ids, ids]), WW, None, None, "add")
    assert torch.allclose(twice, 2 * sparse_rgcn(xx.view(B * N, Fi), ei, ids, WW, None, None, "add"), atol=1e-12)


def test_restatement_gradcheck():
    torch.manual_seed(2)
    B, N, Fi, Fo, R = 2, 5, 3, 4, 3
    rel = torch.randint(0, 1 << R, (B, N, N)).to(F64)
    args = [torch.randn(B, N, Fi, dtype=F64), torch.randn(B, N, N, dtype=F64), torch.randn(2, Fi, Fo, dtype=F64),
            torch.randn(Fi, Fo, dtype=F64), torch.randn(Fo, dtype=F64), torch.randn(R, 2, dtype=F64)]
    args = [a.requires_grad_() for a in args]
    for aggr in ("mean", "add"):
        assert torch.autograd.gradcheck(lambda x, adj, w, root, b, comp: dense_rgcn(x, adj, rel, w, root, b, aggr, None, comp),
                                        args)
    ei, codes = bridge_edges(rel)
    sargs = [args[0].detach().view(B * N, Fi).requires_grad_()] + args[2:]
    assert torch.autograd.gradcheck(lambda x, w, root, b, comp: sparse_rgcn(x, ei, codes, w, root, b, "mean", True, comp),
                                    sargs)


def test_typed_edge_restatement_by_hand():
    from oracle import dense as od
    sel = TypedEdgeRef([od.TemporalBackedge([1]), od.DenseEdge()], relations=[0, 2])
    adj, rel = torch.zeros(1, 3, 3), torch.zeros(1, 3, 3)
    adj[0, 1, 0], rel[0, 1, 0] = 1.0, 8.0                      # an older edge with a foreign bit
    a2, r2 = sel(torch.zeros(1, 3, 2), adj, rel, torch.tensor([2]), 1)
    assert a2[0].tolist() == [[0, 0, 1], [1, 0, 1], [1, 1, 1]]
    assert r2[0].tolist() == [[0, 0, 4], [8, 0, 4], [4, 5, 4]]
    assert sel.num_relations == 3


# ---- the preconditions of the GPU case tables ----------------------------------------------------------
_NAMED = {"mask", "two_d", "bcast", "weighted", "empty_relation", "empty_rows", "triple", "high_bits", "int64", "bit15"}


def test_case_tables_hold_the_required_shapes():
    shapes = {c[:5] for c in RC.DENSE}
    assert {(3, 7, 3, 5, 1), (3, 7, 3, 5, 3), (5, 1, 4, 3, 2), (2, 33, 8, 8, 2), (2, 70, 16, 12, 5), (1, 130, 6, 9, 3),
            (2, 40, 128, 128, 2), (2, 24, 16, 24, 16)} <= shapes
    opts = [c[5] for c in RC.DENSE]
    assert any(o.get("aggr") == "add" for o in opts) and any(o.get("num_bases") == 2 for o in opts)
    assert any(o.get("root_weight") is False for o in opts) and any(o.get("bias") is False for o in opts)
    assert any(o.get("no_adj_grad") for o in opts)
    assert _NAMED <= {k for o in opts for k in o}
    assert {c[:3] for c in RC.SPARSE} >= {(9, 0, 2), (20, 60, 3), (300, 2000, 5)}
    assert RC.DENSE[4][:5] == (2, 70, 16, 12, 5) and RC.DENSE[15][5] == {"weighted": True}   # test_rgcn_gpu's picks
    assert RC.SPARSE[3][3] == {"hub": True} and RC.SPARSE[1][3] == {}


def _lively_ref(Fi, Fo, R, opts):
    torch.manual_seed(0)
    ref = RGCNRef(Fi, Fo, R, **RC.layer_kwargs(opts))
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn_like(p) * 0.5)
    return ref


@pytest.mark.parametrize("case", RC.DENSE, ids=RC.dense_id)
def test_dense_cases_hold_what_they_name(case):
    B, N, Fi, Fo, R, opts = case
    ops = RC.dense_operands(case)
    assert _NAMED & set(opts) <= RC.dense_features(case, ops)
    ref = _lively_ref(Fi, Fo, R, opts)
    o32 = ref(ops["x"], ops["adj"], ops["rel"], ops["mask"])
    o64 = copy.deepcopy(ref).double()(ops["x"].double(), ops["adj"].double(), ops["rel"], ops["mask"])
    assert float(o64.abs().max()) >= 100 * bound(o64, o32)      # the output is large against its bound


@pytest.mark.parametrize("case", RC.SPARSE, ids=RC.sparse_id)
def test_sparse_cases_hold_what_they_name(case):
    M, E, R, opts = case
    ops = RC.sparse_operands(case)
    assert set(opts) <= RC.sparse_features(case, ops)
    ref = _lively_ref(6, 5, R, opts)
    for et, mask_mode in ((ops["ids"], False), (ops["codes"], True)):
        o32 = ref.sparse(ops["x"], ops["edge_index"], et, mask_mode)
        o64 = copy.deepcopy(ref).double().sparse(ops["x"].double(), ops["edge_index"], et, mask_mode)
        assert float(o64.abs().max()) >= 100 * bound(o64, o32)


@pytest.mark.parametrize("N", sorted(TC.PLANES))
def test_selector_planes_stay_off_their_thresholds(N):
    from oracle import dense as od
    p = TC.plane(N)
    assert TC.threshold_margin(p["nodes"], p["cur"]) >= 1e-3
    picked = [s(p["nodes"], torch.zeros_like(p["adj"]), torch.zeros(0), p["cur"], 3)[0] for s in TC.oracle_children()]
    assert all(float(a.sum()) > 0 for a in picked)                               # every child selects something
    assert bool((p["rel"].long() >> 3 > 0).any())                                # foreign bits to carry through


def test_typed_memory_seed_meets_its_conditions():
    (o64, h64, _), (o32, h32, _) = TC.memory_reference(False)
    rel = h64[2]
    m = bits(rel, TC.R)
    assert all(int(m[r].sum()) > 0 for r in range(TC.R))                         # every relation has edges
    assert bool((m.sum(0) >= 2).any())                                           # some entry carries two bits
    cnt = m.sum(-1)
    assert bool(((cnt == 0).sum(0) == 1).any())                                  # a row empty in one relation only
    assert TC.memory_margin() >= 1e-3                                            # SURVEY 8c's rule for G3
    assert torch.equal(h32[1].double(), h64[1]) and torch.equal(h32[2].double(), h64[2])
    assert int(h64[3].max()) == TC.N and TC.T > TC.N                             # past the overflow roll
    assert torch.equal(h64[1] > 0, rel > 0)
    (_, r64, _), _ = TC.memory_reference(True)
    assert r64[3].tolist() != h64[3].tolist()                                    # the reset run differs


def test_learned_child_seed_keeps_the_selection_margin():
    r64, r32 = TC.learned_reference()
    assert r64[3] >= 1e-3                                                        # tests/test_learned_det_gpu.py's MARGIN
    assert torch.equal(r32[1][1].double(), r64[1][1])
    vals = set(r64[1][2].flatten().tolist())
    assert {1.0, 2.0} <= vals | {3.0} and (2.0 in vals or 3.0 in vals)           # the learned relation is in use
    edge = [v for k, v in r64[2].items() if k.startswith("edge.") and k not in ("edge.5.bias", "edge.6.bias")]
    assert all(float(v.abs().max()) > 1e-3 for v in edge)                        # the adjacency gradient arrives
    assert all(float(r64[2][k].abs().max()) <= 1e-12 for k in ("edge.5.bias", "edge.6.bias"))
