"""KNNEdge host side: constructor checks, the mode encoding, the selector descriptor, where DenseGCM's structure
analysis places it, the C ABI section (include/gcm_hip_knn.h) and its validation without a device, and the properties
of the restatement the GPU tests compare against (tests/_knn_restate.py).  No kernel runs."""
import ctypes
import math
import os
import re

import pytest
import torch

import _knn_restate as R
from gcm.edge_selectors.knn import KNNEdge      # (without the selector nothing here is worth running)
from gcm.edge_selectors.distance import Distance, SpatialEdge


# ---- constructor --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, -1, 256, 1000, 2.0, "3", None, True])
def test_k_outside_1_to_255_raises(k):
    with pytest.raises(ValueError, match="k must be"):
        KNNEdge(k)


def test_unknown_metric_and_cosine_slices_raise():
    with pytest.raises(ValueError, match="metric"):
        KNNEdge(3, metric="l1")
    with pytest.raises(ValueError, match="cosine"):
        KNNEdge(3, slice(0, 3), metric="cosine")
    with pytest.raises(ValueError, match="cosine"):
        KNNEdge(3, None, slice(0, 3), metric="cosine")
    with pytest.raises(TypeError):
        KNNEdge(3, learned=True)                 # not offered: scaling does not change a ranking
    KNNEdge(1), KNNEdge(255), KNNEdge(3, metric="cosine"), KNNEdge(3, slice(0, 3), slice(2, 5), 0.5, "l2", True)


def test_strided_slice_raises_like_spatial_edge():
    for sel in (KNNEdge(3, slice(0, 6, 2)), SpatialEdge(1.0, slice(0, 6, 2))):
        with pytest.raises(NotImplementedError, match="contiguous"):
            sel._slices(8)
    assert KNNEdge(3)._slices(8) == ((0, 8), (0, 8))                  # None: all features
    assert KNNEdge(3, slice(1, 4))._slices(8) == ((1, 4), (1, 4))
    assert KNNEdge(3, slice(1, 4), slice(5, 8))._slices(8) == ((1, 4), (5, 8))
    assert KNNEdge(3, slice(0, 3))._slices(8) == SpatialEdge(1.0, slice(0, 3))._slices(8)


# ---- mode encoding, descriptor -----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 255])
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_mode_round_trips(k, metric):
    from gcm import _hip
    assert (_hip.DIST_KNN_SHIFT, _hip.DIST_KNN_MAX) == (8, 255)
    mode = KNNEdge(k, metric=metric).mode
    want_metric = {"l2": _hip.DIST_L2_PERGRAPH, "cosine": _hip.DIST_COSINE_SIM}[metric]
    assert mode & 0xFF == want_metric and mode >> _hip.DIST_KNN_SHIFT == k and mode < 1 << 16
    assert mode != _hip.DIST_EUCLID_CROSSBATCH                        # the EuclideanEdge fast paths test equality
    # k = 0 is the threshold selector's own mode, byte for byte
    assert SpatialEdge.mode == _hip.DIST_L2_PERGRAPH == KNNEdge(k).mode & 0xFF


def test_is_a_distance_and_its_descriptor():
    from gcm import _hip
    sel = KNNEdge(3)
    assert isinstance(sel, Distance) and isinstance(sel, torch.nn.Module)
    assert not sel.learned and not list(sel.parameters())
    d = KNNEdge(5, slice(1, 4), slice(2, 5), max_distance=0.75, bidirectional=True).native_desc(8)
    assert (d.kind, d.mode) == (_hip.SEL_DISTANCE, _hip.DIST_L2_PERGRAPH | 5 << 8)
    assert (d.a0, d.a1, d.b0, d.b1, d.bidirectional) == (1, 4, 2, 5, 1)
    assert d.max_distance == 0.75 and not d.dist_param and not d.cur_rows and d.n_cur_rows == 0
    d = KNNEdge(200, metric="cosine").native_desc(8)
    assert d.mode == _hip.DIST_COSINE_SIM | 200 << 8 and math.isinf(d.max_distance) and d.max_distance > 0
    assert (d.a0, d.a1, d.b0, d.b1, d.bidirectional) == (0, 8, 0, 8, 0)
    assert KNNEdge(3).pointer_source() == (None, None, 0)
    assert "k=3" in repr(KNNEdge(3))


# ---- DenseGCM's structure analysis ---------------------------------------------------------------------
def _memory(sel, aux=None, fused=True):
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    g = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(8, 8), "x, adj -> x"), torch.nn.Tanh(),
                                               (G.DenseGraphConv(8, 8), "x, adj -> x"), torch.nn.Tanh()])
    return DenseGCM(g, edge_selectors=sel, aux_edge_selectors=aux, graph_size=16, fused=fused)


def _after_backedge(sel):
    from gcm import nn as G
    from gcm.edge_selectors.temporal import TemporalBackedge
    sig = "nodes, adj, weights, num_nodes, B"
    step = "nodes, adj, weights, num_nodes, B -> adj, weights"
    return G.Sequential(sig, [(TemporalBackedge([1]), step), (sel, step)])


def test_structure_is_fused_exactly_where_spatial_edge_is():
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.edge_selectors.dense import DenseEdge

    def pair():
        return KNNEdge(3, slice(0, 3)), SpatialEdge(1.0, slice(0, 3))

    for build in (lambda s: _memory(s), lambda s: _memory(_after_backedge(s)),
                  lambda s: _memory(s, fused=False),
                  lambda s: _memory(s, aux=TemporalBackedge([2])), lambda s: _memory(s, aux=DenseEdge())):
        knn, spatial = pair()
        assert (build(knn)._structure() is None) == (build(spatial)._structure() is None)
    assert _memory(KNNEdge(3, slice(0, 3)))._structure() is not None
    assert _memory(KNNEdge(3, metric="cosine"))._structure() is not None
    assert _memory(_after_backedge(KNNEdge(3, slice(0, 3))))._structure() is not None
    knn = KNNEdge(3, slice(0, 3))
    assert _memory(knn)._structure()[2] == [knn]
    assert _memory(KNNEdge(3, slice(0, 3)), fused=False)._structure() is None
    # the selector as aux_edge_selectors: the layered path, as for every Distance there
    assert (_memory(TemporalBackedge([1]), aux=KNNEdge(3, slice(0, 3)))._structure() is None) == \
           (_memory(TemporalBackedge([1]), aux=SpatialEdge(1.0, slice(0, 3)))._structure() is None)


# ---- the C ABI -------------------------------------------------------------------------------------------
def test_header_section_and_library():
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_knn.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    text = _abi.header("gcm_hip_knn.h")
    assert set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", text)) == {"gcm_edge_knn_supported"} == set(_hip.KNN_PROTOTYPES)
    assert _abi.constants(text) == {"GCM_DIST_KNN_SHIFT": 8, "GCM_DIST_KNN_MAX": 255}
    assert "gcm_edge_knn_supported" not in _hip.PROTOTYPES
    assert len(_hip.PROTOTYPES) == 150                                 # no prototype of gcm_hip.h itself changed
    lib = _hip.lib()
    assert lib.gcm_abi_version() == 8 == _hip.ABI_VERSION            # the section is additive
    fn = lib.gcm_edge_knn_supported
    assert (fn.restype, fn.argtypes) == _hip.KNN_PROTOTYPES["gcm_edge_knn_supported"]
    L2, COS, EUC = _hip.DIST_L2_PERGRAPH, _hip.DIST_COSINE_SIM, _hip.DIST_EUCLID_CROSSBATCH
    assert fn(L2 | 8 << 8, 256, 128, 32) == 1 and fn(COS | 255 << 8, 1, 1, 1) == 1 and fn(L2 | 1 << 8, 2, 8192, 5) == 1
    for mode in (L2, COS, EUC, EUC | 8 << 8, 3 | 8 << 8, L2 | 256 << 8, -1):
        assert fn(mode, 4, 16, 8) == 0, mode
    assert fn(L2 | 8 << 8, 0, 16, 8) == 0 and fn(L2 | 8 << 8, 4, 0, 8) == 0 and fn(L2 | 8 << 8, 4, 16, 0) == 0
    assert fn(L2 | 8 << 8, 4, 8193, 8) == 0
    for mode in (L2 | 8 << 8, COS | 8 << 8, EUC | 8 << 8):            # no scratch
        assert lib.gcm_edge_distance_workspace_bytes(mode, 256, 128, 32) == 0


def test_c_abi_validates_without_a_device():
    """What the host rejects before anything is launched (the pointers are host memory that no kernel may touch)."""
    from gcm import _hip
    lib = _hip.lib()
    B, N, F = 2, 8, 4
    nodes = (ctypes.c_float * (B * N * F))()
    adj = (ctypes.c_float * (B * N * N))()
    row = (ctypes.c_float * (B * N))()
    cur = (ctypes.c_int64 * B)()
    p = ctypes.addressof
    L2, COS, EUC = _hip.DIST_L2_PERGRAPH, _hip.DIST_COSINE_SIM, _hip.DIST_EUCLID_CROSSBATCH
    EINVAL, EUNSUPPORTED = _hip._CONSTANTS["GCM_EINVAL"], _hip.GCM_EUNSUPPORTED

    def ex(mode, a=(0, F), b=(0, F), cur_rows=None, n_rows=0, N_=N):
        return lib.gcm_edge_distance_ex(p(nodes), p(adj), p(cur), mode, 1.0, None, a[0], a[1], b[0], b[1], 0, None,
                                        cur_rows, n_rows, None, 0, B, N_, F, None)

    def pre(mode, cur_rows=None, n_rows=0):
        return lib.gcm_edge_distance_pre_ex(p(nodes), p(cur), p(nodes), p(row), mode, 1.0, None, 0, F, 0, F,
                                            cur_rows, n_rows, None, 0, B, N, F, None)

    assert ex(EUC | 3 << 8) == EINVAL and pre(EUC | 3 << 8) == EINVAL              # no cross-batch kNN
    assert ex(3 | 3 << 8) == EINVAL and ex(L2 | 256 << 8) == EINVAL and ex(-1) == EINVAL
    assert ex(L2 | 3 << 8, cur_rows=p(nodes), n_rows=2) == EINVAL                   # gathered current rows
    assert pre(COS | 3 << 8, cur_rows=p(nodes), n_rows=2) == EINVAL
    assert ex(L2 | 3 << 8, a=(0, 3), b=(0, 2)) == EINVAL and ex(L2 | 3 << 8, a=(2, 6), b=(2, 6)) == EINVAL
    assert ex(L2 | 3 << 8, N_=8193) == EUNSUPPORTED


# ---- the restatement ---------------------------------------------------------------------------------------
def test_restated_in_degree_is_min_k_cur_without_a_cap():
    torch.manual_seed(0)
    B, N, F = 5, 12, 4
    nodes = torch.rand(B, N, F)
    for metric, a in (("l2", slice(0, 3)), ("l2", None), ("cosine", None)):
        for k in (1, 3, 200):
            for cur in (torch.tensor([0, 1, 3, 7, 11]), torch.tensor([11, 2, 0, 5, 4])):
                sel = R.KNNSelector(k, a, metric=metric).select(nodes, cur)
                assert sel.sum(1).tolist() == [float(min(k, int(c))) for c in cur]
                assert all(float(sel[g, int(cur[g]):].sum()) == 0.0 for g in range(B))   # only stored rows j < cur
                # a cap only removes: the capped selection is the uncapped one filtered by distance
                d = R.KNNSelector(k, a, metric=metric).distances(nodes, cur)
                capped = R.KNNSelector(k, a, max_distance=0.6, metric=metric).select(nodes, cur)
                assert torch.equal(capped, sel * (d < 0.6))


def test_restated_ties_go_to_the_lower_index_and_nan_is_never_selected():
    nodes = torch.zeros(1, 8, 3)
    nodes[0, :7] = torch.tensor([[1., 0, 0], [0, 1, 0], [2, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 0]])
    cur = torch.tensor([6])          # rows 0, 1, 3, 4, 5 at distance 1; row 2 at distance 2
    for metric, want in (("l2", {1: [0], 2: [0, 1], 3: [0, 1, 3], 5: [0, 1, 3, 4, 5], 6: [0, 1, 2, 3, 4, 5]}),):
        for k, rows in want.items():
            sel = R.KNNSelector(k, metric=metric).select(nodes, cur)
            assert torch.nonzero(sel[0]).flatten().tolist() == rows, (k, sel)
    dup = torch.rand(1, 8, 4) + 0.1
    dup[0, 3] = dup[0, 1]
    dup[0, 6] = 2.0 * dup[0, 1]      # the same direction as rows 1 and 3: cosine distance 0 for all three
    dup[0, 7] = dup[0, 1]
    sel = R.KNNSelector(2, metric="cosine").select(dup, torch.tensor([7]))
    assert torch.nonzero(sel[0]).flatten().tolist() == [1, 3]
    nodes[0, 1, 0] = float("nan")
    sel = R.KNNSelector(6, metric="l2").select(nodes, cur)
    assert torch.nonzero(sel[0]).flatten().tolist() == [0, 2, 3, 4, 5]
    # the row the new node lands in is empty at cur == 0, whatever k
    adj, _ = R.KNNSelector(200)(torch.rand(2, 4, 3), torch.zeros(2, 4, 4), torch.zeros(0), torch.tensor([0, 2]), 2)
    assert float(adj[0].sum()) == 0.0 and adj[1, 2].tolist() == [1.0, 1.0, 0.0, 0.0] and float(adj[1].sum()) == 2.0


def test_restated_selector_drives_the_oracle_memory():
    """The plug-in signature: in-degree min(k, cur) in the oracle's DenseGCM, wrap-around included; bidirectional
    mirrors the row into the column."""
    from oracle import dense as od
    torch.manual_seed(1)
    B, N, F, T, k = 2, 6, 4, 9, 2
    gnn = od.canonical_gnn(F, 4)
    for bidir in (False, True):
        hid = None
        for t in range(T):
            _, hid = od.dense_step(torch.rand(B, F), hid, gnn, graph_size=N,
                                   edge_selectors=R.KNNSelector(k, slice(0, 2), bidirectional=bidir))
            cur = min(t, N - 1)
            assert hid[1][:, cur].sum(1).tolist() == [float(min(k, cur))] * B
            if bidir:
                assert torch.equal(hid[1][:, :, cur], hid[1][:, cur, :])
