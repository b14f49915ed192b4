"""Sparse spatial selectors (gcm.sparse_edge_selectors.spatial) without a GPU: the constructors against the
reference's, the host-side resolution of position slices, and the g17 fixtures (outputs of the reference's own
selectors and SparseGCM, tests/golden/make_golden_spatial.py) against a brute-force restatement of the semantics
DESIGN.md §3.13 pins.  The restatement is shared with tests/test_spatial_sparse_gpu.py."""
import glob
import inspect
import os

import pytest
import torch

from _golden import GOLDEN, Fixture


# ---------------------------------------------------------------------------------------------------------------
# brute-force restatement (per graph, fp32 like the reference's formula)
# ---------------------------------------------------------------------------------------------------------------
def position_spec(spec):
    """the position_slice a fixture's meta describes"""
    if "slice" in spec:
        return slice(*spec["slice"])
    return list(spec["cols"])


def _d2(pos):
    """[n, n] fp32 squared distances: (x_i - x_j)^2 added in column order, each step rounded to fp32"""
    n = pos.shape[0]
    s = torch.zeros(n, n, dtype=torch.float32)
    for p in range(pos.shape[1]):
        d = pos[:, None, p] - pos[None, :, p]
        s = s + d * d
    return s


def restate(nodes, T, taus, cols, kind, radius=None, k=None, causal=True):
    """COO indices [3, E] (batch, sink, source) in coalesced order.
    radius, causal     sink i new, source j < i, sqrt(d2) < float32(radius)
    radius, non-causal sink j in [0, n), source i new, same predicate (self edges included)
    knn (causal)       sink i new, the min(k, n) smallest (d2, j) over all of [0, n), sources j < i kept
                       (sink = T_b + local index: the deliberate deviation from the reference at T_b > 0)
    no edges at all when max(T + taus) <= 1."""
    nodes = nodes.float().cpu()
    T, taus = T.cpu(), taus.cpu()
    B = nodes.shape[0]
    out = []
    if int((T + taus).max()) <= 1:
        return torch.zeros(3, 0, dtype=torch.long)
    r32 = torch.tensor(float(radius) if radius is not None else 0.0, dtype=torch.float32)
    for b in range(B):
        t0, n = int(T[b]), int(T[b] + taus[b])
        if n == 0:
            continue
        d2 = _d2(nodes[b, :n][:, cols])
        rows = torch.arange(n)[:, None]
        colsj = torch.arange(n)[None, :]
        new_row = rows >= t0
        if kind == "radius":
            # correctly rounded fp32 sqrt on every host: the fp64 root of an fp32 value rounded to fp32 (torch's
            # vectorised fp32 sqrt is 1 ulp off for some inputs on some CPUs)
            near = torch.sqrt(d2.double()).float() < r32
            if causal:
                mask = near & new_row & (colsj < rows)
            else:
                mask = near & (colsj >= t0)       # rows: every node j (the sink), columns: new nodes i (the source)
        else:
            kk = min(int(k), n)
            order = torch.sort(d2, dim=1, stable=True).indices[:, :kk]
            sel = torch.zeros(n, n, dtype=torch.bool)
            sel.scatter_(1, order, True)
            mask = sel & new_row & (colsj < rows)
        ij = mask.nonzero()
        out.append(torch.stack([torch.full((ij.shape[0],), b, dtype=torch.long), ij[:, 0], ij[:, 1]]))
    return torch.cat(out, dim=1) if out else torch.zeros(3, 0, dtype=torch.long)


SELECTOR_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "g17_sparse_spatial_*.npz"))
                           if "_gcm_" not in p)
GCM_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "g17_sparse_spatial_gcm_*.npz")))


def restate_fixture(fx):
    m = fx.meta
    from gcm.sparse_edge_selectors.spatial import resolve_columns
    cols = resolve_columns(position_spec(m["pos"]), fx["nodes"].shape[-1])
    return restate(fx["nodes"], fx["T"], fx["taus"], cols, m["kind"], radius=m.get("radius"), k=m.get("k"),
                   causal=m.get("causal", True))


# ---------------------------------------------------------------------------------------------------------------
def test_module_imports_and_constructors_match_reference():
    """spatial.py:13-18, 66-71: same parameters, defaults and attribute names."""
    from gcm.sparse_edge_selectors.spatial import SpatialKNNEdge, SpatialRadiusEdge
    sk = inspect.signature(SpatialKNNEdge.__init__).parameters
    assert list(sk) == ["self", "position_slice", "k", "causal"]
    assert sk["k"].default is inspect.Parameter.empty and sk["causal"].default is True
    sr = inspect.signature(SpatialRadiusEdge.__init__).parameters
    assert list(sr) == ["self", "position_slice", "radius", "causal"]
    assert sr["radius"].default == 0.25 and sr["causal"].default is True
    k = SpatialKNNEdge(slice(0, 2), 5)
    assert (k.position_slice, k.k, k.causal) == (slice(0, 2), 5, True)
    r = SpatialRadiusEdge([0, 2])
    assert (r.position_slice, r.radius, r.causal) == ([0, 2], 0.25, True)
    assert isinstance(k, torch.nn.Module) and isinstance(r, torch.nn.Module)
    # SparseGCM's no-sort merge: only when every edge ends in a new node
    assert SpatialKNNEdge(slice(0, 2), 3).new_sinks_only
    assert SpatialRadiusEdge(slice(0, 2)).new_sinks_only
    assert not SpatialRadiusEdge(slice(0, 2), causal=False).new_sinks_only


@pytest.mark.parametrize("spec,F,want", [
    (slice(0, 2), 6, [0, 1]), (slice(1, 4), 6, [1, 2, 3]), (slice(0, 6, 2), 6, [0, 2, 4]),
    (slice(None, None, -2), 6, [5, 3, 1]), (slice(-3, None), 6, [3, 4, 5]), (slice(-5, -1, 3), 6, [1, 4]),
    (slice(2, 100), 5, [2, 3, 4]), (slice(None), 3, [0, 1, 2]), ([4, 1], 6, [4, 1]), ([-1, 0], 6, [5, 0]),
    ((2, 3), 6, [2, 3]), (torch.tensor([1, 3]), 6, [1, 3]), (slice(3, 1), 6, []),
])
def test_resolve_columns(spec, F, want):
    from gcm.sparse_edge_selectors.spatial import resolve_columns
    assert resolve_columns(spec, F) == want
    if isinstance(spec, slice) and (spec.step or 1) > 0:
        assert want == torch.arange(F)[spec].tolist()       # what nodes[..., slice] selects


def test_resolve_columns_rejects_out_of_range():
    from gcm.sparse_edge_selectors.spatial import resolve_columns
    with pytest.raises(IndexError):
        resolve_columns([0, 6], 6)
    with pytest.raises(IndexError):
        resolve_columns([-7], 6)


def test_fixtures_exist():
    assert len(SELECTOR_FIXTURES) >= 12, SELECTOR_FIXTURES
    assert len(GCM_FIXTURES) >= 4, GCM_FIXTURES
    kinds = {Fixture(n).meta["kind"] for n in SELECTOR_FIXTURES}
    assert kinds == {"knn", "radius"}
    assert any(int(Fixture(n)["T"].max()) > 0 for n in SELECTOR_FIXTURES)


@pytest.mark.parametrize("name", SELECTOR_FIXTURES)
def test_selector_fixture_matches_restatement(name):
    fx = Fixture(name)
    want = restate_fixture(fx)
    assert torch.equal(fx["indices"], want), (fx["indices"], want)
    assert torch.equal(fx["values"], torch.ones(want.shape[1]))
    B, N = fx["nodes"].shape[:2]
    assert fx["size"].tolist() == [B, N, N]


@pytest.mark.parametrize("name", GCM_FIXTURES)
def test_gcm_fixture_adjacency_matches_restatement(name):
    """the reference SparseGCM's final adjacency = the union over its calls of the spatial edges and the
    TemporalEdge([1]) edges, each call on the node matrix of that call"""
    fx = Fixture(name)
    m = fx.meta
    B, N, F = m["B"], m["N"], m["F"]
    obs, plan = fx["obs"], fx["taus"]
    from gcm.sparse_edge_selectors.spatial import resolve_columns
    nodes = torch.zeros(B, N, F)
    T = torch.zeros(B, dtype=torch.long)
    edges = set()
    for taus in plan:
        for b in range(B):
            nodes[b, T[b]: T[b] + taus[b]] = obs[b, T[b]: T[b] + taus[b]]
        for spec in (m["main"], m["aux"]):
            if spec["kind"] == "temporal":
                for b in range(B):
                    for i in range(int(T[b]), int(T[b] + taus[b])):
                        edges.update((b, i, i - h) for h in spec["hops"] if i - h >= 0 and i > 0)
            else:
                cols = resolve_columns(position_spec(spec["pos"]), F)
                idx = restate(nodes, T, taus, cols, spec["kind"], radius=spec.get("radius"), k=spec.get("k"))
                edges.update(map(tuple, idx.T.tolist()))
        T = T + taus
    want = torch.tensor(sorted(edges), dtype=torch.long).T
    assert torch.equal(fx["hT_adj_indices"], want)
    assert torch.equal(fx["hT_T"], T)


def test_restatement_knn_continuing_graph_uses_absolute_sinks():
    """the T > 0 decision: sink = T_b + local index, sources below it (the reference would emit rows 0..tau-1)"""
    nodes = torch.tensor([[[0.0], [10.0], [0.1], [10.1]]])
    idx = restate(nodes, torch.tensor([2]), torch.tensor([2]), [0], "knn", k=2)
    assert idx.T.tolist() == [[0, 2, 0], [0, 3, 1]]
