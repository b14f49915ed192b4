"""Sparse spatial selectors on the MI355X (csrc/spatial.hip): parity with the reference's g17 fixtures, continuing
graphs and exact edge cases against the restatement of tests/test_spatial_sparse_cpu.py, SparseGCM end to end, and
the full cfg4 size."""
import pytest
import torch

from _golden import Fixture
from oracle import sparse as osp
from test_spatial_sparse_cpu import GCM_FIXTURES, SELECTOR_FIXTURES, position_spec, restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sel(kind, pos, radius=None, k=None, causal=True):
    from gcm.sparse_edge_selectors.spatial import SpatialKNNEdge, SpatialRadiusEdge
    if kind == "knn":
        return SpatialKNNEdge(pos, k, causal=causal)
    return SpatialRadiusEdge(pos, radius, causal=causal)


def _run(sel, nodes, T, taus):
    B = nodes.shape[0]
    out = sel(nodes.to(DEV), T.to(DEV), taus.to(DEV), B)
    assert out.is_sparse and out.is_coalesced()
    assert tuple(out.shape) == (B, nodes.shape[1], nodes.shape[1])
    assert out.values().dtype == torch.float32 and bool((out.values() == 1).all())
    idx = out.indices().cpu()
    bptr = out.gcm_bptr.cpu()
    assert bptr.shape == (B + 1,) and int(bptr[-1]) == idx.shape[1]
    assert torch.equal(bptr[1:] - bptr[:-1], torch.bincount(idx[0], minlength=B))
    return idx


@pytest.mark.parametrize("name", SELECTOR_FIXTURES)
def test_selector_matches_reference_fixture(name):
    fx = Fixture(name)
    m = fx.meta
    sel = _sel(m["kind"], position_spec(m["pos"]), m.get("radius"), m.get("k"), m.get("causal", True))
    idx = _run(sel, fx["nodes"], fx["T"], fx["taus"])
    assert torch.equal(idx, fx["indices"])       # same set, same (coalesced) order


def _continuing_case(seed, B, N, P, F=5):
    g = torch.Generator().manual_seed(seed)
    T = torch.randint(0, N // 2, (B,), generator=g)
    taus = torch.randint(0, N // 2, (B,), generator=g)
    taus[0] = 0                              # a graph without new nodes
    T[1], taus[1] = 0, 1                     # T + tau = 1
    T[2], taus[2] = 1, 0
    taus = torch.minimum(taus, N - T)
    nodes = torch.rand(B, N, F, generator=g)
    return nodes, T, taus


@pytest.mark.parametrize("seed,B,N,P", [(0, 7, 40, 2), (1, 5, 100, 3), (2, 9, 130, 16), (3, 4, 257, 2),
                                        (4, 3, 600, 5)])
def test_continuing_graphs_match_restatement(seed, B, N, P):
    nodes, T, taus = _continuing_case(seed, B, N, P, F=max(P, 5))
    cols = list(range(P))
    for radius in (0.3, 0.6):
        for causal in (True, False):
            got = _run(_sel("radius", slice(0, P), radius=radius, causal=causal), nodes, T, taus)
            assert torch.equal(got, restate(nodes, T, taus, cols, "radius", radius=radius, causal=causal))
    for k in (1, 3, 8, 64, N + 5):
        got = _run(_sel("knn", slice(0, P), k=k), nodes, T, taus)
        assert torch.equal(got, restate(nodes, T, taus, cols, "knn", k=k)), k


def test_integer_grid_radius_is_strict():
    """positions on an integer grid: distance exactly 1.0 is NOT within radius 1.0 (strict <), sqrt(2) neither"""
    xs = torch.tensor([[0., 0.], [1., 0.], [0., 1.], [1., 1.], [2., 0.], [0.5, 0.]])
    nodes = torch.cat([xs, torch.zeros(6, 1)], dim=1)[None]
    T, taus = torch.tensor([0]), torch.tensor([6])
    got = _run(_sel("radius", slice(0, 2), radius=1.0), nodes, T, taus)
    assert torch.equal(got, restate(nodes, T, taus, [0, 1], "radius", radius=1.0))
    assert got.T.tolist() == [[0, 5, 0], [0, 5, 1]]
    got = _run(_sel("radius", slice(0, 2), radius=1.0000001), nodes, T, taus)
    assert [0, 1, 0] in got.T.tolist()


def test_knn_ties_go_to_the_lower_index():
    pos = torch.tensor([[0.], [1.], [1.], [0.], [1.], [0.]])      # duplicates
    nodes = pos[None]
    T, taus = torch.tensor([0]), torch.tensor([6])
    for k in (1, 2, 3, 4):
        got = _run(_sel("knn", [0], k=k), nodes, T, taus)
        assert torch.equal(got, restate(nodes, T, taus, [0], "knn", k=k)), k
    # k = 2: node 3 (at 0) takes {0, 3} -> source 0; node 4 (at 1) takes {1, 2} -> 1, 2; node 5 takes {0, 3}
    got = _run(_sel("knn", [0], k=2), nodes, T, taus)
    assert got.T.tolist() == [[0, 2, 1], [0, 3, 0], [0, 4, 1], [0, 4, 2], [0, 5, 0], [0, 5, 3]]


def test_knn_k_larger_than_graph():
    nodes, T, taus = _continuing_case(11, 4, 20, 2)
    got = _run(_sel("knn", slice(0, 2), k=1000), nodes, T, taus)
    assert torch.equal(got, restate(nodes, T, taus, [0, 1], "knn", k=1000))
    assert got.shape[1] == sum(sum(range(int(t), int(t + u))) for t, u in zip(T, taus))    # every j < i


def test_all_empty_call():
    nodes = torch.rand(3, 8, 2)
    for T, taus in ((torch.tensor([0, 1, 0]), torch.tensor([1, 0, 0])), (torch.tensor([3, 4, 0]), torch.zeros(3, dtype=torch.long))):
        for sel in (_sel("knn", slice(0, 2), k=3), _sel("radius", slice(0, 2), radius=10.0),
                    _sel("radius", slice(0, 2), radius=10.0, causal=False)):
            assert _run(sel, nodes, T, taus).shape == (3, 0)


def test_knn_noncausal_raises():
    with pytest.raises(NotImplementedError):
        _sel("knn", slice(0, 2), k=3, causal=False)(torch.rand(2, 4, 2, device=DEV),
                                                     torch.zeros(2, dtype=torch.long, device=DEV),
                                                     torch.full((2,), 3, dtype=torch.long, device=DEV), 2)


def test_selector_rejects_cpu_tensors():
    from gcm._hip import HipLibraryError
    with pytest.raises(HipLibraryError):
        _sel("radius", slice(0, 2), radius=0.5)(torch.rand(2, 4, 2), torch.zeros(2, dtype=torch.long),
                                                 torch.full((2,), 3, dtype=torch.long), 2)


def _dev_gnn(ref, F, H):
    from gcm import nn as G
    g = G.Sequential("x, edges, weights", [(G.GraphConv(F, H), "x, edges, weights -> x"), torch.nn.Tanh(),
                                            (G.GraphConv(H, H), "x, edges, weights -> x"), torch.nn.Tanh()])
    g.load_state_dict(ref.state_dict())
    return g.to(DEV)


def _module(spec):
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    if spec["kind"] == "temporal":
        return TemporalEdge(spec["hops"])
    return _sel(spec["kind"], position_spec(spec["pos"]), spec.get("radius"), spec.get("k"),
                spec.get("causal", True))


def test_noncausal_radius_inside_sparse_gcm_violates_causality():
    """sparse_gcm.py:171: the non-causal selector's self edges (source == sink) fail the reference's assert"""
    from gcm.sparse_gcm import SparseGCM
    ref = osp.canonical_gnn(2, 4, act=torch.nn.Tanh)
    mem = SparseGCM(_dev_gnn(ref, 2, 4), edge_selectors=_sel("radius", slice(0, 2), radius=0.5, causal=False),
                    graph_size=8)
    with pytest.raises(AssertionError, match="Causality violated"):
        mem(torch.rand(2, 3, 2, device=DEV), torch.full((2,), 3, dtype=torch.long, device=DEV), None)


@pytest.mark.parametrize("name", GCM_FIXTURES)
def test_sparse_gcm_matches_reference_fixture(name):
    from gcm.sparse_gcm import SparseGCM
    fx = Fixture(name)
    m = fx.meta
    ref = osp.canonical_gnn(m["F"], m["H"], act=torch.nn.Tanh)
    ref.load_state_dict(fx.group("param:"))
    g = _dev_gnn(ref, m["F"], m["H"])
    mem = SparseGCM(g, edge_selectors=_module(m["main"]), aux_edge_selectors=_module(m["aux"]), graph_size=m["N"])
    obs = fx["obs"].to(DEV).requires_grad_(True)
    B = m["B"]
    hidden, outs, pos = None, [], torch.zeros(B, dtype=torch.long)
    for taus in fx["taus"]:
        t = int(taus.max())
        rows = [torch.cat([obs[b, pos[b]: pos[b] + taus[b]],
                           torch.zeros(t - int(taus[b]), m["F"], device=DEV)]) for b in range(B)]
        out, hidden = mem(torch.stack(rows), taus.to(DEV), hidden)
        outs.append(out)
        pos = pos + taus
    loss = sum(o.sum() for o in outs) / sum(o.numel() for o in outs)
    loss.backward()
    for i, o in enumerate(outs):
        torch.testing.assert_close(o.cpu(), fx[f"out{i}"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(hidden[0].detach().cpu(), fx["hT_nodes"], rtol=1e-5, atol=0)
    assert torch.equal(hidden[1].coalesce().indices().cpu(), fx["hT_adj_indices"])        # exact
    assert torch.equal(hidden[1].coalesce().values().cpu(), fx["hT_adj_values"])
    assert torch.equal(hidden[2].cpu(), fx["hT_T"])
    gs = float(fx["grad_obs"].abs().max())
    torch.testing.assert_close(obs.grad.cpu(), fx["grad_obs"], rtol=1e-5, atol=1e-5 * gs)
    for k, p in g.named_parameters():
        want = fx["grad:" + k]
        torch.testing.assert_close(p.grad.cpu(), want, rtol=1e-5, atol=1e-5 * float(want.abs().max()) + 1e-7, msg=k)


def test_full_size_matches_restatement():
    """cfg4's shape one shot: B = 512 graphs of 512 nodes, P = 2; radius for ~8 edges per sink, k = 8"""
    g = torch.Generator().manual_seed(4)
    B, N, F = 512, 512, 4
    nodes = torch.rand(B, N, F, generator=g)
    T = torch.zeros(B, dtype=torch.long)
    taus = torch.full((B,), N, dtype=torch.long)
    radius = 0.1       # pi r^2 * i sources within reach of sink i: ~8 on average over a graph's sinks
    got_r = _run(_sel("radius", slice(0, 2), radius=radius), nodes, T, taus)
    got_k = _run(_sel("knn", slice(0, 2), k=8), nodes, T, taus)
    assert 4 * B * N < got_r.shape[1] < 16 * B * N
    want_r, want_k = [], []
    for b in range(B):          # per graph on the CPU (the restatement's loop, one graph at a time)
        one = slice(b, b + 1)
        wr = restate(nodes[one], T[one], taus[one], [0, 1], "radius", radius=radius)
        wk = restate(nodes[one], T[one], taus[one], [0, 1], "knn", k=8)
        wr[0], wk[0] = b, b
        want_r.append(wr)
        want_k.append(wk)
    assert torch.equal(got_r, torch.cat(want_r, dim=1))
    assert torch.equal(got_k, torch.cat(want_k, dim=1))
