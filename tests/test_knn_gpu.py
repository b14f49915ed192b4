"""KNNEdge on the GPU (csrc/knn.hip): the selector alone in both forms of its kernel (advanced state / state before
the step), exact ties, the sparse twin, DenseGCM on every driver against the oracle run with the restated selector
(tests/_knn_restate.py), the per-step path it takes, and the threshold selectors unchanged.  Needs an MI355X."""
import os

import numpy as np
import pytest
import torch

import _knn_restate as R
from gcm.edge_selectors.knn import KNNEdge
from gcm.edge_selectors.distance import CosineEdge, SpatialEdge
from oracle import dense as od

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------
# both forms of the kernel on the same case
# ---------------------------------------------------------------------------------------------------------
def _advanced(sel, nodes, cur, adj0=None):
    """The selector as DenseGCM's layered path calls it: nodes hold the current node in row cur.  -> (adj, dist)"""
    B, N, _ = nodes.shape
    adj = torch.zeros(B, N, N) if adj0 is None else adj0.clone()
    nd, cd = nodes.to(DEV), cur.to(DEV)
    out, _ = sel(nd, adj.to(DEV), torch.zeros(0, device=DEV), cd, B)
    return out.cpu(), sel.distances(nd, cd).cpu()


def _pre(sel, nodes, cur, full=None):
    """The same case as the state BEFORE the step (gcm_edge_distance_pre_ex, what the live-row step calls): the
    current node is the observation; a graph listed in `full` comes in with count == N, so its image row j is stored
    row j + 1 and the node lands in row N - 1 (cur must be N - 1 there).  -> decision row [B, N], prefilled with 7."""
    from gcm import _hip
    B, N, F = nodes.shape
    obs = nodes[torch.arange(B), cur].clone()
    stored, count = nodes.clone(), cur.clone()
    for b in (full or ()):
        assert int(cur[b]) == N - 1
        stored[b, 1:] = nodes[b, :N - 1]
        stored[b, 0] = 123.0                                    # the node the roll drops
        count[b] = N
    for b in range(B):
        if b not in (full or ()):
            stored[b, int(cur[b]):] = -55.0                     # rows the "pre" form must not read as candidates
    row = torch.full((B, N), 7.0, device=DEV)
    sd, cd, xd = stored.to(DEV), count.to(DEV), obs.to(DEV)
    a, b_ = sel._slices(F)
    rc = _hip.lib().gcm_edge_distance_pre_ex(sd.data_ptr(), cd.data_ptr(), xd.data_ptr(), row.data_ptr(), sel.mode,
                                             float(sel.max_distance), None, a[0], a[1], b_[0], b_[1], None, 0, None, 0,
                                             B, N, F, _hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return row.cpu()


def _case(B, N, F, curs, seed):
    g = torch.Generator().manual_seed(seed)
    nodes = torch.rand(B, N, F, generator=g) - 0.3
    return nodes, torch.tensor(curs)


_SHAPES = {"ragged": (3, 7, 5, [0, 3, 6]), "two_per_lane": (2, 70, 8, [69, 37])}
_METRICS = {"l2_slice": dict(a_pose_slice=slice(1, 4)), "l2_ab": dict(a_pose_slice=slice(0, 3), b_pose_slice=slice(2, 5)),
            "l2_all": dict(), "cosine": dict(metric="cosine")}


@pytest.mark.parametrize("k", [1, 3, 200])
@pytest.mark.parametrize("metric", list(_METRICS))
@pytest.mark.parametrize("shape", list(_SHAPES))
def test_selector_alone_both_forms(shape, metric, k):
    """(a) distances() against the float64 restatement, within 3x the error of the restatement's own fp32 evaluation
    (floor 2e-6: the rule of tests/_golden.py fp64_bound); (b) the adjacency row is EXACTLY the top-k, ties to the
    lower index, of the kernel's own distances - without and with a cap; the decision row of the "pre" form is the same
    selection and leaves the entries j >= cur alone."""
    B, N, F, curs = _SHAPES[shape]
    kw = _METRICS[metric]
    nodes, cur = _case(B, N, F, curs, seed=7 * N + k)
    ref = R.KNNSelector(k, kw.get("a_pose_slice"), kw.get("b_pose_slice"), metric=kw.get("metric", "l2"))
    d64 = ref.distances(nodes, cur)
    err32 = float((ref.distances(nodes, cur, dtype=torch.float32).double() - d64).abs().max())
    full = [b for b in range(B) if int(cur[b]) == N - 1]
    for cap in (None, 0.75):
        sel = KNNEdge(k, max_distance=cap, **kw)
        adj, dist = _advanced(sel, nodes, cur)
        bound = max(2e-6, 3.0 * err32)
        err = float((dist.double() - d64).abs().max())
        print(f"{shape} {metric} k={k} cap={cap}: |dist - f64| = {err:.3g}, bound {bound:.3g}, ratio {err / bound:.3g}")
        assert err <= bound
        want = R.topk_rows(dist, cur, k, cap)
        got = adj[torch.arange(B), cur]
        assert torch.equal(got, want)
        assert float(adj.sum()) == float(want.sum())            # nothing outside row cur
        if cap is None:
            assert want.sum(1).tolist() == [float(min(k, int(c))) for c in cur]
        row = _pre(sel, nodes, cur, full)
        for b in range(B):
            n = int(cur[b])
            assert torch.equal(row[b, :n], want[b, :n]) and bool((row[b, n:] == 7.0).all())
    # bidirectional: the row mirrored into the column
    adj, dist = _advanced(KNNEdge(k, bidirectional=True, **kw), nodes, cur)
    want = R.topk_rows(dist, cur, k)
    for b in range(B):
        n = int(cur[b])
        assert torch.equal(adj[b, n], want[b]) and torch.equal(adj[b, :, n], adj[b, n])
        assert float(adj[b].sum()) == 2.0 * float(want[b].sum())


# ---------------------------------------------------------------------------------------------------------
# exact ties
# ---------------------------------------------------------------------------------------------------------
def _grid_case(B, N, F, cols, curs, seed, max_copies=None):
    """Positions on the integer grid 0..3 in `cols` columns from column 0 (squared sums <= 27: exact in fp32, and sqrt
    keeps distinct sums distinct), the other columns random.  max_copies: at most that many rows of a graph share a
    position."""
    g = torch.Generator().manual_seed(seed)
    nodes = torch.rand(B, N, F, generator=g)
    for b in range(B):
        seen = {}
        for j in range(N):
            while True:
                p = tuple(torch.randint(0, 4, (cols,), generator=g).tolist())
                if max_copies is None or seen.get(p, 0) < max_copies:
                    break
            seen[p] = seen.get(p, 0) + 1
            nodes[b, j, :cols] = torch.tensor(p, dtype=torch.float32)
    return nodes, torch.tensor(curs)


@pytest.mark.parametrize("cols", [2, 3])
@pytest.mark.parametrize("k", [1, 3, 200])
def test_grid_ties_match_the_restatement_bit_for_bit(cols, k):
    B, N, F = 3, 70, 5
    nodes, cur = _grid_case(B, N, F, cols, [69, 40, 5], seed=cols * 10 + k)
    for cap in (None, 2.0):                                     # (2.0: a distance many candidates sit at EXACTLY)
        sel, ref = KNNEdge(k, slice(0, cols), max_distance=cap), R.KNNSelector(k, slice(0, cols), max_distance=cap)
        adj, dist = _advanced(sel, nodes, cur)
        d64 = ref.distances(nodes, cur)
        assert torch.equal(dist, d64.float())                   # exact sums, correctly rounded sqrt
        want = ref.select(nodes, cur)
        ties = sum(int(len(set(d64[b, :int(cur[b])].tolist())) < int(cur[b])) for b in range(B))
        assert ties >= 2                                        # the case does hold equal distances
        assert torch.equal(adj[torch.arange(B), cur], want)
        row = _pre(sel, nodes, cur, full=[0])
        for b in range(B):
            n = int(cur[b])
            assert torch.equal(row[b, :n], want[b, :n]) and bool((row[b, n:] == 7.0).all())


def test_cosine_duplicates_go_to_the_lower_index():
    nodes, cur = _case(2, 70, 6, [69, 20], seed=3)
    nodes = nodes + 0.5
    for b, dups in ((0, (2, 11, 40, 66)), (1, (0, 5, 19))):
        nodes[b, list(dups)] = nodes[b, int(cur[b])].clone()      # copies of the current node: equal distances
    for k in (1, 2, 3):
        adj, dist = _advanced(KNNEdge(k, metric="cosine"), nodes, cur)
        for b, dups in ((0, (2, 11, 40, 66)), (1, (0, 5, 19))):
            n = int(cur[b])
            assert len(set(dist[b, list(dups)].tolist())) == 1 and float(dist[b, dups[0]]) <= float(dist[b, :n].min())
            assert torch.nonzero(adj[b, n]).flatten().tolist() == list(dups[:k])
        assert torch.equal(adj[torch.arange(2), cur], R.topk_rows(dist, cur, k))


@pytest.mark.parametrize("metric", ["l2_slice", "cosine"])
def test_nan_row_is_never_selected_and_changes_nothing_else(metric):
    kw = _METRICS[metric]
    nodes, cur = _case(2, 70, 6, [69, 30], seed=5)
    clean = nodes.clone()
    clean[0, 17] = 50.0 if metric != "cosine" else -nodes[0, 69]   # the farthest candidate of graph 0 instead of a NaN
    nodes[0, 17, 2] = float("nan")
    g = torch.Generator().manual_seed(1)
    adj0 = (torch.rand(2, 70, 70, generator=g) < 0.2).float()
    adj0[torch.arange(2), cur] = 0.0
    for k in (1, 5, 68, 200):
        adj, dist = _advanced(KNNEdge(k, **kw), nodes, cur, adj0)
        assert bool(torch.isnan(dist[0, 17])) and int(torch.isnan(dist).sum()) == 1
        assert float(adj[0, 69, 17]) == 0.0
        assert float(adj[0, 69].sum()) == float(min(k, 68)) and float(adj[1, 30].sum()) == float(min(k, 30))
        want = R.topk_rows(dist, cur, k)
        assert torch.equal(adj[torch.arange(2), cur], want)
        # what a clean graph selects among the other 68 candidates
        adj_c, _ = _advanced(KNNEdge(min(k, 68), **kw), clean, cur, adj0)
        assert torch.equal(adj_c, adj)
        keep = torch.ones(2, 70, 70, dtype=torch.bool)
        keep[torch.arange(2), cur] = False
        assert torch.equal(adj[keep], adj0[keep])                # the rest of the adjacency is untouched
        row = _pre(KNNEdge(k, **kw), nodes, cur, full=[0])
        assert torch.equal(row[0, :69], want[0, :69]) and torch.equal(row[1, :30], want[1, :30])


# ---------------------------------------------------------------------------------------------------------
# the sparse twin
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,cols", [(1, 3), (2, 2), (3, 2), (3, 3)])
def test_twin_sparse_spatial_knn_edge(k, cols):
    """Dense KNNEdge(k, slice) stepwise == sparse SpatialKNNEdge(k + 1, slice) with tau = 1 (the sparse selector counts
    the new node itself among its k), given at most k rows of a graph at any one position."""
    from gcm.sparse_edge_selectors.spatial import SpatialKNNEdge
    B, N, F = 3, 24, 5                                          # (4 ** cols * k >= 32 grid slots for the 24 rows)
    nodes, _ = _grid_case(B, N, F, cols, [0] * B, seed=k + cols, max_copies=k)
    for b in range(B):                                          # the precondition
        _, counts = torch.unique(nodes[b, :, :cols], dim=0, return_counts=True)
        assert int(counts.max()) <= k
    if k > 1:                                                   # duplicates do occur
        assert any(int(torch.unique(nodes[b, :, :cols], dim=0).shape[0]) < N for b in range(B))
    dense, sparse = KNNEdge(k, slice(0, cols)), SpatialKNNEdge(slice(0, cols), k + 1)
    nd = nodes.to(DEV)
    for T in ([0, 1, 2], [5, N - 1, 9], [N - 1, 3, N // 2]):
        cur = torch.tensor(T)
        adj, _ = _advanced(dense, nodes, cur)
        coo = sparse(nd, cur.to(DEV), torch.ones(B, dtype=torch.long, device=DEV), B)
        assert torch.equal(coo.to_dense().cpu(), adj)
        assert torch.equal(adj[torch.arange(B), cur], R.KNNSelector(k, slice(0, cols)).select(nodes, cur))


# ---------------------------------------------------------------------------------------------------------
# through DenseGCM
# ---------------------------------------------------------------------------------------------------------
B4, N4, F4, H4, T4, K4 = 4, 16, 8, 8, 21, 3                     # T = N + 5: the wrap-around is crossed


def _gnn_pair(seed=0):
    from gcm import nn as G
    torch.manual_seed(seed)
    ref = od.canonical_gnn(F4, H4)
    g = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(F4, H4), "x, adj -> x"), torch.nn.Tanh(),
                                               (G.DenseGraphConv(H4, H4), "x, adj -> x"), torch.nn.Tanh()])
    g.load_state_dict(ref.state_dict())
    return ref, g.to(DEV)


def _selectors(config, bidirectional=False, spatial=False):
    """(product kwargs of DenseGCM, oracle kwargs of dense_step) for: "alone", "seq" (in a Sequential after
    TemporalBackedge([1])), "aux" (as aux_edge_selectors behind TemporalBackedge([1]))."""
    from gcm import nn as G
    from gcm.edge_selectors.temporal import TemporalBackedge
    if spatial:
        sel = SpatialEdge(1.0, slice(0, 3))
        sel.bidirectional = bidirectional
        ref = od.SpatialEdge(1.0, slice(0, 3), bidirectional=bidirectional)
    else:
        sel = KNNEdge(K4, slice(0, 3), bidirectional=bidirectional)
        ref = R.KNNSelector(K4, slice(0, 3), bidirectional=bidirectional)
    if config == "alone":
        return dict(edge_selectors=sel), dict(edge_selectors=ref)
    if config == "aux":
        return (dict(edge_selectors=TemporalBackedge([1]), aux_edge_selectors=sel),
                dict(edge_selectors=od.TemporalBackedge([1]), aux_edge_selectors=ref))
    step = "nodes, adj, weights, num_nodes, B -> adj, weights"
    seq = G.Sequential("nodes, adj, weights, num_nodes, B", [(TemporalBackedge([1]), step), (sel, step)])
    return dict(edge_selectors=seq), dict(edge_selectors=od.chain(od.TemporalBackedge([1]), ref))


_ORACLE = {}


def _obs():
    """Positions (columns 0..2) on the integer grid 0..3 - equal distances at every step, no ranking that hangs on
    the last bit of a sum - the other columns random."""
    g = torch.Generator().manual_seed(11)
    obs = torch.rand(T4, B4, F4, generator=g)
    obs[:, :, :3] = torch.randint(0, 4, (T4, B4, 3), generator=g).float()
    return obs


def _oracle(config, bidirectional=False):
    """Computed once per configuration and shared: beliefs, the adjacency after every step, parameter gradients."""
    key = (config, bidirectional)
    if key not in _ORACLE:
        ref, _ = _gnn_pair()
        _, okw = _selectors(config, bidirectional)
        obs, hid, outs, adjs = _obs(), None, [], []
        for t in range(T4):
            mx, hid = od.dense_step(obs[t], hid, ref, graph_size=N4, **okw)
            outs.append(mx)
            adjs.append(hid[1].clone())
        out = torch.stack(outs)
        (out * torch.linspace(0.5, 1.5, out.numel()).view_as(out)).sum().backward()
        _ORACLE[key] = (out.detach(), adjs, hid, {k_: p.grad.clone() for k_, p in ref.named_parameters()})
    return _ORACLE[key]


def _drive(config, driver, bidirectional=False, spatial=False):
    from gcm.gcm import DenseGCM
    _, g = _gnn_pair()
    pkw, _ = _selectors(config, bidirectional, spatial)
    mem = DenseGCM(g, graph_size=N4, fused=driver != "layered", donate_state=driver == "donated", **pkw)
    obs = _obs().to(DEV)
    adjs = []
    if driver == "rollout":
        out, hid = mem.rollout(obs)
    else:
        hid, outs = None, []
        for t in range(T4):
            mx, hid = mem(obs[t], hid)
            outs.append(mx)
            adjs.append(hid[1].detach().cpu())
        out = torch.stack(outs)
    (out * torch.linspace(0.5, 1.5, out.numel(), device=DEV).view_as(out)).sum().backward()
    mem.check_flags()
    grads = {k_: p.grad.cpu() for k_, p in g.named_parameters()}
    return mem, out.detach().cpu(), adjs, tuple(h.detach().cpu() for h in hid), grads


def _check_against_oracle(got, want):
    _, out, adjs, hid, grads = got
    w_out, w_adjs, w_hid, w_grads = want
    for t, a in enumerate(adjs):
        assert torch.equal(a, w_adjs[t]), t                     # the adjacency after every step: exact
    assert torch.equal(hid[1], w_hid[1]) and torch.equal(hid[0], w_hid[0]) and torch.equal(hid[3], w_hid[3])
    # (the tolerances of tests/test_dense_gpu.py for its SpatialEdge fixtures: beliefs 1e-5 / 1e-6, gradients 1e-5 of
    #  their scale)
    torch.testing.assert_close(out, w_out, rtol=1e-5, atol=1e-6)
    for k_, wg in w_grads.items():
        torch.testing.assert_close(grads[k_], wg, rtol=1e-5, atol=1e-5 * float(wg.abs().max()), msg=k_)


@pytest.mark.parametrize("driver", ["functional", "donated", "rollout", "layered"])
@pytest.mark.parametrize("config", ["alone", "seq", "aux"])
def test_dense_gcm_matches_the_oracle(config, driver):
    want = _oracle(config)
    assert all(w.sum(dim=2).max() <= K4 + (config != "alone") for w in want[1])     # the in-degree is capped
    assert float(want[1][-1].sum()) > 0
    got = _drive(config, driver)
    mem = got[0]
    assert (mem._structure() is not None) == (driver != "layered" and config != "aux")
    _check_against_oracle(got, want)


@pytest.mark.parametrize("config", ["alone", "seq"])
def test_fused_and_layered_agree(config):
    """The same module on the fused kernels and layer by layer, at the fused-vs-layered tolerances of
    tests/test_dense_gpu.py (state bit exact)."""
    _, w_out, w_adjs, w_hid, w_grads = _drive(config, "layered")
    for driver in ("functional", "donated", "rollout"):
        _, out, adjs, hid, grads = _drive(config, driver)
        torch.testing.assert_close(out, w_out, rtol=1e-5, atol=1e-5 * max(1.0, float(w_out.abs().max())))
        for a, b in zip(hid, w_hid):
            assert torch.equal(a, b)
        for t, a in enumerate(adjs):
            assert torch.equal(a, w_adjs[t])
        for k_, wg in w_grads.items():
            torch.testing.assert_close(grads[k_], wg, rtol=1e-5, atol=1e-5 * (float(wg.abs().max()) + 1e-12), msg=k_)


@pytest.mark.parametrize("config", ["alone", "seq"])
def test_path_is_spatial_edges(config):
    """Non-bidirectional: the live-row / cached-step kernels, exactly where SpatialEdge with the same arguments runs
    them; bidirectional: the path SpatialEdge(bidirectional) takes (no live-row steps), same results as the oracle."""
    for driver in ("functional", "donated"):
        knn, spa = _drive(config, driver)[0], _drive(config, driver, spatial=True)[0]
        assert knn.rows_steps() == spa.rows_steps() > 0
        assert knn.rows_cached_steps_taken() == spa.rows_cached_steps_taken()
        assert knn.rows_cached_launches_per_step(B4) == spa.rows_cached_launches_per_step(B4)
    got = _drive(config, "donated", bidirectional=True)
    spa = _drive(config, "donated", bidirectional=True, spatial=True)[0]
    assert got[0]._structure() is not None and spa._structure() is not None
    assert got[0].rows_steps() == spa.rows_steps()
    assert got[0].rows_cached_launches_per_step(B4) == spa.rows_cached_launches_per_step(B4)
    _check_against_oracle(got, _oracle(config, bidirectional=True))
    _check_against_oracle(_drive(config, "rollout", bidirectional=True), _oracle(config, bidirectional=True))


# ---------------------------------------------------------------------------------------------------------
# the threshold selectors are what they were
# ---------------------------------------------------------------------------------------------------------
def test_threshold_selectors_unchanged():
    """SpatialEdge / CosineEdge adjacency and distances(), bit for bit what commit f03a964 (the parent of the commit
    that added KNNEdge) computed on an MI355X: tests/golden/g18_threshold_parent.npz was recorded by running that
    commit's library on the case stored in it."""
    z = np.load(os.path.join(GOLDEN, "g18_threshold_parent.npz"))
    nodes, cur = torch.from_numpy(z["nodes"]), torch.from_numpy(z["cur"])
    for name, sel in (("spatial", SpatialEdge(0.45, slice(0, 3))), ("spatial_ab", SpatialEdge(0.5, slice(0, 3), slice(1, 4))),
                      ("cosine", CosineEdge(0.3))):
        adj, dist = _advanced(sel, nodes, cur)
        assert float(z[name + "_adj"].sum()) > 0
        assert np.array_equal(adj.numpy(), z[name + "_adj"]), name
        assert np.array_equal(dist.numpy().view(np.uint32), z[name + "_dist"].view(np.uint32)), name
