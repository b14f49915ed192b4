"""SparseGCM's sliding window on the GPU (csrc/sparse_window.hip): the drop kernels against the
plain-torch restatement (exactly: the primitive only moves data), overflow="wrap" against the oracle on every host
path and against DenseGCM, reset_hidden, and every shipped sparse selector across a wrap.  Needs an MI355X."""
import copy

import pytest
import torch

from _sparse_window_restate import drop_oldest_ref, random_causal_state, reset_ref, state_equal, wrap_k
from oracle import sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev_gnn(ref, F, H, act=torch.nn.Tanh):
    from gcm import nn as G
    mods, cin = [], F
    for _ in range(2):
        mods.append((G.GraphConv(cin, H), "x, edges, weights -> x"))
        if act is not None:
            mods.append(act())
        cin = H
    g = G.Sequential("x, edges, weights", mods)
    g.load_state_dict(ref.state_dict())
    return g.to(DEV)


def _to(hidden, dev):
    return hidden[0].to(dev), hidden[1].to(dev), hidden[2].to(dev)


def _assert_state(got, want, what=""):
    """Device state == CPU state, exactly."""
    ga, wa = got[1].coalesce(), want[1].coalesce()
    assert torch.equal(got[0].cpu(), want[0]), what
    assert torch.equal(ga.indices().cpu(), wa.indices()), what
    assert torch.equal(ga.values().detach().cpu(), wa.values().detach()), what
    assert torch.equal(got[2].cpu(), want[2]), what


# ---------------------------------------------------------------------------
# the kernels against the restatement
# ---------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 0.5), (3, 6, 4, 0.5), (5, 33, 3, 0.5), (4, 64, 8, 0.5),
          (2, 200, 32, 0.3)]      # ~6 000 entries per graph: a graph spans several 1024-entry chunks
PATTERNS = ["zero", "all", "one", "random", "clamped", "empty_graphs", "graph_without_edges", "no_edges"]


def _case(B, N, F, density, pattern):
    seed = B * 1000 + N
    gen = torch.Generator().manual_seed(seed)
    T = torch.full((B,), N) if N == 200 else torch.randint(0, N + 1, (B,), generator=gen)
    T[-1] = N                                   # (one full graph in every case)
    if pattern == "empty_graphs":
        T[0] = 0
    nodes, adj, T = random_causal_state(B, N, F, 0.0 if pattern == "no_edges" else density, T=T, seed=seed)
    if pattern == "graph_without_edges":
        idx, val = adj.indices(), adj.values()
        keep = idx[0] != B - 1
        adj = torch.sparse_coo_tensor(idx[:, keep], val[keep], size=adj.shape).coalesce()
    if pattern == "zero":
        k = torch.zeros(B, dtype=torch.long)
    elif pattern == "all":
        k = T.clone()
    elif pattern == "one":
        k = torch.ones(B, dtype=torch.long)
    else:
        k = (torch.rand(B, generator=gen) * (T + 1)).long().clamp(max=T)
        if pattern == "clamped":
            k[0] = T[0] + 3
            k[-1] = -2
            if B > 2:
                k[1] = N + 100
    return (nodes, adj, T), k


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("B,N,F,density", SHAPES)
def test_drop_kernels_match_restatement(B, N, F, density, pattern):
    from gcm import _ops
    from gcm.sparse_gcm import SparseGCM
    hidden, k = _case(B, N, F, density, pattern)
    hd, kd = _to(hidden, DEV), k.to(DEV)
    before = (hd[0].clone(), hd[1].indices().clone(), hd[1].values().clone(), hd[2].clone(), kd.clone())
    want = drop_oldest_ref(hd, kd)              # (the restatement on the same device tensors)
    n2, idx, val, T2, bptr = _ops.sparse_drop_oldest(hd[0], hd[1].indices(), hd[1].values(), hd[2], kd)
    assert torch.equal(n2, want[0])
    assert torch.equal(idx, want[1]._indices()) and torch.equal(val, want[1]._values())
    assert torch.equal(T2, want[2])
    counts = torch.bincount(want[1]._indices()[0], minlength=B)
    assert torch.equal(bptr, torch.cat([torch.zeros(1, dtype=torch.long, device=DEV), counts.cumsum(0)]))
    if pattern == "zero":
        assert torch.equal(n2, hd[0]) and torch.equal(idx, hd[1].indices()) and torch.equal(val, hd[1].values())
    if pattern == "all":
        assert idx.shape[1] == 0 and not n2.any() and not T2.any()
    # the public method: same result as a coalesced sparse tensor, inputs untouched
    got = SparseGCM(torch.nn.Identity(), graph_size=N).drop_oldest(hd, kd)
    assert got[1].is_coalesced() and tuple(got[1].shape) == (B, N, N)
    assert state_equal(got, want)
    assert torch.equal(got[1].gcm_bptr, bptr)
    for a, b in zip(before, (hd[0], hd[1].indices(), hd[1].values(), hd[2], kd)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,N,F,density", [(3, 6, 4, 0.5), (5, 33, 3, 0.5), (2, 200, 32, 0.3)])
def test_drop_gradients_match_restatement(B, N, F, density):
    """nodes and values both need a gradient; against autograd through the restatement, exactly."""
    from gcm.sparse_gcm import SparseGCM
    hidden, k = _case(B, N, F, density, "random")
    k[-1] = 1
    nodes, adj, T = _to(hidden, DEV)
    kd = k.to(DEV)
    gen = torch.Generator().manual_seed(5)
    grads = []
    w_n = None
    for fn in (SparseGCM(torch.nn.Identity(), graph_size=N).drop_oldest, drop_oldest_ref):
        n = nodes.clone().requires_grad_(True)
        v = adj.values().clone().requires_grad_(True)
        a = torch.sparse_coo_tensor(adj.indices(), v, size=adj.shape, is_coalesced=True)
        n2, a2, _ = fn((n, a, T), kd)
        v2 = a2.coalesce().values()              # (differentiable, unlike _values())
        if w_n is None:
            w_n = torch.rand(n2.shape, generator=gen).to(DEV)
            w_v = torch.rand(v2.shape, generator=gen).to(DEV)
        ((n2 * w_n).sum() + (v2 * w_v).sum()).backward()
        grads.append((n.grad, v.grad))
    assert grads[0][0] is not None and grads[0][1] is not None
    assert torch.equal(grads[0][0], grads[1][0])
    assert torch.equal(grads[0][1], grads[1][1])


# ---------------------------------------------------------------------------
# overflow="wrap" against the oracle
# ---------------------------------------------------------------------------
def _taus(step, B):
    """Ragged starts (graph b receives nothing before step b) and a pause of graph 1 now and then."""
    t = torch.tensor([1 if step >= b else 0 for b in range(B)])
    if step % 5 == 3:
        t[1] = 0
    return t


def _oracle_run(ref, xs, taus_list, N, hops, hidden=None, max_hops=None, dtype=torch.float32):
    """drop (restatement) + oracle step per call; -> (outs, states after every call, obs grads, parameter grads)."""
    r = copy.deepcopy(ref).to(dtype)
    xs = [x.clone().to(dtype).requires_grad_(True) for x in xs]
    sel = osp.TemporalEdge(hops)
    if hidden is None:
        hidden = osp.initial_hidden(xs[0], N)
        hidden = (hidden[0].to(dtype), hidden[1], hidden[2])
    outs, states = [], []
    for x, taus in zip(xs, taus_list):
        hidden = drop_oldest_ref(hidden, wrap_k(hidden[2], taus, N))
        o, hidden = osp.sparse_step(x, taus, hidden, r, graph_size=N, edge_selectors=sel, max_hops=max_hops)
        outs.append(o)
        states.append(hidden)
    (sum(o.sum() for o in outs) / sum(o.numel() for o in outs)).backward()
    return ([o.detach() for o in outs], states, [x.grad for x in xs], {k: p.grad for k, p in r.named_parameters()})


def _device_run(mem, g, xs, taus_list, hidden=None, obs_grad=True):
    g.zero_grad(set_to_none=True)
    xs = [x.to(DEV).requires_grad_(obs_grad) for x in xs]
    outs, states = [], []
    for x, taus in zip(xs, taus_list):
        o, hidden = mem(x, taus.to(DEV), hidden)
        outs.append(o)
        states.append(hidden)
    (sum(o.sum() for o in outs) / sum(o.numel() for o in outs)).backward()
    return ([o.detach().cpu() for o in outs], states, [x.grad for x in xs],
            {k: p.grad.cpu() for k, p in g.named_parameters()})


def _compare(got, want):
    """The bounds of test_sparse_rollout_matches_reference: state exact, beliefs rtol = atol = 1e-5, gradients
    rtol 1e-5 and atol 1e-5 of their largest entry."""
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        _assert_state(a, b, f"state after call {i}")
    for a, b in zip(got[0], want[0]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    if got[2][0] is not None:
        gs = max(float(b.abs().max()) for b in want[2])
        for a, b in zip(got[2], want[2]):
            torch.testing.assert_close(a.cpu(), b, rtol=1e-5, atol=1e-5 * gs)
    for k, b in want[3].items():
        torch.testing.assert_close(got[3][k], b, rtol=1e-5, atol=1e-5 * float(b.abs().max()) + 1e-7, msg=k)


def _memory(g, hops, N, path, **kw):
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    mem = SparseGCM(g, edge_selectors=TemporalEdge(hops), graph_size=N, overflow="wrap", **kw)
    mem.fast_host = path != "layered"
    mem.stepwise_cache = path == "cpp_cached"
    return mem


PATHS = ["cpp_cached", "cpp_uncached", "layered"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("hops", [[1], [1, 2, 4]])
@pytest.mark.parametrize("N", [6, 8])
def test_wrap_stepwise_matches_oracle(N, hops, path):
    B, F, H = 3, 3, 5
    steps = int(2.5 * N)
    torch.manual_seed(N * 10 + len(hops))
    ref = osp.canonical_gnn(F, H)
    xs = [torch.rand(B, 1, F) for _ in range(steps)]
    taus_list = [_taus(s, B) for s in range(steps)]
    want = _oracle_run(ref, xs, taus_list, N, hops)
    g = _dev_gnn(ref, F, H)
    got = _device_run(_memory(g, hops, N, path), g, xs, taus_list)
    assert int(got[1][-1][2].max()) == N
    _compare(got, want)


def test_wrap_with_max_hops():
    B, F, H, N, hops = 3, 3, 5, 6, [1, 2, 4]
    torch.manual_seed(3)
    ref = osp.canonical_gnn(F, H)
    # (two nodes per graph first: the k-hop mask kernel takes no empty edge list)
    xs = [torch.rand(B, 2, F)] + [torch.rand(B, 1, F) for _ in range(14)]
    taus_list = [torch.full((B,), 2)] + [_taus(s, B) for s in range(3, 17)]
    want = _oracle_run(ref, xs, taus_list, N, hops, max_hops=2)
    g = _dev_gnn(ref, F, H)
    _compare(_device_run(_memory(g, hops, N, "layered", max_hops=2), g, xs, taus_list), want)


def test_wrap_ends_the_cached_chain():
    """F = H = 32: the calls before the first wrap run on the stepwise chain's caches, the wrap ends the chain (its
    caches depend on the dropped nodes) and the calls behind it run the general path.  State exact; beliefs and
    parameter gradients inside 3x the fp32 oracle's own distance from the float64 oracle, the bound of
    test_sparse_stepwise_cached_chain_vs_oracle."""
    B, F, H, N, hops, steps = 3, 32, 32, 8, [1, 2], 20
    torch.manual_seed(9)
    ref = osp.canonical_gnn(F, H)
    xs = [torch.rand(B, 1, F) for _ in range(steps)]
    taus_list = [torch.ones(B, dtype=torch.long) for _ in range(steps)]
    w32 = _oracle_run(ref, xs, taus_list, N, hops)
    w64 = _oracle_run(ref, xs, taus_list, N, hops, dtype=torch.float64)
    g = _dev_gnn(ref, F, H)
    mem = _memory(g, hops, N, "cpp_cached")
    g.zero_grad(set_to_none=True)
    hidden, outs = None, []
    for s in range(steps):
        o, hidden = mem(xs[s].to(DEV), taus_list[s].to(DEV), hidden)
        outs.append(o)
        if s == N - 1:
            assert mem._chain is not None and mem._chain.steps() == N and mem._chain.live()
        _assert_state(hidden, w32[1][s], f"state after call {s}")
    assert mem._chain is None or not mem._chain.live()
    (sum(o.sum() for o in outs) / sum(o.numel() for o in outs)).backward()
    got, o32, o64 = torch.stack(outs).detach().cpu().double(), torch.stack(w32[0]).double(), torch.stack(w64[0])
    assert float((got - o64).abs().max()) <= max(2e-6, 3.0 * float((o32 - o64).abs().max()))
    for k, p in g.named_parameters():
        want = w64[3][k]
        atol = max(3.0 * float((w32[3][k].double() - want).abs().max()), 5e-7 * float(want.abs().max()))
        assert float((p.grad.cpu().double() - want).abs().max()) <= atol, k


@pytest.mark.parametrize("path", ["cpp_uncached", "layered"])
def test_wrap_multi_node_calls_are_drop_then_call(path):
    """taus up to 3 with T + tau > N: drop first, then the call as it is (DESIGN 3.25's multi-node caveat)."""
    B, F, H, N, hops = 3, 3, 5, 6, [1, 2]
    torch.manual_seed(4)
    ref = osp.canonical_gnn(F, H)
    gen = torch.Generator().manual_seed(4)
    taus_list = [torch.randint(0, 4, (B,), generator=gen) for _ in range(8)]
    for t in taus_list:
        t[0] = max(int(t[0]), 1)            # (the oracle needs a new node in every call)
    xs = []
    for t in taus_list:
        x = torch.rand(B, 3, F, generator=gen)
        xs.append(x * (torch.arange(3)[None, :] < t[:, None])[:, :, None])
    want = _oracle_run(ref, xs, taus_list, N, hops)
    g = _dev_gnn(ref, F, H)
    got = _device_run(_memory(g, hops, N, path), g, xs, taus_list)
    assert int(sum(taus_list)[0]) > N
    _compare(got, want)


@pytest.mark.parametrize("path", ["cpp_uncached", "layered"])
def test_wrap_still_raises_when_one_call_exceeds_the_graph(path):
    ref = osp.canonical_gnn(2, 2)
    mem = _memory(_dev_gnn(ref, 2, 2), [1], 4, path)
    with pytest.raises(Exception, match="Overflow"):
        mem(torch.zeros(2, 5, 2, device=DEV), torch.tensor([5, 1], device=DEV), None)
    out, hidden = mem(torch.rand(2, 3, 2, device=DEV), torch.tensor([3, 1], device=DEV), None)
    with pytest.raises(Exception, match="Overflow"):
        mem(torch.zeros(2, 5, 2, device=DEV), torch.tensor([5, 1], device=DEV), hidden)


def test_wrap_matches_dense_gcm():
    """DenseGCM + TemporalBackedge([1, 2]) on the GPU, 2 N steps past N = 8: nodes and edge sets exactly, beliefs at
    the bound of test_sparse_rollout_matches_reference."""
    from gcm.gcm import DenseGCM
    from gcm import nn as G
    from gcm.edge_selectors.temporal import TemporalBackedge
    F, B, N = 3, 3, 8
    torch.manual_seed(0)
    dense_g = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(F, F), "x, adj -> x"), torch.nn.Tanh(),
                                                      (G.DenseGraphConv(F, F), "x, adj -> x"), torch.nn.Tanh()])
    sparse_g = G.Sequential("x, edges, weights", [(G.GraphConv(F, F), "x, edges, weights -> x"), torch.nn.Tanh(),
                                                   (G.GraphConv(F, F), "x, edges, weights -> x"), torch.nn.Tanh()])
    sparse_g.load_state_dict(dense_g.state_dict())
    dense = DenseGCM(dense_g.to(DEV), edge_selectors=TemporalBackedge([1, 2]), graph_size=N)
    sparse = _memory(sparse_g.to(DEV), [1, 2], N, "cpp_uncached")
    obs = torch.rand(B, 3 * N, F).to(DEV)
    one = torch.ones(B, dtype=torch.long, device=DEV)
    dh = sh = None
    for i in range(3 * N):
        do, dh = dense(obs[:, i], dh)
        so, sh = sparse(obs[:, i:i + 1], one, sh)
        assert torch.equal(dh[0], sh[0]), i
        assert torch.equal(dh[1].nonzero().T, sh[1].coalesce().indices()), i
        assert torch.equal(dh[3], sh[2]), i
        torch.testing.assert_close(so[:, 0], do, rtol=1e-5, atol=1e-5)
    dense.check_flags()


# ---------------------------------------------------------------------------
# reset_hidden
# ---------------------------------------------------------------------------
def test_reset_hidden():
    B, F, H, N, hops = 4, 3, 5, 6, [1, 2]
    torch.manual_seed(6)
    ref = osp.canonical_gnn(F, H)
    g = _dev_gnn(ref, F, H)
    mem = _memory(g, hops, N, "cpp_uncached")
    sel = osp.TemporalEdge(hops)
    xs = [torch.rand(B, 1, F) for _ in range(9)]
    one = torch.ones(B, dtype=torch.long)
    hd = hc = None
    for s in range(4):
        _, hd = mem(xs[s].to(DEV), one.to(DEV), hd)
        _, hc = osp.sparse_step(xs[s], one, hc, ref, graph_size=N, edge_selectors=sel)
    mask = torch.tensor([True, False, True, False])
    r_dev = mem.reset_hidden(hd, mask.to(DEV))
    r_cpu = mem.reset_hidden(hd, mask)                      # a mask on the CPU is accepted
    assert state_equal(r_dev, r_cpu)
    _assert_state(r_dev, reset_ref(hc, mask))
    idx = r_dev[1].indices()
    for b in range(B):
        if mask[b]:
            assert int(r_dev[2][b]) == 0 and not r_dev[0][b].any() and not bool((idx[0] == b).any())
        else:                                               # bitwise untouched
            old = hd[1].coalesce().indices()
            assert torch.equal(r_dev[0][b], hd[0][b]) and int(r_dev[2][b]) == int(hd[2][b])
            assert torch.equal(idx[1:, idx[0] == b], old[1:, old[0] == b])
    # a run that continues behind the reset (and wraps later) matches the oracle
    hd, hc = r_dev, reset_ref(hc, mask)
    for s in range(4, 9):
        od_, hd = mem(xs[s].to(DEV), one.to(DEV), hd)
        hc = drop_oldest_ref(hc, wrap_k(hc[2], one, N))
        oc, hc = osp.sparse_step(xs[s], one, hc, ref, graph_size=N, edge_selectors=sel)
        _assert_state(hd, hc, f"step {s}")
        torch.testing.assert_close(od_.detach().cpu(), oc.detach(), rtol=1e-5, atol=1e-5)
    # the gradient into a cleared graph's incoming nodes is zero, the others' the identity
    nodes = hd[0].clone().requires_grad_(True)
    w = torch.rand(nodes.shape, device=DEV) + 0.5
    n2, _, _ = mem.reset_hidden((nodes, hd[1], hd[2]), mask)
    (n2 * w).sum().backward()
    live = (torch.arange(N, device=DEV)[None, :] < hd[2][:, None])[:, :, None]
    assert not nodes.grad[mask.to(DEV)].any()
    assert torch.equal(nodes.grad[~mask.to(DEV)], (w * live)[~mask.to(DEV)])


# ---------------------------------------------------------------------------
# the other selectors
# ---------------------------------------------------------------------------
def test_learned_edge_values_carry_gradients_across_a_drop():
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.learned import LearnedEdge
    torch.manual_seed(2)
    B, N, F = 3, 16, 8
    ref = osp.canonical_gnn(F, F)
    g = _dev_gnn(ref, F, F)
    sel = LearnedEdge(F, num_edge_samples=3, window=8, store_grads=False).to(DEV)
    mem = SparseGCM(g, edge_selectors=sel, graph_size=N)
    x1, x2 = torch.rand(B, 6, F, device=DEV), torch.rand(B, 4, F, device=DEV)
    t1 = torch.tensor([6, 5, 6], device=DEV)
    t2 = torch.tensor([4, 4, 2], device=DEV)
    k = torch.tensor([2, 0, 3], device=DEV)
    draws, replay = [], []

    def record(logits):
        gz = -torch.empty(logits.numel(), device=DEV).exponential_().log()
        draws.append(gz)
        return gz

    results = []
    for drop, noise in ((mem.drop_oldest, record), (drop_oldest_ref, lambda logits: replay.pop(0))):
        sel.noise_fn = noise
        sel.zero_grad(set_to_none=True)
        g.zero_grad(set_to_none=True)
        o1, hidden = mem(x1, t1, None)
        assert hidden[1].values().requires_grad
        o2, hidden2 = mem(x2, t2, drop(hidden, k))
        (o1.mean() + o2.mean()).backward()
        results.append(({n: p.grad.clone() for n, p in sel.edge_network.named_parameters()},
                        hidden2, o2.detach()))
        replay.extend(draws)
    (got, h_got, o_got), (want, h_want, o_want) = results
    assert state_equal((h_got[0], h_got[1].detach(), h_got[2]), (h_want[0], h_want[1].detach(), h_want[2]))
    torch.testing.assert_close(o_got, o_want, rtol=1e-6, atol=1e-6)
    assert any(float(w.abs().max()) > 0 for w in want.values())
    for n, w in want.items():
        torch.testing.assert_close(got[n], w, rtol=1e-5, atol=1e-5 * float(w.abs().max()) + 1e-7, msg=n)


def test_spatial_radius_edge_wraps():
    """A wrap past N = 8 == the same module in "raise" mode with the restatement's drop between the calls."""
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.spatial import SpatialRadiusEdge
    torch.manual_seed(8)
    B, N, F, H = 3, 8, 4, 5
    g = _dev_gnn(osp.canonical_gnn(F, H), F, H)
    wrap = SparseGCM(g, edge_selectors=SpatialRadiusEdge(slice(0, 2), 0.5), graph_size=N, overflow="wrap")
    plain = SparseGCM(g, edge_selectors=SpatialRadiusEdge(slice(0, 2), 0.5), graph_size=N)
    one = torch.ones(B, dtype=torch.long, device=DEV)
    hw = hp = None
    edges = 0
    for s in range(14):
        x = torch.rand(B, 1, F, device=DEV)
        ow, hw = wrap(x, one, hw)
        if hp is not None:
            hp = drop_oldest_ref(hp, wrap_k(hp[2], one, N))
        op, hp = plain(x, one, hp)
        assert state_equal(hw, hp), s
        torch.testing.assert_close(ow, op, rtol=1e-6, atol=1e-6)
        edges = max(edges, hw[1]._nnz())
    assert edges > 0 and int(hw[2].max()) == N


def test_first_wrap_warns_once(capsys):
    from gcm.sparse_gcm import SparseGCM
    ref = osp.canonical_gnn(3, 5)
    mem = _memory(_dev_gnn(ref, 3, 5), [1], 4, "layered")
    one = torch.ones(2, dtype=torch.long, device=DEV)
    saved, SparseGCM.did_warn = SparseGCM.did_warn, False
    try:
        hidden = None
        for _ in range(7):
            _, hidden = mem(torch.rand(2, 1, 3, device=DEV), one, hidden)
        assert SparseGCM.did_warn
    finally:
        SparseGCM.did_warn = saved
    assert capsys.readouterr().out.count("Overflow detected, wrapping around. Will not warn again") == 1
