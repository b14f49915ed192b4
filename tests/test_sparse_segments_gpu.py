"""Episode resets inside one SparseGCM call on the GPU (csrc/sparse_segments.hip): the segment kernels
against the plain-torch restatement (exactly: they only move data), their gradients, rollout(x, reset=mask) end to
end against the oracle stepping one node at a time with reset_ref in between, the selectors and layers without an
oracle twin against the same module stepping with reset_hidden, overflow per episode, and the stepwise chain.
Needs an MI355X."""
import copy

import pytest
import torch

from _sparse_segments_restate import (MASKS, SEEDS, SHAPES, collect_ref, expand_ref, mask_case, plan_ref, random_case,
                                      stepwise_ref, stored_state)
from _sparse_window_restate import random_causal_state, state_equal
from oracle import dense as od, sparse as osp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _to(hidden, dev=DEV):
    return hidden[0].to(dev), hidden[1].to(dev), hidden[2].to(dev)


def _assert_state(got, want, what=""):
    """Device state == CPU state, exactly."""
    ga, wa = got[1].detach().coalesce(), want[1].detach().coalesce()
    assert torch.equal(got[0].detach().cpu(), want[0].detach()), what
    assert torch.equal(ga.indices().cpu(), wa.indices()), what
    assert torch.equal(ga.values().cpu(), wa.values()), what
    assert torch.equal(got[2].cpu(), want[2]), what


# ---------------------------------------------------------------------------
# the kernels against the restatement
# ---------------------------------------------------------------------------
STATES = ["random", "empty_graphs", "no_edges", "clamped"]


def _kernel_case(B, N, F, t, density, pattern, kind):
    seed = B * 1000 + N
    nodes, adj, T = stored_state(B, N, F, density, seed, "random" if kind == "clamped" else kind)
    taus, mask = mask_case(B, t, pattern)
    if kind == "clamped":               # values no call produces: the device clamps taus into [0, t], T passes through
        taus, T = taus.clone(), T.clone()
        taus[-1] = t + 5
        T[-1] = -2
        if B > 1:
            taus[0] = -3
            T[0] = N + 7
    x = torch.rand(B, t, F, generator=torch.Generator().manual_seed(seed + 1))      # (padding NOT zero)
    return x, taus, (nodes, adj, T), mask


def _check_kernels(B, N, F, t, density, pattern, kind):
    from gcm import _hip, _ops
    x, taus, hidden, mask = _kernel_case(B, N, F, t, density, pattern, kind)
    xd, td, hd, md = x.to(DEV), taus.to(DEV), _to(hidden), mask.to(DEV)
    idx, val = hd[1].indices(), hd[1].values()
    before = [v.clone() for v in (xd, td, hd[0], idx, val, hd[2], md)]
    want_x, want_taus, want_h, (segs, vbase) = expand_ref(xd, td, hd, md)       # (on the same device tensors)

    plan = _ops.SegmentPlan(md.view(torch.uint8), td, hd[2], idx)
    Bp = len(segs)
    assert (plan.Bp, plan.tp) == (Bp, want_x.shape[1])
    assert plan.n_resets == Bp - B and plan.E_keep == want_h[1]._nnz()
    assert plan.vbase.tolist() == vbase
    for row, col in ((_hip.SPARSE_SEG_OWNER, 0), (_hip.SPARSE_SEG_START, 1), (_hip.SPARSE_SEG_LEN, 2),
                     (_hip.SPARSE_SEG_EMPTY, 3)):
        assert plan.row(row).tolist() == [s[col] for s in segs], row
    assert torch.equal(plan.row(_hip.SPARSE_SEG_LEN), want_taus) and torch.equal(plan.row(_hip.SPARSE_SEG_T), want_h[2])
    assert plan.row(_hip.SPARSE_SEG_FINAL).tolist() == [b if v == vbase[b + 1] - 1 else -1
                                                        for v, (b, _, _, _) in enumerate(segs)]
    assert torch.equal(_ops.seg_rows(xd, plan, True), want_x)
    assert torch.equal(_ops.seg_nodes(hd[0], plan, False, True), want_h[0])
    idx_s, val_s = _ops.seg_expand_edges(idx, val, plan)
    assert torch.equal(idx_s, want_h[1]._indices()) and torch.equal(val_s, want_h[1]._values())

    # collection, from a made-up result of the call over the virtual graphs
    H = F + F % 2                      # (1 -> 2, 3 -> 4: the scalar and the 16-byte row kernels, in both directions)
    out_s = torch.rand(Bp, plan.tp, H, generator=torch.Generator().manual_seed(7)).to(DEV)
    after = _to(random_causal_state(Bp, N, F, density, seed=B + N))
    want_out, want_f = collect_ref(out_s, after, (segs, vbase), B, t)
    a_idx, a_val = after[1].indices(), after[1].values()
    held = [v.clone() for v in (out_s, after[0], a_idx, a_val, after[2])]
    assert torch.equal(_ops.seg_rows(out_s, plan, False), want_out)
    assert torch.equal(_ops.seg_nodes(after[0], plan, True, False), want_f[0])
    idx_f, val_f = _ops.seg_collect_edges(a_idx, a_val, plan)
    assert torch.equal(idx_f, want_f[1]._indices()) and torch.equal(val_f, want_f[1]._values())
    assert torch.equal(_ops.seg_final_T(after[2], plan), want_f[2])
    for a, b in zip(before + held, [xd, td, hd[0], idx, val, hd[2], md, out_s, after[0], a_idx, a_val, after[2]]):
        assert torch.equal(a, b)
    if pattern in ("none", "padding_only"):
        assert plan.n_resets == 0


@pytest.mark.parametrize("pattern", MASKS)
@pytest.mark.parametrize("B,N,F,t,density", SHAPES)
def test_segment_kernels_match_restatement(B, N, F, t, density, pattern):
    _check_kernels(B, N, F, t, density, pattern, "random")


@pytest.mark.parametrize("kind", STATES[1:])
@pytest.mark.parametrize("pattern", ["all", "random", "last_valid"])
@pytest.mark.parametrize("B,N,F,t,density", SHAPES[:4])
def test_segment_kernels_on_edge_states(B, N, F, t, density, pattern, kind):
    _check_kernels(B, N, F, t, density, pattern, kind)


def test_large_case_spans_several_chunks():
    """(2, 200, 32, 40): the stored list of one graph is longer than two 1024-entry chunks."""
    B, N, F, t, density = SHAPES[-1]
    _, adj, _ = stored_state(B, N, F, density, B * 1000 + N)
    assert int(torch.bincount(adj.indices()[0]).max()) >= 2 * 1024


@pytest.mark.parametrize("B,N,F,t,density", [SHAPES[1], SHAPES[2], SHAPES[4]])
def test_segment_gradients_match_restatement(B, N, F, t, density):
    """x, the node matrix and the edge values all need a gradient: expansion and collection against autograd
    through the restatement, exactly."""
    from gcm import _ops
    x, taus, hidden, mask = _kernel_case(B, N, F, t, density, "random", "random")
    xd, td, hd, md = x.to(DEV), taus.to(DEV), _to(hidden), mask.to(DEV)
    segs, vbase = plan_ref(taus, mask)
    Bp = len(segs)
    after = _to(random_causal_state(Bp, N, F, density, seed=3))
    plan = _ops.SegmentPlan(md.view(torch.uint8), td, hd[2], hd[1].indices())
    gen = torch.Generator().manual_seed(5)
    weights = None
    grads = []
    out_s = torch.rand(Bp, plan.tp, F, generator=gen).to(DEV)
    for kernels in (True, False):
        leaves = [v.clone().requires_grad_(True)
                  for v in (xd, hd[0], hd[1].values(), out_s, after[0], after[1].values())]
        xi, ni, vi, oi, n2, v2 = leaves
        if kernels:
            xs, ns = _ops.seg_rows(xi, plan, True), _ops.seg_nodes(ni, plan, False, True)
            _, vs = _ops.seg_expand_edges(hd[1].indices(), vi, plan)
            o = _ops.seg_rows(oi, plan, False)
            nf = _ops.seg_nodes(n2, plan, True, False)
            _, vf = _ops.seg_collect_edges(after[1].indices(), v2, plan)
        else:
            a = torch.sparse_coo_tensor(hd[1].indices(), vi, size=hd[1].shape, is_coalesced=True)
            xs, _, (ns, adj_s, _), _ = expand_ref(xi, td, (ni, a, hd[2]), md)
            vs = adj_s.coalesce().values()
            a2 = torch.sparse_coo_tensor(after[1].indices(), v2, size=after[1].shape, is_coalesced=True)
            o, (nf, adj_f, _) = collect_ref(oi, (n2, a2, after[2]), (segs, vbase), B, t)
            vf = adj_f.coalesce().values()
        outs = (xs, ns, vs, o, nf, vf)
        if weights is None:
            weights = [torch.rand(v.shape, generator=gen).to(DEV) for v in outs]
        sum((v * w).sum() for v, w in zip(outs, weights)).backward()
        grads.append([v.grad for v in leaves])
    for a, b in zip(*grads):
        assert a is not None and b is not None and torch.equal(a, b)
    assert all(float(g.abs().max()) > 0 for g in grads[0])


# ---------------------------------------------------------------------------
# end to end against the oracle
# ---------------------------------------------------------------------------
EB, EN, EF, EH, ET = 4, 16, 8, 8, 12
HOPS = [1, 2, 4]


def _dev_gnn(ref, F, H):
    from gcm import nn as G
    g = G.Sequential("x, edges, weights", [(G.GraphConv(F, H), "x, edges, weights -> x"), torch.nn.Tanh(),
                                           (G.GraphConv(H, H), "x, edges, weights -> x"), torch.nn.Tanh()])
    g.load_state_dict(ref.state_dict())
    return g.to(DEV)


def _e2e_inputs(seed=0):
    gen = torch.Generator().manual_seed(seed)
    taus, mask = random_case(EB, ET, SEEDS[(EB, ET)])
    x = torch.rand(EB, ET, EF, generator=gen) * (torch.arange(ET)[None, :] < taus[:, None])[:, :, None]
    taus0 = torch.tensor([3, 0, 2, 1])
    x0 = torch.rand(EB, 3, EF, generator=gen) * (torch.arange(3)[None, :] < taus0[:, None])[:, :, None]
    w = torch.rand(EB, ET, EH, generator=gen)
    return x, taus, mask, x0, taus0, w


def _compare(got, want):
    """The bounds of test_sparse_rollout_matches_reference: state exact, beliefs rtol = atol = 1e-5, gradients
    rtol 1e-5 and atol 1e-5 of their largest entry (+ 1e-7 for the parameters)."""
    (o, state, gx, gp), (ow, state_w, gxw, gpw) = got, want
    _assert_state(state, state_w)
    print("worst belief difference %.3g" % float((o.cpu() - ow).abs().max()))
    torch.testing.assert_close(o.cpu(), ow, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gx.cpu(), gxw, rtol=1e-5, atol=1e-5 * float(gxw.abs().max()))
    assert gpw and set(gp) == set(gpw)
    for k, b in gpw.items():
        torch.testing.assert_close(gp[k].cpu(), b, rtol=1e-5, atol=1e-5 * float(b.abs().max()) + 1e-7, msg=k)


CONFIGS = ["canonical", "layered", "max_hops", "positional_encoder"]


@pytest.mark.parametrize("incoming", [False, True], ids=["from_none", "stored_state"])
@pytest.mark.parametrize("config", CONFIGS)
def test_rollout_with_resets_matches_oracle(config, incoming):
    from gcm.gcm import PositionalEncoding
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    torch.manual_seed(1)
    ref = osp.canonical_gnn(EF, EH)
    g = _dev_gnn(ref, EF, EH)
    x, taus, mask, x0, taus0, w = _e2e_inputs()
    kw, okw = {}, {}
    if config == "max_hops":
        kw = okw = {"max_hops": 2}
    if config == "positional_encoder":
        kw, okw = {"positional_encoder": PositionalEncoding(max_len=64)}, \
            {"positional_encoder": od.PositionalEncoding(max_len=64)}
    mem = SparseGCM(g, edge_selectors=TemporalEdge(HOPS), graph_size=EN, **kw)
    mem.fast_host = config != "layered"
    assert (mem._canonical() is not None) == (config in ("canonical", "layered"))
    sel = osp.TemporalEdge(HOPS)

    hd = hc = None
    if incoming:
        with torch.no_grad():
            _, hd = mem(x0.to(DEV), taus0.to(DEV), None)
            _, hc = osp.sparse_step(x0, taus0, None, ref, graph_size=EN, edge_selectors=sel, **okw)
        _assert_state(hd, hc)
    xd = x.to(DEV).requires_grad_(True)
    out, state = mem.rollout(xd, hd, taus.to(DEV), reset=mask.to(DEV))
    (out * w.to(DEV)).sum().backward()
    xc = x.clone().requires_grad_(True)
    out_c, state_c = stepwise_ref(xc, taus, hc, mask, ref, EN, edge_selectors=sel, **okw)
    (out_c * w).sum().backward()
    assert state[1].is_coalesced() and tuple(state[1].shape) == (EB, EN, EN)
    counts = torch.bincount(state[1].indices()[0], minlength=EB)
    assert torch.equal(state[1].gcm_bptr, torch.cat([counts.new_zeros(1), counts.cumsum(0)]))
    pad = (torch.arange(ET)[None, :] >= taus[:, None]).to(DEV)
    assert not out[pad].any()
    _compare((out.detach(), state, xd.grad, {k: p.grad for k, p in g.named_parameters()}),
             (out_c.detach(), state_c, xc.grad, {k: p.grad for k, p in ref.named_parameters()}))


# ---------------------------------------------------------------------------
# selectors and layers without an oracle twin: the same module, stepping with reset_hidden between the calls
# ---------------------------------------------------------------------------
def _nodewise(mem, x, taus, hidden, mask):
    """One node per call, reset_hidden ahead of a call where the mask says so (the only way at the parent)."""
    outs = []
    for s in range(x.shape[1]):
        live = s < taus
        if not bool(live.any()):
            outs.append(None)
            continue
        m = mask[:, s] & live
        if hidden is not None and bool(m.any()):
            hidden = mem.reset_hidden(hidden, m)
        o, hidden = mem(x[:, s:s + 1], live.long().to(DEV), hidden)
        outs.append(o)
    H = next(o for o in outs if o is not None).shape[-1]
    return torch.cat([o if o is not None else x.new_zeros(x.shape[0], 1, H) for o in outs], dim=1), hidden


def _episodewise(mem, x, taus, hidden, mask):
    """One call per episode: call j feeds every graph its j-th segment whole, reset_hidden ahead of it."""
    segs, vbase = plan_ref(taus, mask)
    B, t, F = x.shape
    out = None
    for j in range(max(vbase[b + 1] - vbase[b] for b in range(B))):
        mine = [segs[vbase[b] + j] if vbase[b] + j < vbase[b + 1] else (b, 0, 0, 0) for b in range(B)]
        lens = torch.tensor([l for _, _, l, _ in mine])
        clear = torch.tensor([bool(e) and vbase[b] + j < vbase[b + 1] for b, (_, _, _, e) in enumerate(mine)])
        if hidden is not None and bool(clear.any()):
            hidden = mem.reset_hidden(hidden, clear)
        if not int(lens.max()):
            continue
        xj = torch.stack([torch.cat([x[b, s:s + l], x.new_zeros(int(lens.max()) - l, F)]) for b, s, l, _ in mine])
        o, hidden = mem(xj, lens.to(DEV), hidden)
        if out is None:
            out = x.new_zeros(B, t, o.shape[-1])
        pieces = out.clone()
        for b, s, l, _ in mine:
            if l:
                pieces[b, s:s + l] = o[b, :l]
        out = pieces
    return out, hidden


def _no_twin_module(name):
    from gcm import nn as G
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.learned import LearnedEdge
    from gcm.sparse_edge_selectors.spatial import SpatialKNNEdge, SpatialRadiusEdge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    torch.manual_seed(4)
    g = _dev_gnn(osp.canonical_gnn(EF, EH), EF, EH)
    if name == "knn":
        sel = SpatialKNNEdge(slice(0, 2), 3)
    elif name == "radius":
        sel = SpatialRadiusEdge(slice(0, 2), 0.5)
    elif name == "learned":
        sel = LearnedEdge(EF, num_edge_samples=3, deterministic=True, store_grads=False, log_stats=False).to(DEV)
    else:
        sel = TemporalEdge([1, 2])
        g = G.Sequential("x, edges, weights", [(G.GATConv(EF, EH // 2, heads=2), "x, edges, weights -> x"),
                                               torch.nn.Tanh(), (G.GATConv(EH, EH), "x, edges, weights -> x")]).to(DEV)
    return SparseGCM(g, edge_selectors=sel, graph_size=EN), g, sel


@pytest.mark.parametrize("incoming", [False, True], ids=["from_none", "stored_state"])
@pytest.mark.parametrize("name", ["knn", "radius", "learned", "gat"])
def test_rollout_with_resets_matches_stepping_with_reset_hidden(name, incoming):
    """State exactly; beliefs and gradients at the bounds the spatial selectors' own SparseGCM test
    (test_sparse_gcm_matches_reference_fixture) and test_sparse_rollout_matches_reference use.  The reference run
    feeds one node per call - except SpatialKNNEdge, whose k nearest are taken among ALL nodes of a call before the
    causal filter (a later node of the same call can displace an earlier one), so that one call of tau nodes is not
    tau calls of one node for it with or without resets: its reference run feeds one whole episode per call."""
    mem, g, sel = _no_twin_module(name)
    x, taus, mask, x0, taus0, w = _e2e_inputs(seed=2)
    params = dict(g.named_parameters())
    params.update({"sel." + k: p for k, p in sel.named_parameters()})
    res = []
    for run in ("rollout", "reference"):
        for p in params.values():
            p.grad = None
        hidden = None
        x0d = x0.to(DEV).requires_grad_(True)
        if incoming:
            _, hidden = mem(x0d, taus0.to(DEV), None)
        xd = x.to(DEV).requires_grad_(True)
        if run == "rollout":
            out, state = mem.rollout(xd, hidden, taus.to(DEV), reset=mask)
        else:
            out, state = (_episodewise if name == "knn" else _nodewise)(mem, xd, taus, hidden, mask)
        (out * w.to(DEV)).sum().backward()
        res.append((out.detach(), state, xd.grad, x0d.grad if incoming else None,
                    {k: p.grad.clone() for k, p in params.items() if p.grad is not None}))
    (o, s, gx, g0, gp), (ow, sw, gxw, g0w, gpw) = res
    assert state_equal((s[0].detach(), s[1].detach(), s[2]), (sw[0].detach(), sw[1].detach(), sw[2]))
    assert s[1]._nnz() > 0
    print("worst belief difference %.3g" % float((o - ow).abs().max()))
    torch.testing.assert_close(o, ow, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gx, gxw, rtol=1e-5, atol=1e-5 * float(gxw.abs().max()))
    if incoming:
        torch.testing.assert_close(g0, g0w, rtol=1e-5, atol=1e-5 * float(g0w.abs().max()))
    assert set(gp) == set(gpw) and gpw
    if name == "learned":
        assert any(k.startswith("sel.") and float(v.abs().max()) > 0 for k, v in gpw.items())
    for k, b in gpw.items():
        torch.testing.assert_close(gp[k], b, rtol=1e-5, atol=1e-5 * float(b.abs().max()) + 1e-7, msg=k)


# ---------------------------------------------------------------------------
# overflow: only the longest episode has to fit
# ---------------------------------------------------------------------------
def _small(overflow="raise", N=8, F=3, H=5, path="cpp"):
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    torch.manual_seed(6)
    ref = osp.canonical_gnn(F, H)
    mem = SparseGCM(_dev_gnn(ref, F, H), edge_selectors=TemporalEdge([1, 2]), graph_size=N, overflow=overflow)
    mem.fast_host = path == "cpp"
    return mem, ref


@pytest.mark.parametrize("path", ["cpp", "layered"])
def test_episodes_that_fit_do_not_overflow(path):
    mem, ref = _small(path=path)
    x = torch.rand(2, 12, 3)
    mask = torch.zeros(2, 12, dtype=torch.bool)
    mask[:, 6] = True
    taus = torch.full((2,), 12)
    with pytest.raises(Exception, match="Overflow"):        # (T + tau > N without the resets)
        mem.rollout(x.to(DEV))
    out, state = mem.rollout(x.to(DEV), reset=mask)
    assert state[2].tolist() == [6, 6]
    with torch.no_grad():
        out_c, state_c = stepwise_ref(x, taus, None, mask, ref, 8, edge_selectors=osp.TemporalEdge([1, 2]))
    _assert_state(state, state_c)
    torch.testing.assert_close(out.detach().cpu(), out_c, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("path", ["cpp", "layered"])
def test_an_episode_of_nine_nodes_overflows(path):
    mem, _ = _small(path=path)
    mask = torch.zeros(2, 12, dtype=torch.bool)
    mask[:, 3] = True                                       # episodes of 3 and 9 nodes, N = 8
    with pytest.raises(Exception, match="Overflow"):
        mem.rollout(torch.rand(2, 12, 3, device=DEV), reset=mask)


@pytest.mark.parametrize("path", ["cpp", "layered"])
def test_wrap_applies_per_virtual_graph(path):
    """overflow="wrap": the same batch == the expanded call (restatement) run by hand through the same module."""
    mem, _ = _small(overflow="wrap", path=path)
    x = torch.rand(2, 12, 3, device=DEV)
    x[0, 4:] = 0
    taus = torch.tensor([4, 12], device=DEV)
    mask = torch.zeros(2, 12, dtype=torch.bool, device=DEV)
    mask[1, 5] = mask[1, 9] = True
    # graph 0: 6 stored + 4 new nodes > N = 8 and no reset, so it wraps; graph 1: 5 stored + 5 new wrap inside its
    # first virtual graph, the next two (4 and 3 nodes) start empty
    with torch.no_grad():
        _, hidden = mem(torch.rand(2, 6, 3, device=DEV), torch.tensor([6, 5], device=DEV), None)
        out, state = mem.rollout(x, hidden, taus, reset=mask)
        xs, taus_s, hs, plan = expand_ref(x, taus, hidden, mask)
        out_s, hs2 = mem(xs, taus_s, (hs[0], hs[1].coalesce(), hs[2]))
        want_out, want = collect_ref(out_s, hs2, plan, 2, 12)
    assert torch.equal(out, want_out) and state_equal(state, want)
    assert state[2].tolist() == [8, 3]
    # the batch of test_an_episode_of_nine_nodes_overflows: a virtual graph of 9 > N nodes raises in wrap mode too
    # (tau_b > N) - in the call with resets as in the expanded call run by hand
    x9, taus9 = torch.rand(2, 12, 3, device=DEV), torch.full((2,), 12, device=DEV)
    mask9 = torch.zeros(2, 12, dtype=torch.bool, device=DEV)
    mask9[:, 3] = True
    with pytest.raises(Exception, match="Overflow"):
        mem.rollout(x9, reset=mask9)
    xs, taus_s, hs, _ = expand_ref(x9, taus9, mem.get_initial_hidden_state(x9), mask9)
    assert taus_s.tolist() == [3, 9, 3, 9]
    with pytest.raises(Exception, match="Overflow"):
        mem(xs, taus_s, (hs[0], hs[1].coalesce(), hs[2]))


# ---------------------------------------------------------------------------
# the stepwise chain, and where the mask lives
# ---------------------------------------------------------------------------
def test_a_call_with_resets_ends_the_stepwise_chain():
    """F = H = 32 (the cached stepwise chain): four single-node calls on the chain, a call with resets, three more
    single-node calls == the same module with stepwise_cache = False: state exactly, beliefs at rtol = atol = 1e-5."""
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    B, F, N = 3, 32, 16
    torch.manual_seed(9)
    g = _dev_gnn(osp.canonical_gnn(F, F), F, F)
    xs = [torch.rand(B, 1, F, device=DEV) for _ in range(7)]
    xr = torch.rand(B, 4, F, device=DEV)
    mask = torch.tensor([[False, False, True, False], [False] * 4, [True, False, False, True]])
    one = torch.ones(B, dtype=torch.long, device=DEV)
    runs = []
    for cached in (True, False):
        mem = SparseGCM(g, edge_selectors=TemporalEdge([1, 2]), graph_size=N)
        mem.stepwise_cache = cached
        hidden, outs = None, []
        with torch.no_grad():
            for s in range(4):
                o, hidden = mem(xs[s], one, hidden)
                outs.append(o)
            if cached:
                assert mem._chain is not None and mem._chain.live() and mem._chain.steps() == 4
            o, hidden = mem.rollout(xr, hidden, reset=mask)
            outs.append(o)
            assert mem._chain is None and mem.stepwise_cache == cached
            assert hidden[2].tolist() == [2, 8, 1]
            for s in range(4, 7):
                o, hidden = mem(xs[s], one, hidden)
                outs.append(o)
        runs.append((torch.cat(outs, dim=1), hidden))
    assert state_equal(runs[0][1], runs[1][1])
    torch.testing.assert_close(runs[0][0], runs[1][0], rtol=1e-5, atol=1e-5)


def test_mask_on_the_cpu_and_on_the_device_give_identical_results():
    mem, _ = _small(N=16)
    x, taus, mask = torch.rand(4, 12, 3, device=DEV), *random_case(4, 12, SEEDS[(4, 12)])
    with torch.no_grad():
        _, hidden = mem(torch.rand(4, 2, 3, device=DEV), torch.tensor([2, 0, 1, 2], device=DEV), None)
        a = mem.rollout(x, hidden, taus.to(DEV), reset=mask)
        b = mem.rollout(x, hidden, taus.to(DEV), reset=mask.to(DEV))
        c = mem(x, taus.to(DEV), hidden, reset=mask)
    assert torch.equal(a[0], b[0]) and state_equal(a[1], b[1])
    assert torch.equal(a[0], c[0]) and state_equal(a[1], c[1])


def test_a_mask_without_a_valid_entry_runs_the_call_as_it_is():
    mem, _ = _small(N=16)
    x = torch.rand(3, 5, 3, device=DEV)
    taus = torch.tensor([5, 2, 0], device=DEV)
    pad = torch.arange(5, device=DEV)[None, :] >= taus[:, None]
    with torch.no_grad():
        want = mem(x, taus, None)
        for mask in (torch.zeros(3, 5, dtype=torch.bool), pad):
            got = mem(x, taus, None, reset=mask)
            assert torch.equal(got[0], want[0]) and state_equal(got[1], want[1])
