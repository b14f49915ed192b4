"""Training loops: optimiser steps between uses of one memory module - between rollouts, inside a kept chain of
hidden states (truncated BPTT), between replays of a captured loop + backward - against the CPU oracle driven the
same way (tests/_training.py: float32 and float64 trajectories, tolerances from their distance).  What a module that
keeps a packed parameter vector, a weight image or a per-chain cache from before an optimiser step gets wrong:
every trajectory asserts that such a run would sit orders of magnitude outside the bounds.  Needs an MI355X."""
import pytest
import torch

import _training as tr
from oracle import dense as od
from oracle import sparse as osp
from test_dense_gpu import dev_gnn_from, DEV
from test_sparse_gpu import dev_sparse_gnn

pytestmark = pytest.mark.gpu

K = 6
# name: (selector, (B, N, F, H, T)) - the smallest shapes that reach each kernel family, T > N (the chain leaves its fill phase)
CASES = {
    "temporal": (("temporal", [1, 2, 4]), (5, 16, 32, 32, 40)),      # cached chain, then rolled
    "temporal_padded": (("temporal", [2, 5]), (3, 24, 20, 48, 30)),  # padded widths
    "dense": (("dense",), (5, 16, 32, 32, 40)),                      # colcache, then its ring form
    "euclid": (("euclid", 3.0), (40, 32, 32, 32, 40)),               # matrix-core selector, ring
}
# LearnedEdge (inputs: tests/_training.py, LEARNED_*): the seed was picked on the CPU so that the float32 and float64 oracle
# runs select identical adjacencies at every step, no chosen entry is closer than 1e-3 (in logit + noise) to the best
# one not chosen, and every edge-network tensor with a gradient moves >= 1000 x its atol - all asserted by the test
LEARNED = (("learned", 3), (40, 32, 32, 32, 40))
LEARNED_K, LEARNED_SEED = 3, 3
SEED = 11      # (any seed will do: tr.assert_sensitive checks, per test, that the inputs it gives are sensitive enough)


class _Tally:
    """Worst error / atol ratio per quantity; everything is measured (and printed) before anything is asserted."""

    def __init__(self, name):
        self.name, self.worst, self.bad = name, {}, []

    def add(self, what, err, atol, where):
        ratio = err / atol
        self.worst[what] = max(self.worst.get(what, 0.0), ratio)
        if not err <= atol:
            self.bad.append((what, where, err, atol))

    def close(self, t):
        move = min(t.move.values()) if t.move else float("nan")
        stale = min(t.stale) if t.stale else float("nan")
        print("\nTRAINING %s: worst error/atol %s | oracle movement/atol >= %.0f, stale beliefs/atol >= %.0f"
              % (self.name, {k: round(v, 3) for k, v in self.worst.items()}, move, stale))
        assert not self.bad, self.bad[:6]


def _compare(tally, t, k, loss, out, named):
    tally.add("loss", abs(float(loss) - t.r64.losses[k]), t.loss_atol[k], k)
    tally.add("belief", float((out.detach().cpu().double() - t.r64.beliefs[k]).abs().max()), t.belief_atol[k], k)
    for name, p in named.items():
        tally.add("param", float((p.detach().cpu().double() - t.r64.params[k][name]).abs().max()),
                  t.param_atol[k][name], (k, name))


def _build(t, donate):
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.edge_selectors.dense import DenseEdge
    from gcm.edge_selectors.distance import EuclideanEdge
    from gcm.edge_selectors.learned import LearnedEdge
    B, N, F, H, T = t.shapes
    ref = od.canonical_gnn(F, H)
    ref.load_state_dict(t.init["gnn"])
    g = dev_gnn_from(ref, [(F, H, torch.nn.Tanh), (H, H, torch.nn.Tanh)])
    named = dict(g.named_parameters())
    kind = t.kind
    if kind[0] == "temporal":
        sel = TemporalBackedge(kind[1])
    elif kind[0] == "dense":
        sel = DenseEdge()
    elif kind[0] == "euclid":
        sel = EuclideanEdge(kind[1])
    else:
        sel = LearnedEdge(F, num_edge_samples=kind[1])
        sel.edge_network.load_state_dict(t.init["net"])
        sel = sel.to(DEV)
        named.update({"net." + k_: p for k_, p in sel.edge_network.named_parameters()})
    return DenseGCM(g, edge_selectors=sel, graph_size=N, donate_state=donate), named


def _loop(mem, x, hidden, step=None):
    """step: where the injected gumbel draws of LearnedEdge are looked up ({"t": step index})"""
    outs = []
    for i in range(x.shape[0]):
        if step is not None:
            step["t"] = i
        mx, hidden = mem(x[i], hidden)
        outs.append(mx)
    return torch.stack(outs), hidden


def _assert_path(mem, t, donate):
    """Which kernels ran - the expectations of test_rows_cached_steps_vs_oracle, test_rows_colcache_steps_vs_oracle and
    test_rows_path_distance_selectors_vs_fused_path for a donated chain from empty graphs."""
    B, N, F, H, T = t.shapes
    assert mem.rows_steps() > 0, "the live-row path was not taken"
    if not donate:
        return
    kind = t.kind[0]
    if kind == "dense":
        assert mem.rows_col_steps_taken() == T and mem.rows_cached_steps_taken() == 0
    elif kind == "euclid":
        assert mem.rows_cached_steps_taken() == T and mem.rows_rolled_steps_taken() == T - N
    elif kind == "temporal":
        steady = N > 2 * max(t.kind[1]) and F in (32, 64) and H in (32, 64)
        assert mem.rows_cached_steps_taken() == (T if steady else min(T, N))
        assert mem.rows_rolled_steps_taken() == (max(0, T - N) if steady else 0)


def _assert_final_state(hidden, t):
    want = t.r32.hidden
    assert torch.equal(hidden[1].detach().cpu(), want[1]), "adjacency must be bit exact"
    assert torch.equal(hidden[3].cpu(), want[3])
    assert torch.equal(hidden[0].detach().cpu(), want[0])


def _captured(t, mem, named, tgt, step=None):
    """donate_state=True, loop + backward captured once after a side-stream warm-up whose optimiser is thrown away
    (the initial parameters are then reloaded IN PLACE: the captured trajectory starts where the oracle's does).
    `tgt`: the target on the device - a static input of the graph like the observation buffer: the CALLER keeps it
    alive for as long as it replays.  -> (graph, static obs, loss, out, hidden)"""
    B, N, F, H, T = t.shapes
    params = list(named.values())
    p0 = [p.detach().clone() for p in params]
    obs = t.obs[0].to(DEV).clone()

    def iteration():
        out, hidden = _loop(mem, obs, None, step)
        loss = ((out - tgt) ** 2).mean()
        loss.backward()
        return loss, out, hidden

    throwaway = tr.make_optimizer(t.opt, params)
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for p in params:
                p.grad = None
            iteration()
            throwaway.step()
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.no_grad():
        for p, q in zip(params, p0):
            p.copy_(q)
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, out, hidden = iteration()
    return graph, obs, loss, out, hidden


# ---------------------------------------------------------------------------------------------------------
# A. trajectory parity on every dense step path
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", ["steps", "steps_donated", "rollout", "captured"])
@pytest.mark.parametrize("case", list(CASES))
def test_training_trajectory_vs_oracle(case, driver):
    """K = 6 iterations of: fresh observations, T steps from hidden = None, backward of ((out - target)**2).mean(),
    SGD(lr 0.05, momentum 0.9) step.  After every iteration the loss, the beliefs and every parameter against the
    float64 oracle (bounds of tests/_training.py); the last iteration's state bit equal to the float32 oracle's.
    Drivers: the per-step loop on a functional and on a donated state, rollout(), and the donated loop + backward
    captured once and replayed (static observation buffer, gradients zeroed in place, eager optimiser step)."""
    kind, shapes = CASES[case]
    t = tr.oracle_trajectory(kind, shapes, K, tr.SGD, SEED)
    tr.assert_sensitive(t)
    donate = driver in ("steps_donated", "captured")
    mem, named = _build(t, donate)
    tally = _Tally("A %s/%s" % (case, driver))
    tgt = t.target.to(DEV)
    if driver == "captured":
        graph, obs_buf, loss, out, hidden = _captured(t, mem, named, tgt)
        _assert_path(mem, t, donate)
        opt = tr.make_optimizer(t.opt, list(named.values()))
        for k in range(K):
            obs_buf.copy_(t.obs[k])
            for p in named.values():
                p.grad.zero_()
            graph.replay()
            opt.step()
            _compare(tally, t, k, loss, out, named)
    else:
        opt = tr.make_optimizer(t.opt, list(named.values()))
        for k in range(K):
            opt.zero_grad(set_to_none=True)
            x = t.obs[k].to(DEV)
            out, hidden = mem.rollout(x) if driver == "rollout" else _loop(mem, x, None)
            if driver != "rollout":
                _assert_path(mem, t, donate)
            loss = ((out - tgt) ** 2).mean()
            loss.backward()
            opt.step()
            _compare(tally, t, k, loss, out, named)
    torch.cuda.synchronize()
    _assert_final_state(hidden, t)
    mem.check_flags()
    tally.close(t)


# ---------------------------------------------------------------------------------------------------------
# B. optimiser steps inside a kept chain (truncated BPTT)
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("donate", [False, True])
@pytest.mark.parametrize("case", ["temporal", "dense", "euclid"])
def test_training_steps_inside_a_kept_chain(case, donate):
    """ONE sequence of T = 40 steps cut into segments of 8: after each segment its loss is backpropagated, the
    optimiser steps and the hidden state is detached and kept.  From the second segment on every belief depends on
    rows inserted under older weights and must be recomputed under the new ones.  The module's answer is to DROP the
    per-chain caches at the optimiser step (_packed_params -> forget()): the first segment runs on them (8 cached /
    column-write steps), the segments behind it on the general live-row kernel from the kept, non-empty state (a chain
    takes the cached forms only from empty graphs) - asserted per segment, so that a cache carried across the step
    would be seen twice: in the counters and in the values.  Against the oracle doing exactly the same, after every
    segment."""
    kind, shapes = CASES[case]
    S, T = 8, shapes[4]
    t = tr.oracle_trajectory(kind, shapes, T // S, tr.SGD, SEED + 1, segments=S)
    tr.assert_sensitive(t)
    mem, named = _build(t, donate)
    tally = _Tally("B %s/%s" % (case, "donated" if donate else "functional"))
    opt = tr.make_optimizer(t.opt, list(named.values()))
    obs, tgt = t.obs[0].to(DEV), t.target.to(DEV)
    hidden = None
    for k in range(T // S):
        opt.zero_grad(set_to_none=True)
        if hidden is not None:
            hidden = tuple(h.detach() for h in hidden)
        out, hidden = _loop(mem, obs[k * S:(k + 1) * S], hidden)
        assert mem.rows_steps() == (k + 1) * S, "the live-row path was not taken"
        first = k == 0
        if case == "dense":        # (the column-write form takes a functional state too)
            assert mem.rows_col_steps_taken() == (S if first else 0) and mem.rows_cached_steps_taken() == 0
        else:                      # (the cached forms of forward hops / EuclideanEdge: donated state only)
            assert mem.rows_cached_steps_taken() == (S if first and donate else 0)
            assert mem.rows_col_steps_taken() == 0 and mem.rows_rolled_steps_taken() == 0
        loss = ((out - tgt[k * S:(k + 1) * S]) ** 2).mean()
        loss.backward()
        opt.step()
        _compare(tally, t, k, loss, out, named)
    _assert_final_state(hidden, t)
    mem.check_flags()
    tally.close(t)


# ---------------------------------------------------------------------------------------------------------
# C. LearnedEdge: the edge network trains too, gumbel draws injected
# ---------------------------------------------------------------------------------------------------------
def _learned_trajectory():
    t = tr.oracle_trajectory(LEARNED[0], LEARNED[1], LEARNED_K, tr.SGD, LEARNED_SEED)
    assert t.same_edges, "the float32 and float64 oracle runs selected different edges: pick another seed"
    assert t.gap > 1e-3, ("a selection is within 1e-3 of flipping: pick another seed", t.gap)
    # the two biases whose gradient is zero analytically (tr.zero_gradient) - and no other tensor - stand still
    assert sorted(tr.zero_gradient(t.r64)) == ["net.5.bias", "net.6.bias"]
    assert len(t.move) == len(t.r64.p0) - 2
    tr.assert_sensitive(t)
    return t


def _learned_taken(mem):
    cfg = mem._cfg_last[3] if mem._cfg_last else None
    return cfg is not None and cfg.learned_sel is not None


@pytest.mark.parametrize("driver", ["steps", "captured"])
def test_training_learned_edge_vs_oracle(driver):
    """(i) LearnedEdge(num_edge_samples=3), its edge network in the optimiser, one recorded gumbel tensor per
    iteration and step through noise_fn: the functional per-step loop and the captured donated loop against the
    oracle's LearnedEdge with the same draws.  (ii) captured: after every replay, the beliefs and the state equal -
    bit for bit - those of a FRESH eager module loaded with the parameters the replay ran under, on the same inputs
    (a staleness check that needs no oracle)."""
    t = _learned_trajectory()
    B, N, F, H, T = t.shapes
    step = {"t": 0}
    donate = driver == "captured"
    mem, named = _build(t, donate)
    noise = t.noise[0].to(DEV).clone()
    mem.edge_selectors.noise_fn = lambda like: noise[step["t"]]
    tally = _Tally("C learned/%s" % driver)
    opt = tr.make_optimizer(t.opt, list(named.values()))
    tgt = t.target.to(DEV)
    if driver == "captured":
        graph, obs_buf, loss, out, hidden = _captured(t, mem, named, tgt, step)
        assert _learned_taken(mem)
        for k in range(LEARNED_K):
            obs_buf.copy_(t.obs[k])
            noise.copy_(t.noise[k])
            for p in named.values():
                if p.grad is not None:
                    p.grad.zero_()
            before = {n_: p.detach().clone() for n_, p in named.items()}
            graph.replay()
            opt.step()
            _compare(tally, t, k, loss, out, named)
            # (ii) a fresh eager module under the parameters of this replay
            mem_e, named_e = _build(t, donate)
            with torch.no_grad():
                for n_, p in named_e.items():
                    p.copy_(before[n_])
            mem_e.edge_selectors.noise_fn = mem.edge_selectors.noise_fn
            out_e, hid_e = _loop(mem_e, obs_buf, None, step)
            mem_e.check_flags()
            assert torch.equal(out_e.detach(), out.detach()), ("beliefs differ from a fresh eager module", k)
            assert torch.equal(hid_e[1].detach(), hidden[1].detach()) and torch.equal(hid_e[0].detach(), hidden[0].detach())
            assert torch.equal(hid_e[3], hidden[3])
    else:
        for k in range(LEARNED_K):
            opt.zero_grad(set_to_none=True)
            noise.copy_(t.noise[k])
            out, hidden = _loop(mem, t.obs[k].to(DEV), None, step)
            assert _learned_taken(mem)
            loss = ((out - tgt) ** 2).mean()
            loss.backward()
            opt.step()
            _compare(tally, t, k, loss, out, named)
    torch.cuda.synchronize()
    _assert_final_state(hidden, t)
    mem.check_flags()
    tally.close(t)


# ---------------------------------------------------------------------------------------------------------
# D. SparseGCM
# ---------------------------------------------------------------------------------------------------------
def _sparse_stepwise(mem, x, taus, hidden, taus_mode):
    outs = []
    for i in range(x.shape[1]):
        if taus_mode == "rewritten":
            taus.fill_(1)             # an ordinary, versioned write: the sizes memo must miss
        o, hidden = mem(x[:, i:i + 1], taus, hidden)
        outs.append(o)
    return torch.cat(outs, dim=1), hidden


def test_training_dense_and_sparse_learn_the_same():
    """The reference's test_learning_temporal_edges on the product: three Adam iterations (default settings) of
    DenseGCM per step, SparseGCM one-shot and SparseGCM one node per call, all from the same initial weights and on
    the same fresh observations, at the reference's own shape (F = 3: below the widths of the stepwise chain's cached
    kernels - those run in test_training_sparse_trajectory_vs_oracle[stepwise-*]).  The reference's own conditions - node matrices equal,
    dense-vs-sparse beliefs and parameters within 0.01 after every step -; its exact equality of the dense and the
    stepwise beliefs becomes the float64 bound of tests/_training.py on each of them."""
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    B, N, F, ts, iters, hops = 3, 8, 3, 8, 3, [1, 2]
    shapes = (B, N, F, F, ts)
    t = tr.sparse_trajectory(shapes, hops, None, iters, ("adam",), 14, stepwise=True, loss="mean")
    tr.assert_sensitive(t, loss_falls=False)     # (out.mean() on fresh observations: no loss to watch falling)
    from gcm import nn as G
    ref_s = osp.canonical_gnn(F, F, act=None)
    ref_s.load_state_dict(t.init)
    dense_g = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(F, F), "x, adj -> x"),
                                                      (G.DenseGraphConv(F, F), "x, adj -> x")])
    dense_g.load_state_dict(t.init)
    dense_g = dense_g.to(DEV)
    gs = [dev_sparse_gnn(ref_s, F, F, None) for _ in range(2)]
    dense = DenseGCM(dense_g, edge_selectors=TemporalBackedge(hops), graph_size=N)
    one_shot = SparseGCM(gs[0], edge_selectors=TemporalEdge(hops), graph_size=N)
    stepwise = SparseGCM(gs[1], edge_selectors=TemporalEdge(hops), graph_size=N)
    opts = [torch.optim.Adam(m.parameters()) for m in (dense, one_shot, stepwise)]
    tally = _Tally("D port")
    for k in range(iters):
        for o in opts:
            o.zero_grad()
        x = t.obs[k].to(DEV)
        d_out, d_hid = _loop(dense, x.transpose(0, 1).contiguous(), None)
        d_out = d_out.transpose(0, 1)
        s_out, s_hid = one_shot(x, torch.full((B,), ts, dtype=torch.long, device=DEV), None)
        w_out, w_hid = _sparse_stepwise(stepwise, x, torch.ones(B, dtype=torch.long, device=DEV), None, "same")
        assert torch.equal(d_hid[0], s_hid[0]) and torch.equal(d_hid[0], w_hid[0])
        assert torch.equal(d_hid[1].nonzero().T, s_hid[1].coalesce().indices())
        assert torch.allclose(d_out, s_out, atol=0.01)
        for name, got in (("dense", d_out), ("stepwise", w_out)):
            tally.add("belief " + name, float((got.detach().cpu().double() - t.r64.beliefs[k]).abs().max()),
                      t.belief_atol[k], k)
        for out_, o in zip((d_out, s_out, w_out), opts):
            out_.mean().backward()
            o.step()
        for g_ in gs:
            for k_, v in g_.state_dict().items():
                assert torch.allclose(v, dense_g.state_dict()[k_], atol=0.01), ("parameters diverged", k, k_)
    tally.close(t)


@pytest.mark.parametrize("driver,taus_mode", [("dense", "same"), ("one_shot", "same"), ("one_shot", "rewritten"),
                                              ("stepwise", "same"), ("stepwise", "rewritten")])
def test_training_sparse_trajectory_vs_oracle(driver, taus_mode):
    """SGD as in A at B = 4, N = 16, F = H = 32, 12 nodes per iteration against oracle/sparse.py::sparse_step in
    float32 / float64: DenseGCM per step, SparseGCM one-shot, SparseGCM one node per call - the last with an
    optimiser step also in the middle of its kept chain (after node 6, hidden detached).  taus: the same tensor object
    for every call (the sizes memo hits), or rewritten in place through the version counter before every call (it
    must miss)."""
    from gcm.gcm import DenseGCM
    from gcm.sparse_gcm import SparseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    shapes, hops = (4, 16, 32, 32, 12), [1, 2]
    B, N, F, H, ts = shapes
    split = 6 if driver == "stepwise" else None
    t = tr.sparse_trajectory(shapes, hops, torch.nn.Tanh, 3 if split else K, tr.SGD, 13, stepwise=split is not None,
                             split=split)
    tr.assert_sensitive(t)
    ref = osp.canonical_gnn(F, H)
    ref.load_state_dict(t.init)
    if driver == "dense":
        ref_d = od.canonical_gnn(F, H)
        ref_d.load_state_dict(t.init)
        g = dev_gnn_from(ref_d, [(F, H, torch.nn.Tanh), (H, H, torch.nn.Tanh)])
        mem = DenseGCM(g, edge_selectors=TemporalBackedge(hops), graph_size=N)
    else:
        g = dev_sparse_gnn(ref, F, H, torch.nn.Tanh)
        mem = SparseGCM(g, edge_selectors=TemporalEdge(hops), graph_size=N)
    named = dict(g.named_parameters())
    opt = tr.make_optimizer(t.opt, list(named.values()))
    tally = _Tally("D %s/%s" % (driver, taus_mode))
    tgt = t.target.to(DEV)
    taus = torch.full((B,), 1 if driver == "stepwise" else ts, dtype=torch.long, device=DEV)
    n = 0
    for k in range(t.K):
        x = t.obs[k].to(DEV)
        hidden = None
        for a, b in zip(t.cuts[:-1], t.cuts[1:]):
            opt.zero_grad(set_to_none=True)
            if hidden is not None:
                hidden = tuple(h.detach() for h in hidden)
            if driver == "dense":
                out, hidden = _loop(mem, x.transpose(0, 1).contiguous(), None)
                out = out.transpose(0, 1)
            elif driver == "one_shot":
                if taus_mode == "rewritten":
                    taus.fill_(ts)
                out, hidden = mem(x, taus, None)
            else:
                out, hidden = _sparse_stepwise(mem, x[:, a:b], taus, hidden, taus_mode)
                # from hidden = None: on the chain's caches (step_ext.cpp: SparseChain); behind the optimiser step in
                # the middle of the chain: the chain has ended (test_sparse_stepwise_cached_chain_ends_and_restarts)
                if a == 0:
                    assert mem._chain.live() and mem._chain.steps() == b - a, "the stepwise chain was not taken"
                else:
                    assert not mem._chain.live()
            loss = ((out - tgt[:, a:b]) ** 2).mean()
            loss.backward()
            opt.step()
            _compare(tally, t, n, loss, out, named)
            n += 1
    if driver == "dense":
        assert torch.equal(hidden[0].cpu(), t.r32.hidden[0])
        assert torch.equal(hidden[1].cpu().nonzero().T, t.r32.hidden[1].coalesce().indices())
    else:
        assert torch.equal(hidden[0].cpu(), t.r32.hidden[0]) and torch.equal(hidden[2].cpu(), t.r32.hidden[2])
        assert torch.equal(hidden[1].coalesce().indices().cpu(), t.r32.hidden[1].coalesce().indices())
    tally.close(t)


# ---------------------------------------------------------------------------------------------------------
# E. the reference's test_dense_learn (the layered path: N = 10, F = 11 is outside the fused kernels)
# ---------------------------------------------------------------------------------------------------------
def test_training_dense_learn():
    """Twenty Adam(lr 0.005) iterations from the reference test's prefilled state (arange nodes, zero adjacency),
    T = 4 steps that feed each belief back as the next observation, loss = norm of the last belief, on a two-layer
    DenseGraphConv + Tanh GNN with TemporalBackedge([1]): the last loss is below the first (the reference's
    condition) and the loss sequence is the oracle's under the same Adam, rtol 1e-3."""
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    B, N, F, T, iters = 5, 10, 11, 4, 20
    init, want = tr.oracle_dense_learn(B, N, F, T, iters, ("adam", 0.005), 15)
    ref = od.canonical_gnn(F, F)
    ref.load_state_dict(init)
    g = dev_gnn_from(ref, [(F, F, torch.nn.Tanh), (F, F, torch.nn.Tanh)])
    mem = DenseGCM(g, edge_selectors=TemporalBackedge([1]), graph_size=N)
    opt = torch.optim.Adam(mem.parameters(), lr=0.005)
    losses = []
    for _ in range(iters):
        mem.zero_grad()
        obs = torch.ones(B, F, device=DEV)
        hidden = tuple(h.to(DEV) for h in tr.dense_learn_state(B, N, F))
        for _t in range(T):
            obs, hidden = mem(obs, hidden)
        loss = torch.norm(obs)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    mem.check_flags()
    print("\nTRAINING E: losses %.6f -> %.6f, worst relative distance to the oracle's %.2e"
          % (losses[0], losses[-1], max(abs(a - b) / abs(b) for a, b in zip(losses, want))))
    assert losses[-1] < losses[0], f"Final loss {losses[-1]} not better than init loss {losses[0]}"
    torch.testing.assert_close(torch.tensor(losses), torch.tensor(want), rtol=1e-3, atol=0)
