"""Helpers of tests/test_training_gpu.py: the CPU oracle driven the way a training loop drives the memory
module - optimiser steps between rollouts (or between the segments of one kept chain) - in float32 and in
float64, and the tolerances that follow from the two runs.

The bound rule is the one of tests/_golden.py (what fp32 can deliver for the case, not a fixed number):

    parameter tensor after step k:  atol = max(3 x |oracle32 - oracle64|_max, floor_k)
    beliefs of iteration k:         atol = max(3 x |oracle32 - oracle64|_max, 2e-6)            (fp64_bound's floor)
    loss of iteration k:            atol = max(3 x |oracle32 - oracle64|, 2 mean|out - target| x belief atol)

floor_k: fp64_grad_bound's floor - 5e-7 of a gradient's scale - for every step's gradient, pushed through the
optimiser's own recurrence (SGD with momentum mu: b_k = mu b_k-1 + e_k, floor_k = floor_k-1 + lr b_k with
e_k = 5e-7 |g_k|_max): the parameter error a run makes whose every gradient is as good as that floor asks.
The loss floor is the first-order change of mean((out - target)^2) under a belief error of the belief atol.

Every trajectory also carries what makes a green comparison mean something (`sensitivity`): how far each
parameter tensor moved over the run against its atol, and how far the float64 beliefs of an iteration are from
the ones the PREVIOUS iteration's parameters give on the same inputs (a stale parameter vector or cache)."""
import copy
import math
import types

import torch

from oracle import dense as od
from oracle import sparse as osp

GRAD_FLOOR = 5e-7        # fp64_grad_bound / fp64_rollout_bounds
BELIEF_FLOOR = 2e-6      # fp64_bound
FACTOR = 3.0
MOVE_FACTOR = 1000.0     # a parameter tensor's movement over the run >= MOVE_FACTOR x its atol
STALE_FACTOR = 100.0     # beliefs under the previous step's parameters differ by >= STALE_FACTOR x their atol

SGD = ("sgd", 0.05, 0.9)     # the parity optimiser (Adam's g / sqrt(v) blows fp32 noise up on near-zero entries)

# The LearnedEdge case: inputs under which EVERY edge-network tensor with a gradient moves >= MOVE_FACTOR x its atol in
# three SGD steps (searched on the CPU).  Observations uniform in [-1.5, 1.5): a selected edge changes the belief more,
# so the edge network's gradient grows.  The default edge network with its Linear layers x 2 (livelier logits: the
# sampled rows change over time) and its LayerNorm weights at 0.5 instead of 1: a parameter stored near 1 or 2 is only
# good to one float32 ulp of 1.2e-7 / 2.4e-7 per step, which is most of such a tensor's atol; at 0.5 an ulp is 6e-8.
LEARNED_OBS_SCALE, LEARNED_LINEAR_GAIN, LEARNED_LAYERNORM_WEIGHT = 3.0, 2.0, 0.5

_cache = {}


def make_optimizer(opt, params):
    if opt[0] == "sgd":
        return torch.optim.SGD(params, lr=opt[1], momentum=opt[2])
    assert opt[0] == "adam"
    return torch.optim.Adam(params, **({"lr": opt[1]} if len(opt) > 1 else {}))


def gumbel(shape, gen):
    return -torch.empty(shape).exponential_(generator=gen).log()


class _WatchedLearnedEdge(od.LearnedEdge):
    """od.LearnedEdge that also records how far its decisions are from flipping: `gap` - the smallest distance
    in logit + noise between a chosen entry and the best one not chosen in its row - and `cut` - the smallest
    |log softmax - log cutoff| over all candidates (the decision itself is softmax > 1 / (1 + k))."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.gap, self.cut = math.inf, math.inf

    def __call__(self, nodes, adj, weights, num_nodes, B):
        if int(num_nodes.max()) >= 1:
            with torch.no_grad():
                N = adj.shape[-1]
                width = int(num_nodes.max())
                live = torch.arange(N)[None, :] < num_nodes[:, None]
                b_idx, j_idx = torch.nonzero(live, as_tuple=True)
                pair = torch.cat((nodes[b_idx, num_nodes[b_idx]], nodes[b_idx, j_idx]), dim=-1)
                z = torch.full((B, width), -1e10, dtype=nodes.dtype).index_put((b_idx, j_idx), self.net(pair).squeeze(-1))
                z = z + self.noise_fn(z.shape)
                soft = torch.softmax(z, dim=-1)
                ok = live[:, :width]
                cutoff = 1.0 / (1 + self.k)
                chosen, rest = ok & (soft > cutoff), ok & ~(soft > cutoff)
                lo = torch.where(chosen, z, torch.full_like(z, math.inf)).min(dim=1).values
                hi = torch.where(rest, z, torch.full_like(z, -math.inf)).max(dim=1).values
                both = chosen.any(dim=1) & rest.any(dim=1)
                if bool(both.any()):
                    self.gap = min(self.gap, float((lo - hi)[both].min()))
                self.cut = min(self.cut, float((soft[ok].log() - math.log(cutoff)).abs().min()))
        return super().__call__(nodes, adj, weights, num_nodes, B)


def dense_observations(kind, shapes, K, gen):
    """K tensors [T, B, F]: uniform in [-0.5, 0.5) - sums over up to N nodes stay off tanh's flat ends -; for the
    Euclidean selector clusters that every graph visits in turn (the cross-batch mean distance separates them,
    as in test_rows_path_distance_selectors_vs_fused_path), so that the decisions sit far from the threshold."""
    B, N, F, H, T = shapes
    if kind[0] == "euclid":
        centres = 3 * torch.randn(6, F, generator=gen)
        return [centres[torch.arange(T) % 6][:, None, :] + 0.05 * torch.randn(T, B, F, generator=gen) for _ in range(K)]
    sc = LEARNED_OBS_SCALE if kind[0] == "learned" else 1.0
    return [sc * (torch.rand(T, B, F, generator=gen) - 0.5) for _ in range(K)]


def _dense_run(kind, shapes, K, opt, init, obs, target, noise, dtype, segments):
    B, N, F, H, T = shapes
    gnn = od.canonical_gnn(F, H)
    gnn.load_state_dict(init["gnn"])
    gnn = gnn.to(dtype)
    mods = {"": gnn}
    step = {"k": 0, "t": 0}
    watch = None
    if kind[0] == "learned":
        net = od.build_edge_network(F)
        net.load_state_dict(init["net"])
        mods["net."] = net = net.to(dtype)
        nf = lambda shape: noise[step["k"]][step["t"]][:, : shape[1]].to(dtype)
        watch = _WatchedLearnedEdge(net, num_edge_samples=kind[1], noise_fn=nf)

    def selector(ms):
        if kind[0] == "temporal":
            return od.TemporalBackedge(kind[1])
        if kind[0] == "dense":
            return od.DenseEdge()
        if kind[0] == "euclid":
            return od.EuclideanEdge(kind[1])
        if ms is mods:
            return watch
        return od.LearnedEdge(ms["net."], num_edge_samples=kind[1], noise_fn=watch.noise_fn)

    def rollout(ms, x, hidden, seq, t0, adjs=None):
        sel, outs = selector(ms), []
        for t in range(x.shape[0]):
            step["k"], step["t"] = seq, t0 + t          # (the draws of this step: noise[seq][t0 + t])
            mx, hidden = od.dense_step(x[t], hidden, ms[""], graph_size=N, edge_selectors=sel)
            outs.append(mx)
            if adjs is not None:
                adjs.append(hidden[1].detach() != 0)
        return torch.stack(outs), hidden

    named = lambda ms: {pre + k: p for pre, m in ms.items() for k, p in m.named_parameters()}
    params = named(mods)
    optimizer = make_optimizer(opt, list(params.values()))
    stale_mods = copy.deepcopy(mods)
    r = types.SimpleNamespace(losses=[], beliefs=[], params=[], grads=[], stale=[], adjs=[], hidden=None,
                              p0={k: p.detach().clone() for k, p in params.items()})
    hidden = None
    for k in range(K):
        if segments:
            seq, t0 = 0, k * segments
            x, tgt = obs[0][t0:t0 + segments], target[t0:t0 + segments]
            hidden = None if hidden is None else tuple(h.detach() for h in hidden)
        else:
            seq, t0, x, tgt, hidden = k, 0, obs[k], target, None
        x, tgt = x.to(dtype), tgt.to(dtype)
        if k > 0 and dtype == torch.float64:     # the same inputs under the parameters of one step earlier
            with torch.no_grad():
                so, _ = rollout(stale_mods, x, hidden, seq, t0)
            r.stale.append(so)
        optimizer.zero_grad(set_to_none=True)
        adjs = []
        out, hidden = rollout(mods, x, hidden, seq, t0, adjs if kind[0] == "learned" else None)
        loss = ((out - tgt) ** 2).mean()
        loss.backward()
        for pre, m in mods.items():
            stale_mods[pre].load_state_dict(m.state_dict())
        optimizer.step()
        r.losses.append(float(loss.detach()))
        r.beliefs.append(out.detach())
        r.grads.append({n: p.grad.detach().clone() for n, p in params.items()})
        r.params.append({n: p.detach().clone() for n, p in params.items()})
        r.adjs.append(adjs)
    r.hidden = tuple(h.detach() for h in hidden)
    if watch is not None:
        r.gap, r.cut = watch.gap, watch.cut
    return r


def _bounds(r32, r64, opt, targets):
    """-> (param_atol[k][name] or None without the SGD recurrence, belief_atol[k], loss_atol[k]).
    targets=None: the loss is out.mean() (slope 1 in the beliefs)."""
    K = len(r64.losses)
    belief_atol, loss_atol = [], []
    for k in range(K):
        err = float((r32.beliefs[k].double() - r64.beliefs[k]).abs().max())
        belief_atol.append(max(FACTOR * err, BELIEF_FLOOR))
        slope = 1.0 if targets is None else 2.0 * float((r64.beliefs[k] - targets[k].double()).abs().mean())
        loss_atol.append(max(FACTOR * abs(r32.losses[k] - r64.losses[k]), slope * belief_atol[-1]))
    if opt[0] != "sgd":
        return None, belief_atol, loss_atol
    _, lr, mu = opt
    param_atol = [dict() for _ in range(K)]
    # (the edge network's tensors share one gradient scale, as in test_learned_fused_gpu._check_learned_grads: two
    #  of its biases have an analytically zero gradient - see zero_gradient() - and no scale of their own)
    net_scale = [max([float(g.abs().max()) for n, g in r64.grads[k].items() if n.startswith("net.")] or [0.0])
                 for k in range(K)]
    for name in r64.p0:
        buf = floor = 0.0
        for k in range(K):
            scale = net_scale[k] if name.startswith("net.") else float(r64.grads[k][name].abs().max())
            buf = mu * buf + GRAD_FLOOR * scale
            floor = floor + lr * buf
            err = float((r32.params[k][name].double() - r64.params[k][name]).abs().max())
            param_atol[k][name] = max(FACTOR * err, floor)
    return param_atol, belief_atol, loss_atol


def zero_gradient(r64):
    """Edge-network tensors whose gradient is zero analytically, found numerically: below 1e-9 of the edge network's
    gradient scale at every step of the float64 run.  LearnedEdge's logits enter the loss through a softmax over
    each row of candidates, so the logit gradients of a row sum to zero; the output bias (net.6.bias) shifts every
    logit of a row alike, and so does the last LayerNorm's bias (net.5.bias: through w . b of the output layer) -
    their gradients are that sum.  No input can move them: the movement condition does not apply to them."""
    names = [n for n in r64.p0 if n.startswith("net.")]
    out = []
    for n in names:
        if all(float(g[n].abs().max()) <= 1e-9 * max(float(g[m].abs().max()) for m in names) for g in r64.grads):
            out.append(n)
    return out


def _sensitivity(r64, param_atol, belief_atol):
    """-> (movement / atol per parameter tensor at the last step, stale distance / atol per iteration >= 1)."""
    move = {}
    if param_atol is not None:
        still = zero_gradient(r64)
        for name, p0 in r64.p0.items():
            if name in still:
                continue
            move[name] = float((r64.params[-1][name] - p0).abs().max()) / param_atol[-1][name]
    stale = [float((s - r64.beliefs[k + 1]).abs().max()) / belief_atol[k + 1] for k, s in enumerate(r64.stale)]
    return move, stale


def assert_sensitive(tr, loss_falls=True):
    """The sensitivity condition every parity test asserts: a module that kept a parameter vector, or a cache
    filled under it, from before an optimiser step cannot pass.  (Under Adam there are no parameter bounds and
    `move` is empty: the stale-belief condition alone.)"""
    for name, ratio in tr.move.items():
        assert ratio >= MOVE_FACTOR, ("parameter moved less than %g x its atol" % MOVE_FACTOR, name, ratio)
    assert len(tr.stale) == len(tr.r64.losses) - 1
    for k, ratio in enumerate(tr.stale):
        assert ratio >= STALE_FACTOR, ("beliefs under stale parameters closer than %g x atol" % STALE_FACTOR, k + 1, ratio)
    if tr.whole and loss_falls:      # (the segments of one sequence have targets and graph sizes of their own: nothing to compare)
        assert tr.r64.losses[-1] < tr.r64.losses[0], "the oracle's loss does not fall"


def oracle_trajectory(kind, shapes, K, opt, seed, segments=None):
    """The oracle's DenseGCM through K optimiser steps, in float32 (r32) and float64 (r64), same initial
    parameters, observations, loss ((out - target)**2).mean() against a fixed random target.
    kind: ("temporal", hops) | ("dense",) | ("euclid", max_distance) | ("learned", num_edge_samples);
    shapes (B, N, F, H, T); opt: SGD / ("adam"[, lr]).  segments=None: every iteration a rollout of fresh
    observations obs[k] from hidden = None.  segments=S: ONE sequence obs[0], an optimiser step after every S
    steps of it on a kept, detached hidden state (K = T // S).
    -> namespace: init (state dicts "gnn" [, "net"]), obs, target, noise (learned: [K][T, B, N] gumbel draws),
    r32 / r64 (losses, beliefs, params[k][name] after step k, grads, hidden of the last iteration, adjs),
    param_atol[k][name], belief_atol[k], loss_atol[k], move, stale (see assert_sensitive)."""
    key = ("dense", repr(kind), tuple(shapes), K, tuple(opt), seed, segments)
    if key in _cache:
        return _cache[key]
    B, N, F, H, T = shapes
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    init = {"gnn": copy.deepcopy(od.canonical_gnn(F, H).state_dict())}
    noise = None
    if kind[0] == "learned":
        net = od.build_edge_network(F)
        with torch.no_grad():
            for m in net:
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(LEARNED_LINEAR_GAIN)
                    m.bias.mul_(LEARNED_LINEAR_GAIN)
                elif isinstance(m, torch.nn.LayerNorm):
                    m.weight.fill_(LEARNED_LAYERNORM_WEIGHT)
        init["net"] = copy.deepcopy(net.state_dict())
    n_seq = 1 if segments else K
    if segments:
        assert T % segments == 0 and K == T // segments
    obs = dense_observations(kind, shapes, n_seq, gen)
    target = torch.rand(T, B, H, generator=gen) * 1.6 - 0.8
    if kind[0] == "learned":
        noise = [gumbel((T, B, N), gen) for _ in range(n_seq)]
    r32 = _dense_run(kind, shapes, K, opt, init, obs, target, noise, torch.float32, segments)
    r64 = _dense_run(kind, shapes, K, opt, init, obs, target, noise, torch.float64, segments)
    targets = [target[k * segments:(k + 1) * segments] for k in range(K)] if segments else [target] * K
    param_atol, belief_atol, loss_atol = _bounds(r32, r64, opt, targets)
    move, stale = _sensitivity(r64, param_atol, belief_atol)
    tr = types.SimpleNamespace(kind=kind, shapes=shapes, K=K, opt=opt, segments=segments, whole=not segments, init=init, obs=obs,
                               target=target, targets=targets, noise=noise, r32=r32, r64=r64, param_atol=param_atol,
                               belief_atol=belief_atol, loss_atol=loss_atol, move=move, stale=stale)
    if kind[0] == "learned":
        tr.same_edges = all(torch.equal(a, b) for ka, kb in zip(r32.adjs, r64.adjs) for a, b in zip(ka, kb))
        tr.gap, tr.cut = r64.gap, r64.cut
    _cache[key] = tr
    return tr


# ---------------------------------------------------------------------------------------------------------
# SparseGCM: TemporalEdge hops, GraphConv x 2, one-shot calls or one node per call
# ---------------------------------------------------------------------------------------------------------
def _sparse_run(shapes, hops, act, K, opt, init, obs, target, dtype, stepwise, split, loss_kind):
    B, N, F, H, ts = shapes
    gnn = osp.canonical_gnn(F, H, act=act)
    gnn.load_state_dict(init)
    gnn = gnn.to(dtype)
    stale_gnn = copy.deepcopy(gnn)
    params = dict(gnn.named_parameters())
    optimizer = make_optimizer(opt, list(params.values()))
    cuts = [0, ts] if not split else [0, split, ts]
    r = types.SimpleNamespace(losses=[], beliefs=[], params=[], grads=[], stale=[], hidden=None,
                              p0={k: p.detach().clone() for k, p in params.items()})

    def run(g, x, hidden):
        """x [B, t, F] -> beliefs [B, t, H]"""
        sel = osp.TemporalEdge(hops)
        fn = lambda a, b, c: g(a, b, c)
        if not stepwise:
            return osp.sparse_step(x, torch.full((B,), x.shape[1], dtype=torch.long), hidden, fn, graph_size=N,
                                   edge_selectors=sel)
        outs = []
        for t in range(x.shape[1]):
            o, hidden = osp.sparse_step(x[:, t:t + 1], torch.ones(B, dtype=torch.long), hidden, fn, graph_size=N,
                                        edge_selectors=sel)
            outs.append(o)
        return torch.cat(outs, dim=1), hidden

    first = True
    for k in range(K):
        hidden = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            x, tgt = obs[k][:, a:b].to(dtype), target[:, a:b].to(dtype)
            if hidden is not None:
                hidden = tuple(h.detach() for h in hidden)
            h_in = hidden
            if hidden is None:     # (the oracle's zero state is float32: osp.initial_hidden)
                n0, a0, T0 = osp.initial_hidden(x, N)
                h_in = (n0.to(dtype), a0.to(dtype), T0)
            if not first and dtype == torch.float64:
                with torch.no_grad():
                    so, _ = run(stale_gnn, x, h_in)
                r.stale.append(so)
            first = False
            optimizer.zero_grad(set_to_none=True)
            out, hidden = run(gnn, x, h_in)
            loss = ((out - tgt) ** 2).mean() if loss_kind == "mse" else out.mean()
            loss.backward()
            stale_gnn.load_state_dict(gnn.state_dict())
            optimizer.step()
            r.losses.append(float(loss.detach()))
            r.beliefs.append(out.detach())
            r.grads.append({n: p.grad.detach().clone() for n, p in params.items()})
            r.params.append({n: p.detach().clone() for n, p in params.items()})
    r.hidden = tuple(h.detach() for h in hidden)
    return r


def sparse_trajectory(shapes, hops, act, K, opt, seed, stepwise=False, split=None, loss="mse"):
    """oracle/sparse.py::sparse_step through K iterations of fresh observations obs[k] [B, ts, F] from
    hidden = None, float32 and float64.  stepwise: one node per call (t_pad = 1); split=s: an optimiser step
    also after the first s nodes of every iteration, on the kept, detached hidden state (two steps per
    iteration: the records of r32 / r64 are per optimiser step).  loss="mean": out.mean(), the reference tests'
    loss, instead of the squared distance to the target.  Same namespace as oracle_trajectory."""
    key = ("sparse", tuple(shapes), tuple(hops), act, K, tuple(opt), seed, stepwise, split, loss)
    if key in _cache:
        return _cache[key]
    B, N, F, H, ts = shapes
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    init = copy.deepcopy(osp.canonical_gnn(F, H, act=act).state_dict())
    obs = [torch.rand(B, ts, F, generator=gen) - 0.5 for _ in range(K)]
    target = torch.rand(B, ts, H, generator=gen) * 1.6 - 0.8
    r32 = _sparse_run(shapes, hops, act, K, opt, init, obs, target, torch.float32, stepwise, split, loss)
    r64 = _sparse_run(shapes, hops, act, K, opt, init, obs, target, torch.float64, stepwise, split, loss)
    cuts = [0, ts] if not split else [0, split, ts]
    targets = [target[:, a:b] for _ in range(K) for a, b in zip(cuts[:-1], cuts[1:])]
    param_atol, belief_atol, loss_atol = _bounds(r32, r64, opt, targets if loss == "mse" else None)
    move, stale = _sensitivity(r64, param_atol, belief_atol)
    tr = types.SimpleNamespace(shapes=shapes, hops=hops, K=K, opt=opt, whole=not split, init=init, obs=obs, target=target,
                               targets=targets, cuts=cuts, r32=r32, r64=r64, param_atol=param_atol,
                               belief_atol=belief_atol, loss_atol=loss_atol, move=move, stale=stale)
    _cache[key] = tr
    return tr


# ---------------------------------------------------------------------------------------------------------
# the reference's test_dense_learn: beliefs fed back as observations from a prefilled state, loss = norm
# ---------------------------------------------------------------------------------------------------------
def dense_learn_state(B, N, F):
    """The reference test's state: arange nodes, zero adjacency, no stored node yet."""
    nodes = torch.arange(B * N * F, dtype=torch.float).reshape(B, N, F)
    return nodes, torch.zeros(B, N, N), torch.zeros(0), torch.zeros(B, dtype=torch.long)


def oracle_dense_learn(B, N, F, T, iters, opt, seed):
    """-> (initial state dict of the two-layer DenseGraphConv + Tanh GNN, the oracle's float32 losses)."""
    torch.manual_seed(seed)
    gnn = od.canonical_gnn(F, F)
    init = copy.deepcopy(gnn.state_dict())
    optimizer = make_optimizer(opt, list(gnn.parameters()))
    sel = od.TemporalBackedge([1])
    losses = []
    for _ in range(iters):
        optimizer.zero_grad()
        obs, hidden = torch.ones(B, F), dense_learn_state(B, N, F)
        for _t in range(T):
            obs, hidden = od.dense_step(obs, hidden, gnn, graph_size=N, edge_selectors=sel)
        loss = torch.norm(obs)
        loss.backward()
        optimizer.step()
        losses.append(float(loss))
    return init, losses
