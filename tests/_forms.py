"""Helpers of tests/test_step_forms_cpu.py / test_step_forms_gpu.py: the two-layer DenseGraphConv stack in every
activation / bias form the fused DenseGCM kernels take as run-time arguments (act1, act2, has_bias), on the smallest
shapes that reach each kernel family, against the CPU oracle in float32 and float64.

A form is (act1, act2, bias mask): mask bit 1 = layer 1's lin_rel.bias, bit 2 = layer 2's.  Every (case, form) has ONE
oracle trajectory (`trajectory`, cached) that all drivers of the GPU test share, and a seed (SEEDS, found by
tools/search_form_seeds.py) under which the comparison means something - `preconditions`, computed from the oracle alone:

1. ReLU margin.  The outputs of every conv that a ReLU follows, on the live rows (< min(t + 1, N)) of every step: the
   smallest |pre-activation| of the float64 run is >= RELU_MARGIN x the largest float32 - float64 difference on the
   same entries, and no sign differs.  (The tolerance rule grants a kernel 3x the oracle's own fp32 error: 10 leaves
   another 3x before a kernel that is right could flip a ReLU mask and send its gradient out of any bound.)
2. Sensitivity.  The float64 beliefs of the same weights under every neighbouring WRONG form - the activations swapped,
   either one replaced, a present bias dropped, the folded preprocessor's W_root1 b_p term left out - are further than
   STALE_FACTOR x the belief atol from the right ones: a kernel that does not honour the form cannot pass.
3. Decision margins.  EuclideanEdge: every |d - max_distance| >= 1e-3; LearnedEdge: chosen-to-unchosen gap >= 1e-3
   in logit + noise and the same adjacency at every step in float32 and float64.

Bounds: tests/_golden.fp64_rollout_bounds (3x the oracle's fp32 distance from float64, floors 2e-6 on the beliefs and
5e-7 of a gradient's scale); loss = sum(out * w)."""
import copy
import math
import types

import torch

import _training as tr
from _golden import fp64_rollout_bounds
from oracle import dense as od
from oracle import pyg

RELU_MARGIN = 10.0       # asserted by the tests
SEARCH_MARGIN = 15.0     # what tools/search_form_seeds.py asks for (float32 CPU BLAS differs between hosts)
SENSITIVITY = tr.STALE_FACTOR
DECISION_MARGIN = 1e-3
BELIEF_FLOOR, GRAD_FLOOR, FACTOR = tr.BELIEF_FLOOR, tr.GRAD_FLOOR, tr.FACTOR
LEARNED_NET_FLOOR = 2e-6     # test_learned_fused_gpu._check_learned_grads: the edge network's common scale

ACTS = {"none": None, "tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}

FORMS = [("none", "none", 0), ("none", "tanh", 1), ("none", "relu", 2), ("tanh", "none", 2), ("tanh", "relu", 0),
         ("relu", "none", 1), ("relu", "tanh", 0), ("relu", "relu", 3), ("tanh", "tanh", 0), ("tanh", "tanh", 1),
         ("tanh", "tanh", 2)]
LEARNED_FORMS = [("relu", "relu", 3), ("none", "tanh", 0), ("tanh", "none", 1), ("relu", "none", 2)]

# name: selector, (B, N, F, H1, H2, T) - T = N + 8 (N + 4 for `ragged` and `fold`): the chain leaves its fill phase.
# "pre": width of the Linear preprocessor's output (the GNN's input)
CASES = {
    "temporal": dict(sel=("temporal", [1, 2, 4], "forward"), shape=(3, 16, 32, 32, 32, 24)),
    "padded": dict(sel=("temporal", [2, 5], "forward"), shape=(3, 24, 20, 48, 24, 32)),
    "wide": dict(sel=("temporal", [1, 3], "forward"), shape=(3, 20, 64, 64, 16, 28)),
    "dense8": dict(sel=("dense",), shape=(3, 16, 32, 32, 32, 24)),
    "both4": dict(sel=("temporal", [1, 3], "both"), shape=(3, 16, 64, 64, 40, 24)),
    "euclid": dict(sel=("euclid", 3.0), shape=(32, 16, 32, 32, 32, 24)),
    "ragged": dict(sel=("temporal", [1, 2], "forward"), shape=(3, 10, 6, 12, 10, 14)),
    "obs_grad": dict(sel=("temporal", [1, 2, 4], "forward"), shape=(3, 16, 32, 32, 32, 24), obs_grad=True),
    "fold": dict(sel=("temporal", [1, 2], "forward"), shape=(3, 12, 8, 32, 32, 16), pre=32),
    "learned": dict(sel=("learned", 3), shape=(6, 16, 32, 32, 32, 24)),
}


def form_id(form):
    return "%s-%s-b%d" % form


def forms_of(case):
    return LEARNED_FORMS if case == "learned" else FORMS


def pairs():
    return [(case, form) for case in CASES for form in forms_of(case)]


# (case, form id) -> seed: the smallest seed in range(32) that meets every precondition with the ReLU ratio at
# SEARCH_MARGIN - the table tools/search_form_seeds.py prints.  Seed 0 serves all but these:
_SEEDS_NOT_0 = {
    ("temporal", "tanh-relu-b0"): 1, ("dense8", "tanh-relu-b0"): 1, ("dense8", "relu-tanh-b0"): 2,
    ("dense8", "relu-relu-b3"): 1, ("both4", "relu-relu-b3"): 1, ("euclid", "none-relu-b2"): 3,
    ("euclid", "relu-none-b1"): 1, ("euclid", "relu-tanh-b0"): 3, ("euclid", "relu-relu-b3"): 1,
    ("obs_grad", "tanh-relu-b0"): 1,
}
SEEDS = {(case, form_id(form)): _SEEDS_NOT_0.get((case, form_id(form)), 0) for case, form in pairs()}


def build_gnn(fin, h1, h2, form, conv_cls=pyg.DenseGraphConv, seq_cls=pyg.Sequential):
    """The two-layer stack of `form` - from the oracle's classes, or from gcm.nn's (same state_dict keys)."""
    a1, a2, mask = form
    mods = []
    for cin, cout, act, bit in ((fin, h1, a1, 1), (h1, h2, a2, 2)):
        mods.append((conv_cls(cin, cout, bias=bool(mask & bit)), "x, adj -> x"))
        if ACTS[act] is not None:
            mods.append(ACTS[act]())
    return seq_cls("x, adj, weights, B, N", mods)


def convs_of(gnn):
    return [m for m in gnn.modules() if hasattr(m, "lin_rel")]


class PreGnn(torch.nn.Module):
    """Linear preprocessor + GNN as ONE module in the place of the oracle's `gnn`: index-writing selectors do not read
    the nodes, so gnn(pre(dirty)) is od.dense_step(..., preprocessor=pre) - in a shape fp64_rollout_bounds takes."""

    def __init__(self, pre, gnn):
        super().__init__()
        self.pre, self.gnn = pre, gnn

    def forward(self, x, adj, weights, B, N):
        return self.gnn(self.pre(x), adj, weights, B, N)


class _WatchedEuclid(od.EuclideanEdge):
    """od.EuclideanEdge that records how far its decisions are from flipping: min |d - max_distance| over the
    candidates (j < num_nodes)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.margin = math.inf

    def __call__(self, nodes, adj, weights, num_nodes, B):
        with torch.no_grad():
            d = self.distances(nodes, num_nodes)
            ok = torch.arange(nodes.shape[1])[None, :] < num_nodes[:, None]
            if bool(ok.any()):
                self.margin = min(self.margin, float((d[ok] - self.max_distance).abs().min()))
        return super().__call__(nodes, adj, weights, num_nodes, B)


def inputs(case, form, seed):
    """Initial parameters (default initialisation under `seed`), observations, loss weights, gumbel draws."""
    c = CASES[case]
    B, N, F, H1, H2, T = c["shape"]
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    fin = c.get("pre", F)
    inp = types.SimpleNamespace(case=case, form=form, seed=seed, pre=None, net=None, noise=None)
    inp.gnn = copy.deepcopy(build_gnn(fin, H1, H2, form).state_dict())
    if "pre" in c:
        inp.pre = copy.deepcopy(torch.nn.Linear(F, fin, bias=True).state_dict())
    kind = c["sel"]
    if kind[0] == "learned":      # the edge network of tests/_training.py (LEARNED_*: livelier logits)
        net = od.build_edge_network(F)
        with torch.no_grad():
            for m in net:
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(tr.LEARNED_LINEAR_GAIN)
                    m.bias.mul_(tr.LEARNED_LINEAR_GAIN)
                elif isinstance(m, torch.nn.LayerNorm):
                    m.weight.fill_(tr.LEARNED_LAYERNORM_WEIGHT)
        inp.net = copy.deepcopy(net.state_dict())
    inp.obs = tr.dense_observations(kind, (B, N, F, H1, T), 1, gen)[0]
    inp.w = torch.rand(T, B, H2, generator=gen)
    if kind[0] == "learned":
        inp.noise = tr.gumbel((T, B, N), gen)
    return inp


def _modules(inp, form=None, dtype=torch.float32):
    """Oracle modules holding inp's parameters, as `form` (default: the form they were made for; another one: the same
    weights, a bias that `form` lacks dropped)."""
    c = CASES[inp.case]
    B, N, F, H1, H2, T = c["shape"]
    fin = c.get("pre", F)
    base = build_gnn(fin, H1, H2, inp.form)
    base.load_state_dict(inp.gnn)
    gnn = base
    if form is not None and form != inp.form:
        gnn = build_gnn(fin, H1, H2, form)
        with torch.no_grad():
            for src, dst in zip(convs_of(base), convs_of(gnn)):
                dst.lin_rel.weight.copy_(src.lin_rel.weight)
                dst.lin_root.weight.copy_(src.lin_root.weight)
                if dst.lin_rel.bias is not None:
                    dst.lin_rel.bias.copy_(src.lin_rel.bias)
    pre = net = None
    if inp.pre is not None:
        pre = torch.nn.Linear(F, fin, bias=True)
        pre.load_state_dict(inp.pre)
        pre = pre.to(dtype)
    if inp.net is not None:
        net = od.build_edge_network(F)
        net.load_state_dict(inp.net)
        net = net.to(dtype)
    return gnn.to(dtype), pre, net


def _selector(inp, dtype, net, step):
    kind = CASES[inp.case]["sel"]
    if kind[0] == "temporal":
        return od.TemporalBackedge(kind[1], kind[2])
    if kind[0] == "dense":
        return od.DenseEdge()
    if kind[0] == "euclid":
        return _WatchedEuclid(kind[1])
    nf = lambda shape: inp.noise[step["t"]][:, : shape[1]].to(dtype)
    return tr._WatchedLearnedEdge(net, num_edge_samples=kind[1], noise_fn=nf)


def _rollout(inp, dtype, form=None, drop_root_bp=False, grad=False, obs_grad=False):
    """The oracle's per-step loop from hidden = None.  -> namespace: out [T, B, H2], hidden, pre ({layer: the outputs of
    a conv that a ReLU follows, live rows of every step, flat}), adjs, margin / gap of the selector's decisions, and
    with grad (loss = sum(out * w)) grads {name: gradient} (edge network under "net."; obs_grad: the observations'
    under "obs")."""
    c = CASES[inp.case]
    B, N, F, H1, H2, T = c["shape"]
    gnn, pre, net = _modules(inp, form, dtype)
    form = form or inp.form
    convs = convs_of(gnn)
    if drop_root_bp:      # layer 1 without W_root1 b_p: every row of its input is W_p x + b_p
        conv, b_p = convs[0], pre.bias.detach()
        conv.forward = lambda x, adj, mask=None: conv.lin_rel(torch.matmul(adj, x)) + conv.lin_root(x - b_p)
    store, handles = {}, []
    for i, (conv, act) in enumerate(zip(convs, form[:2])):
        if act == "relu":
            store[i] = []
            handles.append(conv.register_forward_hook(
                lambda m, a, out, i=i: store[i].append(out.detach()[:, : min(len(store[i]) + 1, N)].reshape(-1).clone())))
    step = {"t": 0}
    sel = _selector(inp, dtype, net, step)
    r = types.SimpleNamespace(adjs=[], margin=math.inf, gap=math.inf)
    hidden, outs = None, []
    obs = inp.obs.to(dtype, copy=True).requires_grad_(bool(grad and obs_grad))
    with torch.set_grad_enabled(grad):
        for t in range(T):
            step["t"] = t
            mx, hidden = od.dense_step(obs[t], hidden, gnn, graph_size=N, edge_selectors=sel,
                                       preprocessor=pre)
            outs.append(mx)
            r.adjs.append(hidden[1].detach() != 0)
        out = torch.stack(outs)
        if grad:
            (out * inp.w.to(dtype)).sum().backward()
            r.grads = {k: p.grad for k, p in gnn.named_parameters()}
            if net is not None:
                r.grads.update({"net." + k: p.grad for k, p in net.named_parameters()})
            if obs_grad:
                r.grads["obs"] = obs.grad
    for h in handles:
        h.remove()
    r.out, r.hidden = out.detach(), tuple(h.detach() for h in hidden)
    r.pre = {i: torch.cat(v) for i, v in store.items()}
    if isinstance(sel, _WatchedEuclid):
        r.margin = sel.margin
    if isinstance(sel, tr._WatchedLearnedEdge):
        r.gap = sel.gap
    return r


def wrong_forms(form, fold=False):
    """{name: (form, drop_root_bp)}: the neighbouring forms a kernel could run by mistake."""
    a1, a2, mask = form
    out = {}
    if a1 != a2:
        out["swapped"] = ((a2, a1, mask), False)
    for other in ACTS:
        if other != a1:
            out["act1=" + other] = ((other, a2, mask), False)
        if other != a2:
            out["act2=" + other] = ((a1, other, mask), False)
    for bit in (1, 2):
        if mask & bit:
            out["no bias %d" % bit] = ((a1, a2, mask & ~bit), False)
    if fold:
        out["no W_root1 b_p"] = (form, True)
    return out


def preconditions(case, form, seed, inp=None, grad=False, obs_grad=False):
    """What must hold of the oracle's own runs for a comparison under `seed` to mean something (module docstring).
    -> namespace: n_pre, relu_ratio (inf without a ReLU), signs_equal, belief_atol, sens {wrong form: distance / atol},
    margin (euclid), gap / same_edges (learned), r32 / r64 (the two runs; grad: with their gradients)."""
    inp = inp or inputs(case, form, seed)
    r32 = _rollout(inp, torch.float32, grad=grad, obs_grad=obs_grad)
    r64 = _rollout(inp, torch.float64, grad=grad, obs_grad=obs_grad)
    p = types.SimpleNamespace(case=case, form=form, seed=seed, n_pre=0, relu_ratio=math.inf, signs_equal=True)
    for i, v64 in r64.pre.items():
        v32 = r32.pre[i].double()
        p.n_pre += v64.numel()
        err = float((v32 - v64).abs().max())
        p.relu_ratio = min(p.relu_ratio, float(v64.abs().min()) / max(err, 1e-300))
        p.signs_equal = p.signs_equal and bool(((v32 > 0) == (v64 > 0)).all())
    p.belief_atol = max(BELIEF_FLOOR, FACTOR * float((r32.out.double() - r64.out).abs().max()))
    p.sens = {}
    for name, (wf, drop) in wrong_forms(form, fold="pre" in CASES[case]).items():
        wrong = _rollout(inp, torch.float64, form=wf, drop_root_bp=drop)
        p.sens[name] = float((wrong.out - r64.out).abs().max()) / p.belief_atol
    p.margin = min(r32.margin, r64.margin)
    p.gap = min(r32.gap, r64.gap)
    p.same_edges = all(torch.equal(a, b) for a, b in zip(r32.adjs, r64.adjs))
    p.r32, p.r64 = r32, r64
    return p


def failures(p, relu_margin=RELU_MARGIN):
    """The preconditions `p` does not meet (empty: all hold)."""
    bad = []
    if not (p.signs_equal and p.relu_ratio >= relu_margin):
        bad.append(("relu margin", p.relu_ratio, p.signs_equal, p.n_pre))
    for name, ratio in p.sens.items():
        if not ratio >= SENSITIVITY:
            bad.append(("beliefs under the wrong form too close", name, ratio))
    kind = CASES[p.case]["sel"][0]
    if kind == "euclid" and not p.margin >= DECISION_MARGIN:
        bad.append(("euclid decision margin", p.margin))
    if kind == "learned" and not (p.same_edges and p.gap >= DECISION_MARGIN):
        bad.append(("learned decision margin", p.gap, p.same_edges))
    return bad


def assert_preconditions(p):
    bad = failures(p)
    assert not bad, (p.case, form_id(p.form), p.seed, bad)


_cache = {}


def trajectory(case, form, obs_grad=None):
    """The oracle's trajectory of (case, form) under its seed, once per process: inputs, preconditions (`pre`), the
    float32 state (`hidden`: nodes, adj, weights, count), the float64 beliefs with their atol, and `bounds`
    {parameter name (| "obs"): (float64 gradient, atol)} - names as the product's modules have them ("pre." / "net."
    for the preprocessor / edge network).  obs_grad (default: what the case says): the observations take a gradient,
    so `bounds` has the "obs" entry."""
    c = CASES[case]
    obs_grad = bool(c.get("obs_grad")) if obs_grad is None else bool(obs_grad)
    key = (case, form, obs_grad)
    if key in _cache:
        return _cache[key]
    B, N, F, H1, H2, T = c["shape"]
    seed = SEEDS[(case, form_id(form))]
    inp = inputs(case, form, seed)
    t = types.SimpleNamespace(case=case, form=form, seed=seed, inp=inp, shape=c["shape"],
                              pre=preconditions(case, form, seed, inp, grad=c["sel"][0] == "learned",
                                                obs_grad=obs_grad))
    if c["sel"][0] != "learned":
        gnn, pre, _ = _modules(inp)
        ref = gnn if pre is None else PreGnn(pre, gnn)
        obs = inp.obs.clone().requires_grad_(obs_grad)
        watched = []

        def factory():
            watched.append(_selector(inp, None, None, None))
            return watched[-1]
        out32, hid32, bounds, (out64, atol) = fp64_rollout_bounds(ref, obs, None, inp.w, factory, N)
        t.hidden, t.out64, t.out_atol = tuple(h.detach() for h in hid32), out64, atol
        t.bounds = {(k[len("gnn."):] if k.startswith("gnn.") else k): v for k, v in bounds.items()}
    else:
        r32, r64 = t.pre.r32, t.pre.r64
        t.hidden, t.out64 = r32.hidden, r64.out
        t.out_atol = max(BELIEF_FLOOR, FACTOR * float((r32.out.double() - r64.out).abs().max()))
        # (the edge network's tensors share one gradient scale and the floor of _check_learned_grads: two of its
        #  biases have an analytically zero gradient - tests/_training.zero_gradient)
        net_scale = max(float(g.abs().max()) for k, g in r64.grads.items() if k.startswith("net."))
        assert net_scale > 0
        t.bounds = {}
        for k, g64 in r64.grads.items():
            err = float((r32.grads[k].double() - g64).abs().max())
            floor = LEARNED_NET_FLOOR * net_scale if k.startswith("net.") else GRAD_FLOOR * float(g64.abs().max())
            t.bounds[k] = (g64, max(FACTOR * err, floor))
    _cache[key] = t
    return t
