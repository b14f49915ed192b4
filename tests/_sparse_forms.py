"""Helpers of tests/test_sparse_forms_cpu.py / test_sparse_forms_gpu.py: the two-layer GraphConv stack of SparseGCM in
every activation / bias form the sparse path takes as run-time arguments (act1, act2, has_b1, has_b2 of
sparse_temporal_step, gcm_sparse_step_cached, gcm_csr_graphconv_fwd / _fwd_checked / _bwd and the chain's
gcm_dense_rows_bptt_cached), on the smallest shapes that reach each CSR kernel family, against the CPU oracle
(oracle/sparse.py) in float32 and float64.

Forms, margins, floors and the neighbouring wrong forms are the ones of tests/_forms.py (imported, not copied).  Every
(case, form) has ONE oracle trajectory (`trajectory`, cached) that all drivers of the GPU test share, and a seed (SEEDS,
found by tools/search_form_seeds.py --sparse) under which the comparison means something - `preconditions`, computed
from the oracle alone:

1. ReLU margin.  The outputs of every conv that a ReLU follows, all flat rows of every call: the smallest
   |pre-activation| of the float64 run is >= RELU_MARGIN x the largest float32 - float64 difference on the same entries,
   and no sign differs.
2. Sensitivity.  The float64 beliefs of the same weights under every neighbouring wrong form (_forms.wrong_forms: the
   activations swapped, either one replaced, a present bias dropped) are >= SENSITIVITY x the belief atol away.
3. `learned`: the float32 and float64 oracles select the same edges in every call, the smallest distance in
   (logit + noise) / tau between a chosen candidate and the best one not chosen in its row and the smallest
   |log softmax - log cutoff| over all candidates are >= DECISION_MARGIN.

Bounds (loss = sum(out * w) over all calls): beliefs of a call  max(FACTOR x |out32 - out64|, BELIEF_FLOOR) over that
call; a gradient  max(FACTOR x |g32 - g64|, GRAD_FLOOR x max|g64|); the edge network's tensors share one gradient scale
and _forms.LEARNED_NET_FLOOR.  The belief atol of the sensitivity condition is the largest of the calls'."""
import copy
import math
import types

import torch

from _forms import (ACTS, FORMS, LEARNED_FORMS, RELU_MARGIN, SEARCH_MARGIN, SENSITIVITY, DECISION_MARGIN,  # noqa: F401
                    BELIEF_FLOOR, GRAD_FLOOR, FACTOR, LEARNED_NET_FLOOR, form_id, wrong_forms, convs_of)
import _training as tr
from oracle import dense as od
from oracle import pyg
from oracle import sparse as osp

# name: shape (B, N, F, H1, H2); TemporalEdge hops (strictly descending: the closed-form structure kernel) or the
# LearnedEdge options; the calls - "taus": one row of valid lengths per call (x [B, max(row), F], zero padded),
# "chain": (T, p) = T calls of x [B, 1, F] in which a graph gets no node with probability p.
CASES = {
    "oneshot": dict(shape=(4, 16, 32, 32, 32), hops=[4, 2, 1], taus=[[16] * 4]),
    "oneshot64": dict(shape=(5, 16, 32, 32, 64), hops=[3, 1], taus=[[16] * 5]),
    "two_calls": dict(shape=(5, 24, 20, 48, 24), hops=[5, 2], taus=[[12, 7, 0, 12, 9], [10, 3, 10, 0, 8]], x_grad=True),
    "wide": dict(shape=(3, 12, 96, 128, 40), hops=[2, 1], taus=[[12, 5, 9]]),
    "chain": dict(shape=(4, 12, 32, 32, 32), hops=[3, 1], chain=(12, 0.2)),
    "chain64": dict(shape=(3, 10, 64, 64, 16), hops=[2], chain=(10, 0.0)),
    "khop": dict(shape=(4, 16, 32, 32, 32), hops=[4, 2, 1], taus=[[16] * 4], max_hops=2),
    # window / num_edge_samples of tests/golden/g12_sparse_learned_win3
    "learned": dict(shape=(4, 16, 32, 32, 32), learned=dict(window=3, k=3), taus=[[8] * 4, [8] * 4]),
}


def forms_of(case):
    return LEARNED_FORMS if case == "learned" else FORMS


def pairs():
    return [(case, form) for case in CASES for form in forms_of(case)]


# (case, form id) -> seed: the smallest seed in range(32) that meets every precondition with the ReLU ratio at
# SEARCH_MARGIN - the table tools/search_form_seeds.py --sparse prints.  Seed 0 serves all but these:
_SEEDS_NOT_0 = {
    ("oneshot", "relu-none-b1"): 1, ("oneshot", "relu-relu-b3"): 1, ("wide", "relu-none-b1"): 1,
    ("wide", "relu-relu-b3"): 1, ("khop", "relu-none-b1"): 1, ("khop", "relu-relu-b3"): 1,
}
SEEDS = {(case, form_id(form)): _SEEDS_NOT_0.get((case, form_id(form)), 0) for case, form in pairs()}


def build_gnn(fin, h1, h2, form, conv_cls=pyg.GraphConv, seq_cls=pyg.Sequential):
    """The two-layer stack of `form` - from the oracle's classes, or from gcm.nn's (same state_dict keys).  A missing
    bias is no tensor (bias=False), a missing activation no module."""
    a1, a2, mask = form
    mods = []
    for cin, cout, act, bit in ((fin, h1, a1, 1), (h1, h2, a2, 2)):
        mods.append((conv_cls(cin, cout, bias=bool(mask & bit)), "x, edges, weights -> x"))
        if ACTS[act] is not None:
            mods.append(ACTS[act]())
    return seq_cls("x, edges, weights", mods)


def call_taus(case, gen):
    """[taus [B] per call].  `chain`: a call in which no graph would get a node gives graph 0 one (the oracle, like the
    reference, takes no call without a new node)."""
    c = CASES[case]
    if "chain" not in c:
        return [torch.tensor(row, dtype=torch.long) for row in c["taus"]]
    T, p = c["chain"]
    taus = (torch.rand(T, c["shape"][0], generator=gen) >= p).long()
    taus[taus.sum(dim=1) == 0, 0] = 1
    return list(taus)


class _WatchedLearnedEdge(osp.LearnedEdge):
    """osp.LearnedEdge that records how far its decisions (softmax > 1 / (1 + k) over each new node's candidates) are
    from flipping: `gap` - the smallest distance in (logit + noise) / tau between a chosen candidate and the best one
    not chosen in its row - and `cut` - the smallest |log softmax - log cutoff| over all candidates."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.gap, self.cut = math.inf, math.inf

    def __call__(self, nodes, T, taus, B):
        if int((T + taus).max()) > 1:
            with torch.no_grad():
                idx = osp.get_causal_edges(T, taus, self.window)      # (coalesced order: the draws line up)
                b, sink, src = idx.unbind()
                z = self.net(torch.cat((nodes[b, sink], nodes[b, src]), dim=-1)).squeeze(-1)
                z = (z + self.noise_fn(z.numel())) / self.tau
                row = b * nodes.shape[1] + sink
                cutoff = 1.0 / (1 + self.k)
                for r in row.unique():
                    zr = z[row == r]
                    soft = torch.softmax(zr, dim=0)
                    chosen = soft > cutoff
                    if bool(chosen.any()) and bool((~chosen).any()):
                        self.gap = min(self.gap, float(zr[chosen].min() - zr[~chosen].max()))
                    self.cut = min(self.cut, float((soft.log() - math.log(cutoff)).abs().min()))
        return super().__call__(nodes, T, taus, B)


def inputs(case, form, seed):
    """Initial parameters (default initialisation under `seed`; the edge network as tests/_training.py's LEARNED_*
    constants make it), the calls [(x [B, t, F] uniform in [-1, 1), zero behind taus; taus [B])], loss weights
    [B, t, H2] per call, gumbel draws per call (one per candidate pair, in candidate order)."""
    c = CASES[case]
    B, N, Fin, H1, H2 = c["shape"]
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    inp = types.SimpleNamespace(case=case, form=form, seed=seed, net=None, noise=None)
    inp.gnn = copy.deepcopy(build_gnn(Fin, H1, H2, form).state_dict())
    if "learned" in c:
        net = od.build_edge_network(Fin)
        with torch.no_grad():
            for m in net:
                if isinstance(m, torch.nn.Linear):
                    m.weight.mul_(tr.LEARNED_LINEAR_GAIN)
                    m.bias.mul_(tr.LEARNED_LINEAR_GAIN)
                elif isinstance(m, torch.nn.LayerNorm):
                    m.weight.fill_(tr.LEARNED_LAYERNORM_WEIGHT)
        inp.net = copy.deepcopy(net.state_dict())
    inp.calls, inp.w = [], []
    for taus in call_taus(case, gen):
        t = int(taus.max())
        x = torch.rand(B, t, Fin, generator=gen) * 2 - 1
        x = x * (torch.arange(t)[None, :] < taus[:, None])[:, :, None]
        inp.calls.append((x, taus))
    for x, _ in inp.calls:
        inp.w.append(torch.rand(B, x.shape[1], H2, generator=gen))
    if "learned" in c:
        inp.noise, T = [], torch.zeros(B, dtype=torch.long)
        for _, taus in inp.calls:
            n = osp.get_causal_edges(T, taus, c["learned"]["window"]).shape[1]
            inp.noise.append(tr.gumbel((n,), gen))
            T = T + taus
    return inp


def _modules(inp, form=None, dtype=torch.float32):
    """Oracle modules holding inp's parameters, as `form` (default: the form they were made for; another one: the same
    weights, a bias that `form` lacks dropped)."""
    B, N, Fin, H1, H2 = CASES[inp.case]["shape"]
    base = build_gnn(Fin, H1, H2, inp.form)
    base.load_state_dict(inp.gnn)
    gnn = base
    if form is not None and form != inp.form:
        gnn = build_gnn(Fin, H1, H2, form)
        with torch.no_grad():
            for src, dst in zip(convs_of(base), convs_of(gnn)):
                dst.lin_rel.weight.copy_(src.lin_rel.weight)
                dst.lin_root.weight.copy_(src.lin_root.weight)
                if dst.lin_rel.bias is not None:
                    dst.lin_rel.bias.copy_(src.lin_rel.bias)
    net = None
    if inp.net is not None:
        net = od.build_edge_network(Fin)
        net.load_state_dict(inp.net)
        net = net.to(dtype)
    return gnn.to(dtype), net


def _run(inp, dtype, form=None, grad=False):
    """The oracle's calls from empty graphs.  -> namespace: outs [[B, t, H2] per call], hidden (nodes, coalesced adj,
    T), pre ({layer: the outputs of a conv that a ReLU follows, all flat rows of every call, flat}), rows (flat rows
    the GNN saw, summed over the calls), edges (the stored COO indices behind every call), gap / cut of the selector's
    decisions, and with grad (loss = sum(out * w) over all calls) grads {name: gradient}: the GNN's parameters, "x<i>"
    for call i's observations where the case asks for them, the edge network under "net."."""
    c = CASES[inp.case]
    B, N, Fin, H1, H2 = c["shape"]
    gnn, net = _modules(inp, form, dtype)
    form = form or inp.form
    store, handles, rows = {}, [], []
    convs = convs_of(gnn)
    handles.append(convs[0].register_forward_hook(lambda m, a, out: rows.append(out.shape[0])))
    for i, (conv, act) in enumerate(zip(convs, form[:2])):
        if act == "relu":
            store[i] = []
            handles.append(conv.register_forward_hook(
                lambda m, a, out, i=i: store[i].append(out.detach().reshape(-1).clone())))
    step = {"call": 0}
    if "learned" in c:
        sel = _WatchedLearnedEdge(net, c["learned"]["k"], window=c["learned"]["window"],
                                  noise_fn=lambda n: inp.noise[step["call"]][:n].to(dtype))
    else:
        sel = osp.TemporalEdge(c["hops"])
    r = types.SimpleNamespace(outs=[], edges=[], gap=math.inf, cut=math.inf)
    n0, a0, T0 = osp.initial_hidden(inp.calls[0][0], N)      # (the oracle's zero state is float32)
    hidden = (n0.to(dtype), a0.to(dtype), T0)
    xs = [x.detach().clone().to(dtype).requires_grad_(bool(grad and c.get("x_grad"))) for x, _ in inp.calls]
    with torch.set_grad_enabled(grad):
        loss = 0.0
        for i, (_, taus) in enumerate(inp.calls):
            step["call"] = i
            out, hidden = osp.sparse_step(xs[i], taus, hidden, gnn, graph_size=N, edge_selectors=sel,
                                          max_hops=c.get("max_hops"))
            r.outs.append(out.detach())
            r.edges.append(hidden[1].coalesce().indices().clone())
            loss = loss + (out * inp.w[i].to(dtype)).sum()
        if grad:
            loss.backward()
            r.grads = {k: p.grad for k, p in gnn.named_parameters()}
            if c.get("x_grad"):
                r.grads.update({"x%d" % i: x.grad for i, x in enumerate(xs)})
            if net is not None:
                r.grads.update({"net." + k: p.grad for k, p in net.named_parameters()})
    for h in handles:
        h.remove()
    r.hidden = (hidden[0].detach(), hidden[1].detach().coalesce(), hidden[2])
    r.pre = {i: torch.cat(v) for i, v in store.items()}
    r.rows = sum(rows)
    if isinstance(sel, _WatchedLearnedEdge):
        r.gap, r.cut = sel.gap, sel.cut
    return r


def belief_atols(r32, r64):
    """Per call: max(FACTOR x the float32 oracle's distance from float64, BELIEF_FLOOR)."""
    return [max(BELIEF_FLOOR, FACTOR * float((a.double() - b).abs().max())) for a, b in zip(r32.outs, r64.outs)]


def preconditions(case, form, seed, inp=None, grad=False):
    """What must hold of the oracle's own runs for a comparison under `seed` to mean something (module docstring).
    -> namespace: n_pre, relu_ratio (inf without a ReLU), signs_equal, belief_atol (the largest of the calls'), sens
    {wrong form: distance / atol}, gap / cut / same_edges (learned), inp, r32 / r64 (the two runs; grad: with gradients)."""
    inp = inp or inputs(case, form, seed)
    r32, r64 = _run(inp, torch.float32, grad=grad), _run(inp, torch.float64, grad=grad)
    p = types.SimpleNamespace(case=case, form=form, seed=seed, n_pre=0, relu_ratio=math.inf, signs_equal=True)
    for i, v64 in r64.pre.items():
        v32 = r32.pre[i].double()
        p.n_pre += v64.numel()
        err = float((v32 - v64).abs().max())
        p.relu_ratio = min(p.relu_ratio, float(v64.abs().min()) / max(err, 1e-300))
        p.signs_equal = p.signs_equal and bool(((v32 > 0) == (v64 > 0)).all())
    p.belief_atol = max(belief_atols(r32, r64))
    p.sens = {}
    for name, (wf, _) in wrong_forms(form).items():
        wrong = _run(inp, torch.float64, form=wf)
        p.sens[name] = max(float((a - b).abs().max()) for a, b in zip(wrong.outs, r64.outs)) / p.belief_atol
    p.gap, p.cut = min(r32.gap, r64.gap), min(r32.cut, r64.cut)
    p.same_edges = all(torch.equal(a, b) for a, b in zip(r32.edges, r64.edges))
    p.inp, p.r32, p.r64 = inp, r32, r64
    return p


def failures(p, relu_margin=RELU_MARGIN):
    """The preconditions `p` does not meet (empty: all hold)."""
    bad = []
    if not (p.signs_equal and p.relu_ratio >= relu_margin):
        bad.append(("relu margin", p.relu_ratio, p.signs_equal, p.n_pre))
    for name, ratio in p.sens.items():
        if not ratio >= SENSITIVITY:
            bad.append(("beliefs under the wrong form too close", name, ratio))
    if "learned" in CASES[p.case] and not (p.same_edges and p.gap >= DECISION_MARGIN and p.cut >= DECISION_MARGIN):
        bad.append(("learned decision margin", p.gap, p.cut, p.same_edges))
    return bad


def assert_preconditions(p):
    bad = failures(p)
    assert not bad, (p.case, form_id(p.form), p.seed, bad)


_cache = {}


def trajectory(case, form):
    """The oracle's trajectory of (case, form) under its seed, once per process: inputs, preconditions (`pre`), the
    float32 state (`hidden`: nodes, coalesced adj, T), the float64 beliefs per call with their atols, and `bounds`
    {name: (float64 gradient, atol)} - the GNN's parameter names as the product's module has them, "x<i>" for the
    observations of call i, "net." for the edge network."""
    key = (case, form)
    if key in _cache:
        return _cache[key]
    seed = SEEDS[(case, form_id(form))]
    inp = inputs(case, form, seed)
    t = types.SimpleNamespace(case=case, form=form, seed=seed, inp=inp, shape=CASES[case]["shape"],
                              pre=preconditions(case, form, seed, inp, grad=True))
    r32, r64 = t.pre.r32, t.pre.r64
    t.hidden, t.out64, t.out_atol = r32.hidden, r64.outs, belief_atols(r32, r64)
    # (the edge network's tensors share one gradient scale and the floor of test_learned_fused_gpu._check_learned_grads:
    #  two of its biases have an analytically zero gradient - tests/_training.zero_gradient)
    net_scale = max([float(g.abs().max()) for k, g in r64.grads.items() if k.startswith("net.")] or [0.0])
    t.bounds = {}
    for k, g64 in r64.grads.items():
        assert g64 is not None and r32.grads[k] is not None, k
        err = float((r32.grads[k].double() - g64).abs().max())
        floor = LEARNED_NET_FLOOR * net_scale if k.startswith("net.") else GRAD_FLOOR * float(g64.abs().max())
        assert floor > 0, k
        t.bounds[k] = (g64, max(FACTOR * err, floor))
    _cache[key] = t
    return t
