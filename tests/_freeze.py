"""Helpers of tests/test_freeze_cpu.py / test_freeze_conv_gpu.py / test_freeze_memory_gpu.py: every backward of this
project branches on which gradients are wanted (`ctx.needs_input_grad` in gcm/_ops.py, null pointers into the C ABI,
`packed.requires_grad()` on the memories' host path), so the tests ask for every SUBSET of them.

A call's differentiable tensors are named: "x", "adj" or "edge_weight" where the layer defines a gradient for it, and
every parameter by its state_dict name.  `subsets` enumerates what to ask for, `apply` sets a subset as requires_grad
flags BEFORE the forward (a Python autograd Function fixes needs_input_grad at forward time from these flags) - on the
product module and on its reference alike.

The second half is the table of conv layers (LAYERS) on two shapes each, built with each family's own input recipe
(tests/test_*_gpu.py, tests/_*_cases.py, tests/_pna_restate.py): weights of the family's sign convention, duplicate
edges and loops, isolated nodes, empty rows, no near ties for the weighted sparse max, dyadic inputs for PNA's var / std,
parameters moved off their init (`lively`)."""
import copy
import functools
import itertools
import types

import torch

import _aggr_restate as AG
import _gat_restate as GA
import _gatedgraph_cases as GGC
import _gcn_restate as GC
import _gin_restate as GI
import _pna_restate as PN
import _resgated_restate as RG
import _tag_cases as TC
import _transformer_restate as TR
from oracle import pyg

OUT_FLOOR, GRAD_FLOOR = 2e-6, 5e-7        # tests/_golden.py's floors, what every family's GPU test uses
INPUT_NAMES = ("x", "adj", "edge_weight")
EXHAUSTIVE_UP_TO = 6


# ---------------------------------------------------------------------------
# names, subsets, flags
# ---------------------------------------------------------------------------
def tensor_names(inputs, module):
    """The differentiable tensors of a call, inputs first (in INPUT_NAMES order), then the parameters."""
    return [k for k in INPUT_NAMES if k in inputs] + [k for k, _ in module.named_parameters()]


def is_bias(name):
    return name not in INPUT_NAMES and "bias" in name.rsplit(".", 1)[-1]


def subsets(names):
    """Tuples of names (each in the order of `names`), the full set first: all 2^k for k <= 6; otherwise the empty set,
    the full set, every singleton, every leave-one-out, {x}, {adj / edge_weight}, all parameters, biases only and
    weights only (the parameters that are no bias)."""
    names = list(names)
    k = len(names)
    if k <= EXHAUSTIVE_UP_TO:
        picks = [tuple(n for n, bit in zip(names, bits) if bit) for bits in itertools.product((1, 0), repeat=k)]
    else:
        params = [n for n in names if n not in INPUT_NAMES]
        picks = [tuple(names), ()]
        picks += [(n,) for n in names]
        picks += [tuple(m for m in names if m != n) for n in names]
        picks += [tuple(n for n in names if n == "x"), tuple(n for n in names if n in ("adj", "edge_weight")),
                  tuple(params), tuple(n for n in params if is_bias(n)), tuple(n for n in params if not is_bias(n))]
    seen, out = set(), []
    for s in picks:
        if s not in seen:
            seen.add(s)
            out.append(s)
    assert out[0] == tuple(names)
    return out


def subset_id(subset, names):
    if len(subset) == len(names):
        return "all"
    return "+".join(subset) if subset else "none"


def apply(subset, module, inputs):
    """`subset` as requires_grad flags on the parameters of `module` (in place) and on the floating `inputs` of the
    differentiable names -> the inputs as fresh leaves (detached copies; the others are passed through)."""
    subset = set(subset)
    named = dict(module.named_parameters())
    unknown = subset - set(named) - set(inputs)
    assert not unknown, unknown
    for k, p in named.items():
        p.requires_grad_(k in subset)
        p.grad = None
    out = {}
    for k, t in inputs.items():
        out[k] = t.detach().clone().requires_grad_(k in subset) if k in INPUT_NAMES else t
    return out


def grads_of(module, inputs):
    """{name: .grad} over the differentiable tensors of a call that has run its backward."""
    got = {k: inputs[k].grad for k in INPUT_NAMES if k in inputs}
    got.update({k: p.grad for k, p in module.named_parameters()})
    return got


def bound(f64, f32, out=False):
    """tests/_gcn_restate.bound with the floors every family's GPU test uses."""
    return GC.bound(f64, f32, OUT_FLOOR, False) if out else GC.bound(f64, f32, GRAD_FLOOR, True)


# ---------------------------------------------------------------------------
# the conv layers
# ---------------------------------------------------------------------------
DENSE_SHAPES = ((3, 7, 3, 5), (2, 130, 16, 12))        # (B, N, Fi, Fo): below one tile, odd widths / N past 128
SPARSE_SHAPES = ((40, 90, 3, 5), (129, 700, 16, 12))   # (M, E, Fi, Fo)
HEADS = (1, 4)                                         # attention layers: Fo = heads * C, C = (5, 3)
GATED_WIDTHS = ((3, 5), (12, 12))                      # GatedGraphConv takes no input wider than its output
PNA_TOWERS = (1, 2)                                    # (towers divide Fo)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31))


def _lively_biases(mod, gen):
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.rand(p.shape, generator=gen) - 0.5)
    return mod


def _seeded(make, gen):
    """make() under a seed of its own (module constructors draw from the global generator), global state untouched."""
    state = torch.random.get_rng_state()
    torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=gen)))
    try:
        return make()
    finally:
        torch.random.set_rng_state(state)


def _adj(gen, B, N, lo, hi, diag=False, empty_row=True):
    """Density 0.3, weights in [lo, hi); diag: a weighted diagonal (the GCN / GIN recipe), else a free one; one row
    without a neighbour."""
    adj = (torch.rand(B, N, N, generator=gen) < 0.3).float() * (torch.rand(B, N, N, generator=gen) * (hi - lo) + lo)
    if diag:
        eye = torch.eye(N).expand(B, N, N)
        adj = adj * (1 - eye) + eye * torch.rand(B, N, 1, generator=gen) * 3
    if empty_row and N > 2:
        adj[:, 1] = 0
    return adj


def _spec(name, ref, product, inputs, const, call, g, **extra):
    return types.SimpleNamespace(name=name, ref=ref, product=product, inputs=inputs, const=const, call=call, g=g,
                                 names=tensor_names(inputs, ref), **extra)


def _dense_call(**kw):
    return lambda mod, t, c: mod(t["x"], t["adj"] if "adj" in t else c["adj"], **kw)


def _sparse_call(mod, t, c):
    return mod(t["x"], c["edge_index"], t["edge_weight"]) if "edge_weight" in t else mod(t["x"], c["edge_index"])


def _loaded(make, ref):
    def product():
        conv = make()
        conv.load_state_dict(ref.state_dict())
        return conv
    return product


def _graphconv(aggr, dense, i):
    """tests/test_aggr_gpu.py: dense weights of both signs with rows summing below 1 and an empty row (max reads the
    pattern alone: adj gets no gradient); sparse: weighted_max_case (weights of both signs away from 0)."""
    from gcm import nn as G
    if dense:
        B, N, Fi, Fo = DENSE_SHAPES[i]
        gen = _gen(1, aggr == "mean", aggr == "max", i)
        cls = pyg.DenseGraphConv if aggr == "add" else functools.partial(AG.DenseGraphConvRef, aggr=aggr)
        ref = _lively_biases(_seeded(lambda: cls(Fi, Fo), gen), gen)
        x, adj = torch.randn(B, N, Fi, generator=gen), _adj(gen, B, N, -0.5, 1.5)
        inputs, const = ({"x": x}, {"adj": adj}) if aggr == "max" else ({"x": x, "adj": adj}, {})
        return _spec("DenseGraphConv-" + aggr, ref, _loaded(lambda: G.DenseGraphConv(Fi, Fo, aggr=aggr), ref), inputs,
                     const, _dense_call(), torch.randn(B, N, Fo, generator=gen))
    M, E, Fi, Fo = SPARSE_SHAPES[i]
    gen = _gen(2, aggr == "mean", aggr == "max", i)
    cls = pyg.GraphConv if aggr == "add" else functools.partial(AG.GraphConvRef, aggr=aggr)
    ref = _lively_biases(_seeded(lambda: cls(Fi, Fo), gen), gen)
    x, ei, w = AG.weighted_max_case(M, E, Fi, MAX_SEEDS[i])
    return _spec("GraphConv-" + aggr, ref, _loaded(lambda: G.GraphConv(Fi, Fo, aggr=aggr), ref),
                 {"x": x, "edge_weight": w}, {"edge_index": ei}, _sparse_call, torch.randn(M, Fo, generator=gen),
                 max_margin=AG.sparse_max_margin(x, ei, w) if aggr == "max" else None)


MAX_SEEDS = (130, 957)      # weighted_max_case seeds: no two candidates of a sparse max within 1e-5 (asserted on the CPU)


def _sage(dense, i):
    from gcm import nn as G
    if dense:
        B, N, Fi, Fo = DENSE_SHAPES[i]
        gen = _gen(3, i)
        ref = _lively_biases(_seeded(lambda: AG.DenseSAGERef(Fi, Fo), gen), gen)
        return _spec("DenseSAGEConv", ref, _loaded(lambda: G.DenseSAGEConv(Fi, Fo), ref),
                     {"x": torch.randn(B, N, Fi, generator=gen), "adj": _adj(gen, B, N, -0.5, 1.5)}, {}, _dense_call(),
                     torch.randn(B, N, Fo, generator=gen))
    M, E, Fi, Fo = SPARSE_SHAPES[i]
    gen = _gen(4, i)
    ref = _lively_biases(_seeded(lambda: AG.SAGERef(Fi, Fo), gen), gen)
    return _spec("SAGEConv", ref, _loaded(lambda: G.SAGEConv(Fi, Fo), ref), {"x": torch.randn(M, Fi, generator=gen)},
                 {"edge_index": AG.random_edges(M, E, 40 + i)}, _sparse_call, torch.randn(M, Fo, generator=gen))


def _gcn(dense, i):
    """tests/test_gcn_gpu.py: non-negative weights (the degrees are their sums), a weighted diagonal."""
    from gcm import nn as G
    if dense:
        B, N, Fi, Fo = DENSE_SHAPES[i]
        gen = _gen(5, i)
        ref = _lively_biases(_seeded(lambda: GC.DenseGCNRef(Fi, Fo), gen), gen)
        return _spec("DenseGCNConv", ref, _loaded(lambda: G.DenseGCNConv(Fi, Fo), ref),
                     {"x": torch.randn(B, N, Fi, generator=gen), "adj": _adj(gen, B, N, 0.0, 2.0, diag=True)}, {},
                     _dense_call(), torch.randn(B, N, Fo, generator=gen))
    M, E, Fi, Fo = SPARSE_SHAPES[i]
    gen = _gen(6, i)
    ref = _lively_biases(_seeded(lambda: GC.GCNRef(Fi, Fo), gen), gen)
    ei = AG.random_edges(M, E, 60 + i)
    return _spec("GCNConv", ref, _loaded(lambda: G.GCNConv(Fi, Fo), ref),
                 {"x": torch.randn(M, Fi, generator=gen), "edge_weight": torch.rand(ei.shape[1], generator=gen) + 0.5},
                 {"edge_index": ei}, _sparse_call, torch.randn(M, Fo, generator=gen))


def _gin(dense, i):
    """tests/test_gin_gpu.py's `mlp` (Tanh: no kink), train_eps."""
    from gcm import nn as G
    Fi, Fo = (DENSE_SHAPES if dense else SPARSE_SHAPES)[i][2:]
    gen = _gen(7, dense, i)
    nn = _seeded(lambda: torch.nn.Sequential(torch.nn.Linear(Fi, 2 * Fo), torch.nn.Tanh(), torch.nn.Linear(2 * Fo, Fo)),
                 gen)
    eps = (0.3, -0.4)[i]
    if dense:
        B, N = DENSE_SHAPES[i][:2]
        ref = GI.DenseGINRef(nn, eps, train_eps=True)
        return _spec("DenseGINConv", ref,
                     _loaded(lambda: G.DenseGINConv(copy.deepcopy(nn), eps=eps, train_eps=True), ref),
                     {"x": torch.randn(B, N, Fi, generator=gen), "adj": _adj(gen, B, N, 0.0, 2.0, diag=True)}, {},
                     _dense_call(), torch.randn(B, N, Fo, generator=gen))
    M, E = SPARSE_SHAPES[i][:2]
    ref = GI.GINRef(nn, eps, train_eps=True)
    return _spec("GINConv", ref, _loaded(lambda: G.GINConv(copy.deepcopy(nn), eps=eps, train_eps=True), ref),
                 {"x": torch.randn(M, Fi, generator=gen)}, {"edge_index": AG.random_edges(M, E, 70 + i)}, _sparse_call,
                 torch.randn(M, Fo, generator=gen))


def _gat(dense, i):
    """tests/test_gat_gpu.py: attention vectors N(0, 0.7), only the pattern of adj is read (values of both signs)."""
    from gcm import nn as G
    Fi, Fo = (DENSE_SHAPES if dense else SPARSE_SHAPES)[i][2:]
    H = HEADS[i]
    C = Fo // H
    gen = _gen(8, dense, i)

    def lively(ref):
        with torch.no_grad():
            ref.att_src.copy_(torch.randn(ref.att_src.shape, generator=gen) * 0.7)
            ref.att_dst.copy_(torch.randn(ref.att_dst.shape, generator=gen) * 0.7)
        return _lively_biases(ref, gen)
    if dense:
        B, N = DENSE_SHAPES[i][:2]
        ref = lively(_seeded(lambda: GA.DenseGATRef(Fi, C, heads=H), gen))
        return _spec("DenseGATConv", ref, _loaded(lambda: G.DenseGATConv(Fi, C, heads=H), ref),
                     {"x": torch.randn(B, N, Fi, generator=gen)}, {"adj": _adj(gen, B, N, -2.0, 2.0)}, _dense_call(),
                     torch.randn(B, N, Fo, generator=gen))
    M, E = SPARSE_SHAPES[i][:2]
    ref = lively(_seeded(lambda: GA.GATRef(Fi, C, heads=H), gen))
    return _spec("GATConv", ref, _loaded(lambda: G.GATConv(Fi, C, heads=H), ref),
                 {"x": torch.randn(M, Fi, generator=gen)}, {"edge_index": AG.random_edges(M, E, 80 + i)}, _sparse_call,
                 torch.randn(M, Fo, generator=gen))


def _transformer(dense, i):
    """tests/test_transformer_gpu.py: query and key weights x3, non-zero biases; beta=True."""
    from gcm import nn as G
    Fi, Fo = (DENSE_SHAPES if dense else SPARSE_SHAPES)[i][2:]
    H = HEADS[i]
    C = Fo // H
    gen = _gen(9, dense, i)

    def lively(ref):
        with torch.no_grad():
            ref.lin_query.weight.mul_(3)
            ref.lin_key.weight.mul_(3)
        return _lively_biases(ref, gen)
    if dense:
        B, N = DENSE_SHAPES[i][:2]
        ref = lively(_seeded(lambda: TR.DenseTransformerRef(Fi, C, heads=H, beta=True), gen))
        return _spec("DenseTransformerConv", ref, _loaded(lambda: G.DenseTransformerConv(Fi, C, heads=H, beta=True), ref),
                     {"x": torch.randn(B, N, Fi, generator=gen)}, {"adj": _adj(gen, B, N, -2.0, 2.0)}, _dense_call(),
                     torch.randn(B, N, Fo, generator=gen))
    M, E = SPARSE_SHAPES[i][:2]
    ref = lively(_seeded(lambda: TR.TransformerRef(Fi, C, heads=H, beta=True), gen))
    return _spec("TransformerConv", ref, _loaded(lambda: G.TransformerConv(Fi, C, heads=H, beta=True), ref),
                 {"x": torch.randn(M, Fi, generator=gen)}, {"edge_index": AG.random_edges(M, E, 90 + i)}, _sparse_call,
                 torch.randn(M, Fo, generator=gen))


def _resgated(dense, i):
    """tests/test_resgated_gpu.py: key and query weights x2, a non-zero bias; dense weights in [-2, 2]."""
    from gcm import nn as G
    Fi, Fo = (DENSE_SHAPES if dense else SPARSE_SHAPES)[i][2:]
    gen = _gen(10, dense, i)

    def lively(ref):
        with torch.no_grad():
            ref.lin_key.weight.mul_(2)
            ref.lin_query.weight.mul_(2)
            ref.bias.copy_(torch.rand(ref.bias.shape, generator=gen) - 0.5)
        return ref
    if dense:
        B, N = DENSE_SHAPES[i][:2]
        ref = lively(_seeded(lambda: RG.DenseResGatedRef(Fi, Fo), gen))
        return _spec("DenseResGatedGraphConv", ref, _loaded(lambda: G.DenseResGatedGraphConv(Fi, Fo), ref),
                     {"x": torch.randn(B, N, Fi, generator=gen), "adj": _adj(gen, B, N, -2.0, 2.0)}, {}, _dense_call(),
                     torch.randn(B, N, Fo, generator=gen))
    M, E = SPARSE_SHAPES[i][:2]
    ref = lively(_seeded(lambda: RG.ResGatedRef(Fi, Fo), gen))
    return _spec("ResGatedGraphConv", ref, _loaded(lambda: G.ResGatedGraphConv(Fi, Fo), ref),
                 {"x": torch.randn(M, Fi, generator=gen)}, {"edge_index": AG.random_edges(M, E, 100 + i)}, _sparse_call,
                 torch.randn(M, Fo, generator=gen))


def _gated(dense, i):
    """tests/_gatedgraph_cases.py's constructors on this file's shapes: two rounds, weights in [-0.5, 1.5]."""
    from gcm import nn as G
    Fi, C = GATED_WIDTHS[i]
    if dense:
        B, N = DENSE_SHAPES[i][:2]
        inp = GGC.dense_inputs((B, N, Fi, C, 2, {"weighted": True, "adj_grad": True}))
        return _spec("DenseGatedGraphConv", inp["ref"], _loaded(lambda: G.DenseGatedGraphConv(C, 2), inp["ref"]),
                     {"x": inp["x"], "adj": inp["adj"]}, {}, _dense_call(), inp["g"])
    M, E = SPARSE_SHAPES[i][:2]
    inp = GGC.sparse_inputs((M, E, Fi, C, 2, {"edge_weight": True}))
    return _spec("GatedGraphConv", inp["ref"], _loaded(lambda: G.GatedGraphConv(C, 2), inp["ref"]),
                 {"x": inp["x"], "edge_weight": inp["edge_weight"]}, {"edge_index": inp["edge_index"]}, _sparse_call,
                 inp["g"])


def _tag(dense, i):
    """tests/_tag_cases.py's constructors on this file's shapes: K = 3, non-negative weights."""
    from gcm import nn as G
    if dense:
        B, N, Fi, Fo = DENSE_SHAPES[i]
        inp = TC.dense_inputs((B, N, Fi, Fo, 3, {"weighted": True, "adj_grad": True}))
        return _spec("DenseTAGConv", inp["ref"], _loaded(lambda: G.DenseTAGConv(Fi, Fo, 3), inp["ref"]),
                     {"x": inp["x"], "adj": inp["adj"]}, {}, _dense_call(), inp["g"])
    M, E, Fi, Fo = SPARSE_SHAPES[i]
    inp = TC.sparse_inputs((M, E, Fi, Fo, 3, {"edge_weight": True}))
    return _spec("TAGConv", inp["ref"], _loaded(lambda: G.TAGConv(Fi, Fo, 3), inp["ref"]),
                 {"x": inp["x"], "edge_weight": inp["edge_weight"]}, {"edge_index": inp["edge_index"]}, _sparse_call,
                 inp["g"])


def _pna(dense, i):
    """tests/_pna_restate.py's constructors on this file's shapes: every aggregator and scaler on dyadic inputs (var /
    std) on the small shape, the generic family (sum, mean, min, max on normal inputs) on the large one."""
    from gcm import nn as G
    lists = (PN.ALL, PN.NOVAR)[i]
    T = PNA_TOWERS[i]
    if dense:
        B, N, Fi, Fo = DENSE_SHAPES[i]
        inp = PN.dense_inputs(dict(shape=(B, N, Fi, Fo, T, False), pattern="random", lists=lists, mask=False,
                                   add_loop=False, flat=False, post_layers=1, seed=PNA_SEEDS[0][i]))
        ref = inp["ref"]
        return _spec("DensePNAConv", ref, _loaded(lambda: G.DensePNAConv(deg=[1], **ref.kwargs()), ref),
                     {"x": inp["x"]}, {"adj": inp["adj"]}, _dense_call(), inp["g"],
                     violations=PN.family_violations(ref, inp["x"], inp["adj"]))
    M, E, Fi, Fo = SPARSE_SHAPES[i]
    inp = PN.sparse_inputs(dict(M=M, E=E, widths=(Fi, Fo, T, False), lists=lists, post_layers=1, seed=PNA_SEEDS[1][i]))
    ref = inp["ref"]
    return _spec("PNAConv", ref, _loaded(lambda: G.PNAConv(deg=[1], **ref.kwargs()), ref), {"x": inp["x"]},
                 {"edge_index": inp["edge_index"]}, _sparse_call, inp["g"],
                 violations=PN.family_violations(ref, inp["x"][None], PN.sparse_pattern(inp["edge_index"], M)))


PNA_SEEDS = ((700, 701), (710, 711))      # (dense, sparse) x shape: no family violation (asserted on the CPU)

_BUILDERS = {"GraphConv-add": functools.partial(_graphconv, "add"),
             "GraphConv-mean": functools.partial(_graphconv, "mean"),
             "GraphConv-max": functools.partial(_graphconv, "max"), "SAGEConv": _sage, "GCNConv": _gcn, "GINConv": _gin,
             "GATConv": _gat, "TransformerConv": _transformer, "ResGatedGraphConv": _resgated, "GatedGraphConv": _gated,
             "TAGConv": _tag, "PNAConv": _pna}
# (family, dense form?) - one parametrised test per layer class, two shapes each
LAYERS = [(family, dense) for family in _BUILDERS for dense in (True, False)]
CASES = [(family, dense, i) for family, dense in LAYERS for i in (0, 1)]


def layer_id(family, dense, i=None):
    name = ("Dense" if dense else "") + family
    return name if i is None else "%s-%d" % (name, i)


@functools.lru_cache(maxsize=None)
def spec(family, dense, i):
    return _BUILDERS[family](dense, i)


def run(module, s, subset, dtype=None, device=None):
    """One forward (and, when anything asks for a gradient, backward) of `module` - the product (dtype None: as it is,
    on `device`) or a copy of the reference made by the caller - under `subset` -> (out detached, {name: grad}, did the
    output require a gradient)."""
    def place(t):
        if dtype is not None and t.is_floating_point():
            t = t.to(dtype)
        return t if device is None else t.to(device)
    inputs = apply(subset, module, {k: place(v) for k, v in s.inputs.items()})
    const = {k: place(v) for k, v in s.const.items()}
    out = s.call(module, inputs, const)
    if out.requires_grad:
        out.backward(place(s.g).view_as(out))
    return out.detach(), grads_of(module, inputs), out.requires_grad


@functools.lru_cache(maxsize=None)
def reference(family, dense, i, subset):
    """The restatement under `subset` in float64 and float32 -> {dtype: (out, {name: grad})}; once per process."""
    s = spec(family, dense, i)
    res = {}
    for dt in (torch.float64, torch.float32):
        out, grads, req = run(copy.deepcopy(s.ref).to(dt), s, subset, dtype=dt)
        assert req == bool(subset)
        res[dt] = (out, grads)
    return res


# ---------------------------------------------------------------------------
# the memories: DenseGCM on tests/_forms.py, SparseGCM on tests/_sparse_forms.py
# ---------------------------------------------------------------------------
RELU3 = ("relu", "relu", 3)              # both biases: every tensor of the packed vector exists
DENSE_MEMORY = [(case, RELU3) for case in ("temporal", "dense8", "both4", "euclid", "fold", "learned", "obs_grad")]
DENSE_MEMORY.append(("temporal", ("tanh", "tanh", 1)))       # the lean cached step
SPARSE_MEMORY = [(case, RELU3) for case in ("oneshot", "two_calls", "chain", "khop", "learned")]
EUCLID_LEARNED = "euclid_learned"        # EuclideanEdge(learned=True) on the inputs of _forms' `euclid`: see below

# Tensors whose gradient is zero analytically, so no input can make it large: the sensitivity condition of
# tests/test_freeze_cpu.py does not apply to them (it asserts that they are zero in float64 instead).
#  * TransformerConv's lin_key.bias adds q_i . b_k to every score of row i alike: the softmax does not see it.
#  * LearnedEdge's net.6.bias / net.5.bias shift every logit of a row alike (tests/_training.zero_gradient).
ANALYTIC_ZERO = {"TransformerConv": ("lin_key.bias",), "learned": ("net.5.bias", "net.6.bias")}


def gnn_layers(names):
    """The GNN's parameter names (no "pre." / "net." / "sel." prefix) by layer -> (layer 1's, layer 2's)."""
    gnn = [n for n in names if not n.startswith(("pre.", "net.", "sel."))]
    heads = sorted({n.split(".", 1)[0] for n in gnn}, key=lambda h: int(h.rsplit("_", 1)[-1]))     # "module_<i>"
    assert len(heads) == 2, heads
    return tuple([n for n in gnn if n.split(".", 1)[0] == h] for h in heads)


def memory_patterns(names, case_has_obs_grad=False, x_grad_possible=True):
    """{pattern: (tensors with requires_grad, do the observations take a gradient, tensors asked of
    torch.autograd.grad | None = loss.backward())} for a memory whose parameters are `names`.  The frozen patterns
    set flags before the forward; the grad_* patterns leave everything trainable and ask torch.autograd.grad for a
    subset - the route that sets task_should_compute_output in the C++ nodes of csrc/torch_ext/step_ext.cpp."""
    names = list(names)
    l1, l2 = gnn_layers(names)
    gnn = set(l1) | set(l2)
    og = bool(case_has_obs_grad)
    pats = {
        "layer1_frozen": ([n for n in names if n not in l1], og, None),
        "layer2_frozen": ([n for n in names if n not in l2], og, None),
        "biases_only": ([n for n in names if is_bias(n)], og, None),
        "weights_only": ([n for n in names if not is_bias(n)], og, None),
        "all_frozen": ([], False, None),
        "grad_layer2": (names, og, list(l2)),
        "grad_bias": (names, og, [n for n in l1 if is_bias(n)][:1]),
    }
    if x_grad_possible:
        pats["gnn_frozen_obs_grad"] = ([], True, None)
        pats["grad_obs"] = (names, True, ["obs"])
    for prefix, what in (("net.", "net"), ("pre.", "pre"), ("sel.", "sel")):
        own = [n for n in names if n.startswith(prefix)]
        if own:
            pats[what + "_frozen"] = ([n for n in names if n not in own], og, None)
            pats["gnn_frozen_%s_trained" % what] = ([n for n in names if n not in gnn], og, None)
    return pats


def keeps_the_path(pattern, spec_, names, case_has_obs_grad=False):
    """A pattern under which the kernels of the unfrozen run must still run: at least one GNN parameter trainable and
    no observation gradient beyond what the case itself asks for."""
    trainable, obs_grad, _ = spec_
    l1, l2 = gnn_layers(names)
    return bool(set(trainable) & (set(l1) | set(l2))) and obs_grad == bool(case_has_obs_grad)


_euclid_cache = {}


def euclid_learned_trajectory(obs_grad=False):
    """tests/_forms.py's `euclid` case (form relu-relu-b3, its seed, parameters and observations) under
    EuclideanEdge(max_distance, learned=True): the node matrix divided by dist_param = max_distance, threshold 1 - the
    oracle selector tests/_golden.oracle_selector builds for a fixture with `learned` in its meta.  The decisions are
    those of the plain case as long as none sits on the threshold (`margin`, of d / dist_param against 1).  -> the
    namespace of _forms.trajectory (hidden, out64, out_atol, bounds - dist_param under "sel.dist_param" when the
    oracle gave it a gradient; it does not: the threshold is a comparison), plus `margin` and `dist_param`."""
    import _forms as F
    from _golden import fp64_rollout_bounds, oracle_selector
    if obs_grad in _euclid_cache:
        return _euclid_cache[obs_grad]
    case, form = "euclid", RELU3
    c = F.CASES[case]
    B, N, Fin, H1, H2, T = c["shape"]
    inp = F.inputs(case, form, F.SEEDS[(case, F.form_id(form))])
    gnn, _, _ = F._modules(inp)
    meta = dict(selector="euclid", max_distance=float(c["sel"][1]), learned=True)
    made = []

    def factory():
        base = oracle_selector(meta, {"dist_param": torch.tensor([float(c["sel"][1])], requires_grad=True)})
        sel = F._WatchedEuclid(c["sel"][1], dist_param=base.dist_param)
        assert type(base) is F.od.EuclideanEdge and sel.max_distance == base.max_distance == 1.0
        made.append(sel)
        return sel
    obs = inp.obs.clone().requires_grad_(obs_grad)
    out32, hid32, bounds, (out64, atol) = fp64_rollout_bounds(gnn, obs, None, inp.w, factory, N)
    t = types.SimpleNamespace(case=EUCLID_LEARNED, form=form, inp=inp, shape=c["shape"], bounds=bounds,
                              hidden=tuple(h.detach() for h in hid32), out64=out64, out_atol=atol,
                              margin=min(s.margin for s in made), dist_param=float(c["sel"][1]),
                              dist_param_grads=[s.dist_param.grad for s in made])
    _euclid_cache[obs_grad] = t
    return t
