"""Eager, dtype-generic restatement of gcm.nn.PNAConv / DensePNAConv (Corso et al. 2020, as PyG's PNAConv lays it
out), written literally from the layers' contract: the message is pre_nn([x_i | x_j]) per edge, the aggregators are
taken over the materialised messages, var = mean(m^2) - mean(m)^2.  Also the modules with the layers' parameter
layout, the two input families of the GPU tests and their case table, shared by tests/test_pna_cpu.py (which checks
the families' conditions) and tests/test_pna_gpu.py.

Two families, because min / max / std are not continuous:
  dyadic  - x integers in [-2, 2], pre weights and biases multiples of 1/4 in [-1/2, 1/2]: every message is a multiple
            of 1/4 and exact in fp32, ties are exact in every precision, and a neighbourhood's variance is exactly 0
            or at least (n-1)/(16 n^2), far from the 1e-5 rule of std.  Every case that lists var or std, and the tie
            tests.
  generic - randn; only for lists without var / std.  The min / max winners need a margin (min_max_margin)."""
import functools
import math

import torch
import torch.nn.functional as F

from _aggr_restate import random_edges

AGGREGATORS = ("sum", "mean", "min", "max", "var", "std")
SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")
PAPER = (("mean", "min", "max", "std"), ("identity", "amplification", "attenuation"))
STD_EPS = 1e-5


# ---------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------
def aggregate(msg, valid, aggregators):
    """msg [R, D, C]: the candidate messages of every row (any finite value where not valid), valid [R, D] ->
    ([R, A C] the aggregators in list order, n [R]).  A tie in min / max goes to the first candidate."""
    v = valid.unsqueeze(-1)
    n = valid.sum(1)
    nf = n.clamp(min=1).to(msg.dtype).unsqueeze(-1)
    m0 = torch.where(v, msg, torch.zeros_like(msg))
    total = m0.sum(1)
    mean = total / nf
    var = (m0 * m0).sum(1) / nf - mean * mean
    std = var.clamp(min=STD_EPS).sqrt()
    std = torch.where(std <= math.sqrt(STD_EPS), torch.zeros_like(std), std)
    out = []
    for a in aggregators:
        if a in ("min", "max"):
            fill = torch.full_like(msg, float("inf") if a == "min" else float("-inf"))
            cand = torch.where(v, msg.detach(), fill)
            win = (cand.argmin(1, keepdim=True) if a == "min" else cand.argmax(1, keepdim=True))
            val = msg.gather(1, win).squeeze(1)
        else:
            val = {"sum": total, "mean": mean, "var": var, "std": std}[a]
        out.append(torch.where((n > 0).unsqueeze(-1), val, torch.zeros_like(val)))
    return torch.cat(out, -1), n


def scale(agg, n, scalers, avg_lin, avg_log):
    """[R, A C] -> [R, S A C]: each scaler times the whole block, in list order."""
    nf = n.to(agg.dtype).unsqueeze(-1)
    n1 = nf.clamp(min=1)
    table = {"identity": torch.ones_like(nf), "amplification": (nf + 1).log() / avg_log,
             "attenuation": avg_log / (n1 + 1).log(), "linear": nf / avg_lin, "inverse_linear": avg_lin / n1}
    return torch.cat([table[s] * agg for s in scalers], -1)


def dense_messages(x_t, w_pre, b_pre):
    """x_t [B,N,Fi] -> m [B,N,N,Fi]: m[b,i,j] = W_pre [x_i | x_j] + b_pre."""
    B, N, Fi = x_t.shape
    pair = torch.cat([x_t.unsqueeze(2).expand(B, N, N, Fi), x_t.unsqueeze(1).expand(B, N, N, Fi)], -1)
    return F.linear(pair, w_pre, b_pre)


def dense_pattern(adj, add_loop):
    pat = adj != 0
    if add_loop:
        pat = pat | torch.eye(adj.shape[-1], dtype=torch.bool, device=adj.device)
    return pat


def csr_slots(edge_index, M):
    """The layer's CSR order: (src, dst, slot, D) of the edges stably sorted by sink; slot: the place in its row."""
    E = edge_index.shape[1]
    order = torch.sort(edge_index[1], stable=True)[1]
    src, dst = edge_index[0][order], edge_index[1][order]
    count = torch.bincount(dst, minlength=M)
    D = max(int(count.max()) if E else 0, 1)
    slot = torch.arange(E, device=dst.device) - (torch.cumsum(count, 0) - count)[dst]
    return src, dst, slot, D


def sparse_messages(x_t, edge_index, w_pre, b_pre):
    """x_t [M,Fi] -> (msg [M,D,Fi] in CSR order, valid [M,D])."""
    M = x_t.shape[0]
    src, dst, slot, D = csr_slots(edge_index, M)
    m = F.linear(torch.cat([x_t[dst], x_t[src]], -1), w_pre, b_pre)
    msg = torch.zeros(M, D, x_t.shape[1], dtype=x_t.dtype, device=x_t.device).index_put((dst, slot), m)
    valid = torch.zeros(M, D, dtype=torch.bool, device=x_t.device).index_put((dst, slot), torch.ones_like(dst, dtype=torch.bool))
    return msg, valid


class _PNARef(torch.nn.Module):
    """The parameter layout of gcm.nn.PNAConv / DensePNAConv (PyG 2.3+ names)."""

    def __init__(self, in_channels, out_channels, aggregators, scalers, deg, towers=1, post_layers=1,
                 divide_input=False):
        super().__init__()
        self.in_channels, self.out_channels, self.towers, self.divide_input = in_channels, out_channels, towers, divide_input
        self.aggregators, self.scalers, self.post_layers = list(aggregators), list(scalers), post_layers
        self.F_in = in_channels // towers if divide_input else in_channels
        self.F_out = out_channels // towers
        self.pre_nns, self.post_nns = torch.nn.ModuleList(), torch.nn.ModuleList()
        for _ in range(towers):
            self.pre_nns.append(torch.nn.Sequential(torch.nn.Linear(2 * self.F_in, self.F_in)))
            mods = [torch.nn.Linear((len(self.aggregators) * len(self.scalers) + 1) * self.F_in, self.F_out)]
            for _ in range(post_layers - 1):
                mods += [torch.nn.ReLU(), torch.nn.Linear(self.F_out, self.F_out)]
            self.post_nns.append(torch.nn.Sequential(*mods))
        self.lin = torch.nn.Linear(out_channels, out_channels)
        self.aggr_module = torch.nn.Module()
        deg = torch.as_tensor(deg).detach().to("cpu", torch.float64)
        d = torch.arange(deg.numel(), dtype=torch.float64)
        self.aggr_module.register_buffer("avg_deg_lin", ((d * deg).sum() / deg.sum()).float().reshape(1))
        self.aggr_module.register_buffer("avg_deg_log", (((d + 1).log() * deg).sum() / deg.sum()).float().reshape(1))

    def kwargs(self):
        return dict(in_channels=self.in_channels, out_channels=self.out_channels, aggregators=self.aggregators,
                    scalers=self.scalers, towers=self.towers, post_layers=self.post_layers,
                    divide_input=self.divide_input)

    def _tower_x(self, x, t):
        return x[..., t * self.F_in:(t + 1) * self.F_in] if self.divide_input else x

    def _towers(self, x, messages):
        """x [R.., in]; messages(x_t, w, b) -> (msg [R, D, Fi], valid [R, D])."""
        lead = x.shape[:-1]
        am = self.aggr_module
        hs = []
        for t in range(self.towers):
            x_t = self._tower_x(x, t)
            pre = self.pre_nns[t][0]
            msg, valid = messages(x_t, pre.weight, pre.bias)
            agg, n = aggregate(msg, valid, self.aggregators)
            scaled = scale(agg, n, self.scalers, am.avg_deg_lin, am.avg_deg_log)
            hs.append(self.post_nns[t](torch.cat([x_t.reshape(-1, self.F_in), scaled], -1)))
        return self.lin(torch.cat(hs, -1)).reshape(*lead, self.out_channels)


class DensePNARef(_PNARef):
    def forward(self, x, adj, mask=None, add_loop=False):
        x = x.unsqueeze(0) if x.dim() == 2 else x
        adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
        B, N, _ = x.shape
        pat = dense_pattern(adj.expand(B, N, N), add_loop).reshape(B * N, N)

        def messages(x_t, w, b):
            return dense_messages(x_t, w, b).reshape(B * N, N, self.F_in), pat
        out = self._towers(x, messages)
        return out if mask is None else out * mask.view(B, N, 1).to(out.dtype)


class PNARef(_PNARef):
    def forward(self, x, edge_index, edge_attr=None):
        return self._towers(x, lambda x_t, w, b: sparse_messages(x_t, edge_index, w, b))


# ---------------------------------------------------------------------------
# the input families
# ---------------------------------------------------------------------------
def lively(ref, seed, dyadic):
    """Parameters away from their initial scale; dyadic: the pre linears on the 1/4 grid in [-1/2, 1/2]."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.4)
        if dyadic:
            for seq in ref.pre_nns:
                for p in seq.parameters():
                    p.copy_(torch.randint(-2, 3, p.shape, generator=gen).float() / 4)
    return ref


def features(shape, seed, dyadic):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, shape, generator=gen).float() if dyadic else torch.randn(shape, generator=gen)


def is_dyadic(aggregators):
    return "var" in aggregators or "std" in aggregators


def min_max_margin(msg, valid):
    """[R, C] the smaller of the relative gaps between the two best candidates for max and for min, inf with fewer
    than two; float64.  Candidates are the columns of `valid`: for a sparse layer pass the pattern of distinct
    sources (sparse_pattern) - duplicate edges carry bit-identical messages in every precision, the first of them
    wins everywhere, and x gets the same gradient whichever does, so they are one candidate."""
    msg = msg.double()
    if msg.shape[1] < 2:
        return torch.full(msg[:, 0].shape, float("inf"), dtype=torch.float64)
    gaps = []
    for sign in (1.0, -1.0):
        cand = torch.where(valid.unsqueeze(-1), sign * msg, torch.full_like(msg, float("-inf")))
        top = cand.topk(2, dim=1).values
        gap = (top[:, 0] - top[:, 1]) / top[:, 0].abs().clamp(min=1e-30)
        gaps.append(torch.where(torch.isfinite(top[:, 1]), gap, torch.full_like(gap, float("inf"))))
    return torch.minimum(*gaps)


def sparse_pattern(edge_index, M):
    """adj [1, M, M]: 1 where there is at least one edge j -> i."""
    adj = torch.zeros(M, M)
    adj[edge_index[1], edge_index[0]] = 1
    return adj.unsqueeze(0)


def family_violations(ref, x, adj, add_loop=False):
    """How many (node, channel) break the case's family condition, over every tower, in float64.  dyadic (var / std
    listed): n >= 2 with variance in (0, 1e-4).  generic: min_max_margin < 1e-5 when min or max is listed.  x [B,N,in]
    and adj [B,N,N] (for a sparse case x[None] and sparse_pattern)."""
    ref64 = _as(ref, torch.float64)
    x = x.double()
    B, N, _ = x.shape
    pat = dense_pattern(adj.expand(B, N, N), add_loop).reshape(B * N, N)
    bad = 0
    for t in range(ref.towers):
        pre = ref64.pre_nns[t][0]
        msg = dense_messages(ref64._tower_x(x, t), pre.weight, pre.bias).reshape(B * N, N, ref.F_in).detach()
        if is_dyadic(ref.aggregators):
            agg, n = aggregate(msg, pat, ["var"])
            bad += int(((n >= 2).unsqueeze(-1) & (agg > 0) & (agg < 1e-4)).sum())
        elif "min" in ref.aggregators or "max" in ref.aggregators:
            bad += int((min_max_margin(msg, pat) < 1e-5).sum())
    return bad


def _as(ref, dtype):
    import copy
    return copy.deepcopy(ref).to(dtype)


# ---------------------------------------------------------------------------
# the GPU tests' case table
# ---------------------------------------------------------------------------
ALL = (AGGREGATORS, SCALERS)
NOVAR = (("sum", "mean", "min", "max"), SCALERS)                      # generic family
PERMUTED = (("std", "max", "sum", "min"), ("attenuation", "identity", "linear"))
LISTS = (ALL, NOVAR, PAPER, PERMUTED)
DENSE_SHAPES = ((1, 5, 3, 4, 1, False), (3, 33, 8, 6, 2, False), (3, 33, 8, 6, 2, True), (2, 70, 33, 5, 1, False),
                (2, 128, 32, 32, 1, False), (1, 130, 4, 8, 2, False))   # (B, N, in, out, towers, divide_input)
PATTERNS = ("empty", "chain", "tril", "random")


def pattern(name, B, N, seed):
    if name == "empty":
        return torch.zeros(B, N, N)
    if name == "chain":                                             # TemporalBackedge([1]): i aggregates from i - 1
        return torch.diag(torch.ones(N - 1), -1).expand(B, N, N).clone()
    if name == "tril":                                              # DenseEdge: every earlier node
        return torch.tril(torch.ones(N, N), -1).expand(B, N, N).clone()
    gen = torch.Generator().manual_seed(seed)
    adj = (torch.rand(B, N, N, generator=gen) < 0.3).float() * (torch.rand(B, N, N, generator=gen) + 0.5)
    adj[:, ::4] = 0                                                 # some empty rows
    return adj


def _dense_cases():
    cases, k = [], 0
    for shape in DENSE_SHAPES:
        for p in PATTERNS:
            cases.append(dict(shape=shape, pattern=p, lists=LISTS[k % 4], mask=k % 2 == 1, add_loop=(k // 2) % 2 == 1,
                              flat=False, post_layers=1, seed=100 + k))
            k += 1
    for a in AGGREGATORS:                                           # each aggregator alone
        cases.append(dict(shape=DENSE_SHAPES[1], pattern="random", lists=((a,), ("identity",)), mask=False,
                          add_loop=False, flat=False, post_layers=1, seed=100 + k))
        k += 1
    cases.append(dict(shape=(2, 20, 40, 6, 2, False), pattern="random", lists=ALL, mask=False, add_loop=False,
                      flat=False, post_layers=1, seed=99))          # 80 channels: more than one channel block
    cases.append(dict(shape=(1, 33, 8, 6, 2, False), pattern="random", lists=PAPER, mask=False, add_loop=False,
                      flat=True, post_layers=1, seed=100 + k))      # a 2-D x and one shared adj
    cases.append(dict(shape=DENSE_SHAPES[1], pattern="random", lists=PAPER, mask=True, add_loop=True, flat=False,
                      post_layers=2, seed=101 + k))                 # the torch tail behind the first post linear
    return cases


DENSE_CASES = _dense_cases()
SPARSE_WIDTHS = {7: ((3, 4, 1, False),), 70: ((8, 6, 2, False), (33, 5, 1, False), (8, 6, 2, True)),
                 200: ((32, 32, 1, False), (4, 8, 2, False))}


def _sparse_cases():
    cases, k = [], 0
    for M in (7, 70, 200):
        for E in (0, 12, 400, 2000):
            widths = SPARSE_WIDTHS[M]
            cases.append(dict(M=M, E=E, widths=widths[k % len(widths)], lists=LISTS[k % 4], post_layers=1,
                              seed=300 + k))
            k += 1
    for a in AGGREGATORS:
        cases.append(dict(M=70, E=400, widths=(8, 6, 2, False), lists=((a,), ("identity",)), post_layers=1,
                          seed=300 + k))
        k += 1
    cases.append(dict(M=70, E=400, widths=(8, 6, 2, False), lists=PAPER, post_layers=2, seed=300 + k))
    return cases


SPARSE_CASES = _sparse_cases()


def case_id(case):
    lists = "+".join(case["lists"][0]) + "x" + str(len(case["lists"][1]))
    if "shape" in case:
        B, N, cin, cout, T, div = case["shape"]
        tags = "".join(t for t, on in (("-div", div), ("-mask", case["mask"]), ("-loop", case["add_loop"]),
                                        ("-2d", case["flat"]), ("-post2", case["post_layers"] > 1)) if on)
        return f"{B}x{N}x{cin}x{cout}t{T}-{case['pattern']}-{lists}{tags}"
    cin, cout, T, div = case["widths"]
    return f"M{case['M']}E{case['E']}-{cin}x{cout}t{T}{'-div' if div else ''}-{lists}" + \
        ("-post2" if case["post_layers"] > 1 else "")


def histogram(n):
    """A degree histogram from the in-degrees n of the case itself, plus one node in every bin (and in bins 1 and 2)
    so that neither degree statistic is 0 on an empty graph."""
    return torch.bincount(n.reshape(-1).long(), minlength=3) + 1


def dense_inputs(case):
    B, N, cin, cout, T, div = case["shape"]
    aggregators, scalers = case["lists"]
    dyadic = is_dyadic(aggregators)
    adj = pattern(case["pattern"], B, N, case["seed"])
    deg = histogram(dense_pattern(adj, case["add_loop"]).sum(-1))
    ref = lively(DensePNARef(cin, cout, aggregators, scalers, deg, T, case["post_layers"], div), case["seed"], dyadic)
    gen = torch.Generator().manual_seed(case["seed"] + 1)
    mask = (torch.rand(B, N, generator=gen) < 0.8) if case["mask"] else None
    x = features((B, N, cin), case["seed"] + 2, dyadic)
    g = torch.randn(B, N, cout, generator=gen)
    if case["flat"]:
        x, adj = x[0], adj[0]
    return dict(ref=ref, x=x, adj=adj, mask=mask, add_loop=case["add_loop"], g=g, dyadic=dyadic)


def sparse_inputs(case):
    M, E = case["M"], case["E"]
    cin, cout, T, div = case["widths"]
    aggregators, scalers = case["lists"]
    dyadic = is_dyadic(aggregators)
    ei = random_edges(M, E, case["seed"])
    deg = histogram(torch.bincount(ei[1], minlength=M))
    ref = lively(PNARef(cin, cout, aggregators, scalers, deg, T, case["post_layers"], div), case["seed"], dyadic)
    gen = torch.Generator().manual_seed(case["seed"] + 1)
    x = features((M, cin), case["seed"] + 2, dyadic)
    return dict(ref=ref, x=x, edge_index=ei, g=torch.randn(M, cout, generator=gen), dyadic=dyadic)


def evaluate(ref, call, g):
    """{dtype: {"out", "x", parameter names}} of the restatement in float64 and float32; call(ref, cast) -> (out, x)."""
    res = {}
    for dt in (torch.float64, torch.float32):
        r = _as(ref, dt)
        out, x = call(r, lambda t: t.to(dt) if t.is_floating_point() else t)
        out.backward(g.to(dt).view_as(out))
        res[dt] = {"out": out.detach(), "x": x.grad, **{k: p.grad for k, p in r.named_parameters()}}
    return res


@functools.lru_cache(maxsize=None)
def dense_reference(index):
    inp = dense_inputs(DENSE_CASES[index])

    def call(r, cast):
        x = cast(inp["x"]).clone().requires_grad_()
        return r(x, cast(inp["adj"]), inp["mask"], inp["add_loop"]), x
    return inp, evaluate(inp["ref"], call, inp["g"])


@functools.lru_cache(maxsize=None)
def sparse_reference(index):
    inp = sparse_inputs(SPARSE_CASES[index])

    def call(r, cast):
        x = cast(inp["x"]).clone().requires_grad_()
        return r(x, inp["edge_index"]), x
    return inp, evaluate(inp["ref"], call, inp["g"])
