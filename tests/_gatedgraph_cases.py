"""The case table of the GatedGraphConv tests, shared by tests/test_gatedgraph_cpu.py (which checks that every case
is well conditioned) and tests/test_gatedgraph_gpu.py (which runs the kernels on them).  A case's inputs are built on
the CPU from its own seed; its references - the restatement in float64 and float32, outputs and every gradient - are
computed once per process and shared."""
import copy
import functools

import torch

from _gatedgraph_restate import DenseGatedRef, GatedRef, lively

# (B, N, Fi, C, L, options): each hits one edge of the kernels
DENSE_CASES = [
    (3, 7, 3, 5, 1, {}),                                        # below one tile, odd widths
    (5, 1, 4, 4, 2, {}),                                        # a single node, Fi == C
    (3, 33, 8, 8, 2, {"mask": True}),                           # image word boundary at 32
    (2, 40, 16, 24, 3, {"empty_rows": True}),                   # a quarter of the rows without a neighbour
    (2, 40, 16, 24, 2, {"add_loop": True}),
    (3, 50, 10, 33, 3, {"weighted": True, "adj_grad": True}),   # negative weights too; two column tiles
    (2, 65, 20, 65, 2, {}),                                     # one past the 64-lane / 64-channel edge
    (2, 130, 20, 128, 2, {}),                                   # the widest C, N past 128
    (4, 300, 64, 64, 1, {}),                                    # rows of one graph over many workgroups
    (1, 20, 6, 9, 2, {"two_d": True}),
    (4, 20, 6, 9, 2, {"bcast": True}),
    (3, 33, 8, 8, 2, {"bias": False}),
    (256, 128, 32, 32, 2, {"pattern": "band"}),                 # cfg2's shape on TemporalBackedge([1, 2, 4])'s band
    (4, 128, 32, 32, 3, {"pattern": "triangle"}),               # DenseEdge's full lower triangle
]

# (M, E, Fi, C, L, options).  The weighted case is 6 wide in and 8 out: the layer takes no input wider than its output.
SPARSE_CASES = [
    (6, 0, 3, 5, 1, {}),                                        # no edges
    (40, 90, 8, 16, 2, {}),
    (40, 90, 6, 8, 3, {"edge_weight": True}),                   # weights that ask for a gradient (Fi < C: padded)
    (300, 1500, 32, 32, 1, {}),
    (129, 700, 64, 128, 2, {}),
    (50, 120, 8, 8, 2, {"bias": False}),
]


def case_id(case):
    return "-".join(str(v) for v in case[:5]) + "".join("-" + k for k in case[5])


def band(N, hops=(1, 2, 4)):
    """The pattern of TemporalBackedge(hops) on a full graph: row i reads the nodes i - k."""
    adj = torch.zeros(N, N)
    for k in hops:
        idx = torch.arange(k, N)
        adj[idx, idx - k] = 1.0
    return adj


def triangle(N):
    """The pattern of DenseEdge on a full graph: row i reads every earlier node."""
    return torch.ones(N, N).tril(-1)


def edges(M, E, seed):
    """tests/test_gat_gpu.py's construction: duplicate loops, a duplicate edge, the last three nodes isolated."""
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, M - 3), (2, E), generator=gen)      # the last 3 nodes stay isolated
    if E:
        extra = torch.tensor([[0, 1, 0, 2, 1], [0, 2, 0, 2, 2]])      # duplicate loops (0, 0), duplicate edge 1 -> 2
        ei = torch.cat([ei[:, : E // 2], extra, ei[:, E // 2:]], 1)
    return ei


def dense_inputs(case):
    """-> dict: ref (DenseGatedRef, float32, lively), x, adj, mask, g, add_loop, adj_grad."""
    B, N, Fi, C, L, opts = case
    gen = torch.Generator().manual_seed(B * 1000 + N * 7 + Fi + C + L)
    state = torch.random.get_rng_state()
    torch.manual_seed(B * 1000 + N * 7 + Fi + C + L)
    ref = lively(DenseGatedRef(C, L, bias=opts.get("bias", True)))
    torch.random.set_rng_state(state)
    nb = 1 if opts.get("bcast") else B
    if opts.get("pattern") == "band":
        adj = band(N).expand(nb, N, N).clone()
    elif opts.get("pattern") == "triangle":
        adj = triangle(N).expand(nb, N, N).clone()
    else:
        adj = (torch.rand(nb, N, N, generator=gen) < 0.3).float()
        if opts.get("weighted"):
            adj = adj * (torch.rand(nb, N, N, generator=gen) * 2 - 0.5)      # weights in [-0.5, 1.5]
    if opts.get("empty_rows"):
        adj[:, : N // 4] = 0
    x = torch.randn(B, N, Fi, generator=gen)
    mask = (torch.rand(B, N, generator=gen) < 0.7) if opts.get("mask") else None
    g = torch.randn(B, N, C, generator=gen)
    if opts.get("two_d"):
        x, adj = x[0], adj[0]
    return {"ref": ref, "x": x, "adj": adj, "mask": mask, "g": g, "add_loop": opts.get("add_loop", False),
            "adj_grad": opts.get("adj_grad", False)}


def sparse_inputs(case):
    """-> dict: ref (GatedRef, float32, lively), x, edge_index, edge_weight (or None), g."""
    M, E, Fi, C, L, opts = case
    gen = torch.Generator().manual_seed(M + E * 3 + Fi + C + L)
    state = torch.random.get_rng_state()
    torch.manual_seed(M + E * 3 + Fi + C + L)
    ref = lively(GatedRef(C, L, bias=opts.get("bias", True)))
    torch.random.set_rng_state(state)
    ei = edges(M, E, seed=M + E)
    ew = (torch.rand(ei.shape[1], generator=gen) * 2 - 0.5) if opts.get("edge_weight") else None
    return {"ref": ref, "x": torch.randn(M, Fi, generator=gen), "edge_index": ei, "edge_weight": ew,
            "g": torch.randn(M, C, generator=gen)}


def _evaluate(inp, dense):
    """{dtype: {name: tensor}}: out, the gradients of x, of every parameter and of adj / edge_weight when asked."""
    res = {}
    for dt in (torch.float64, torch.float32):
        r = copy.deepcopy(inp["ref"]).to(dt)
        x = inp["x"].to(dt, copy=True).requires_grad_()
        if dense:
            adj = inp["adj"].to(dt, copy=True).requires_grad_(inp["adj_grad"])
            out = r(x, adj, inp["mask"], inp["add_loop"])
        else:
            ew = None if inp["edge_weight"] is None else inp["edge_weight"].to(dt, copy=True).requires_grad_()
            out = r(x, inp["edge_index"], ew)
        out.backward(inp["g"].to(dt).view_as(out))
        got = {"out": out.detach(), "x": x.grad}
        got.update({k: p.grad for k, p in r.named_parameters()})
        if dense and inp["adj_grad"]:
            got["adj"] = adj.grad
        if not dense and inp["edge_weight"] is not None:
            got["edge_weight"] = ew.grad
        res[dt] = got
    return res


@functools.lru_cache(maxsize=None)
def dense_reference(index):
    inp = dense_inputs(DENSE_CASES[index])
    return inp, _evaluate(inp, True)


@functools.lru_cache(maxsize=None)
def sparse_reference(index):
    inp = sparse_inputs(SPARSE_CASES[index])
    return inp, _evaluate(inp, False)


def conditioning(res):
    """{name: |f32 restatement - f64| / max|f64|}: a case is usable when every value is at most 1e-4, which keeps the
    3x bound of assert_bounded from going slack."""
    out = {}
    for k, v64 in res[torch.float64].items():
        if v64.numel() == 0:
            continue
        scale = float(v64.abs().max())
        err = float((res[torch.float32][k].double() - v64).abs().max())
        out[k] = err / scale if scale > 0 else err
    return out
