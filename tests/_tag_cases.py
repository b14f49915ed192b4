"""The case table of the TAGConv tests, shared by tests/test_tag_cpu.py (which checks that every case is well
conditioned) and tests/test_tag_gpu.py (which runs the kernels on them).  A case's inputs are built on the CPU from its
own seed; its references - the restatement in float64 and float32, outputs and every gradient - are computed once per
process and shared.  Every weight is non-negative (the degrees are sums of them)."""
import copy
import functools

import torch

from _tag_restate import DenseTagRef, TagRef, lively

# (B, N, Fi, Fo, K, options): each hits one edge of the kernels
DENSE_CASES = [
    (3, 7, 3, 5, 1, {}),                                                # below one tile, odd widths
    (3, 7, 3, 5, 3, {"mask": True, "weighted": True, "adj_grad": True}),
    (5, 1, 4, 3, 2, {"add_loop": True}),                                # a single node
    (2, 33, 8, 8, 2, {"bias": False, "empty": True, "adj_grad": True}),  # one past a tile; deg == 0 rows and columns
    (2, 40, 16, 12, 3, {"normalize": False, "weighted": True, "adj_grad": True}),
    (2, 40, 6, 9, 0, {"adj_grad": True}),                               # K = 0: the plain linear layer
    (4, 128, 32, 32, 3, {"pattern": "band", "adj_grad": True}),         # TemporalBackedge([1, 2, 4]): node 0 reads nobody
    (2, 129, 32, 32, 3, {"weighted": True, "adj_grad": True, "add_loop": True}),   # first N past the one-workgroup path
    (2, 70, 128, 128, 2, {"mask": True}),                               # the widest channels
    (2, 64, 64, 96, 4, {"bcast": True, "add_loop": True}),
    (1, 33, 8, 8, 2, {"two_d": True, "weighted": True}),                # 2-D x and adj
    (2, 129, 20, 40, 2, {"empty": True, "normalize": False}),           # the per-hop path without the degrees
]

# (M, E, Fi, Fo, K, options); edges() adds duplicate edges and loops and leaves the last three nodes isolated
SPARSE_CASES = [
    (10, 30, 3, 5, 1, {}),
    (40, 90, 8, 6, 3, {"edge_weight": True}),
    (300, 900, 64, 32, 2, {"edge_weight": True, "normalize": False}),
    (50, 0, 4, 4, 2, {}),                                               # no edges
    (70, 400, 128, 128, 2, {"bias": False}),
    (40, 90, 8, 6, 0, {"edge_weight": True}),                           # K = 0
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


def edges(M, E, seed):
    """tests/test_gat_gpu.py's construction: duplicate loops, a duplicate edge, the last three nodes isolated."""
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, M - 3), (2, E), generator=gen)      # the last 3 nodes stay isolated
    if E:
        extra = torch.tensor([[0, 1, 0, 2, 1], [0, 2, 0, 2, 2]])      # duplicate loops (0, 0), duplicate edge 1 -> 2
        ei = torch.cat([ei[:, : E // 2], extra, ei[:, E // 2:]], 1)
    return ei


def _ref(cls, case, seed):
    _, _, Fi, Fo, K, opts = case
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    ref = lively(cls(Fi, Fo, K, bias=opts.get("bias", True), normalize=opts.get("normalize", True)))
    torch.random.set_rng_state(state)
    return ref


def dense_inputs(case):
    """-> dict: ref (DenseTagRef, float32), x, adj, mask, g, add_loop, adj_grad."""
    B, N, Fi, Fo, K, opts = case
    seed = B * 1000 + N * 7 + Fi + Fo + K
    gen = torch.Generator().manual_seed(seed)
    ref = _ref(DenseTagRef, case, seed)
    nb = 1 if opts.get("bcast") else B
    if opts.get("pattern") == "band":
        adj = band(N).expand(nb, N, N).clone()
    else:
        adj = (torch.rand(nb, N, N, generator=gen) < 0.3).float()
        if opts.get("weighted"):
            adj = adj * (torch.rand(nb, N, N, generator=gen) * 1.5 + 0.1)      # weights in [0.1, 1.6]
    if opts.get("empty"):
        adj[:, : N // 4] = 0            # nodes that read nobody: deg == 0
        adj[:, :, N // 2] = 0           # a node nobody reads
    x = torch.randn(B, N, Fi, generator=gen)
    mask = (torch.rand(B, N, generator=gen) < 0.7) if opts.get("mask") else None
    g = torch.randn(B, N, Fo, generator=gen)
    if opts.get("two_d"):
        x, adj = x[0], adj[0]
    return {"ref": ref, "x": x, "adj": adj, "mask": mask, "g": g, "add_loop": opts.get("add_loop", False),
            "adj_grad": opts.get("adj_grad", False)}


def sparse_inputs(case):
    """-> dict: ref (TagRef, float32), x, edge_index, edge_weight (or None), g."""
    M, E, Fi, Fo, K, opts = case
    seed = M + E * 3 + Fi + Fo + K
    gen = torch.Generator().manual_seed(seed)
    ref = _ref(TagRef, case, seed)
    ei = edges(M, E, seed=M + E)
    ew = (torch.rand(ei.shape[1], generator=gen) * 1.5 + 0.1) if opts.get("edge_weight") else None
    return {"ref": ref, "x": torch.randn(M, Fi, generator=gen), "edge_index": ei, "edge_weight": ew,
            "g": torch.randn(M, Fo, generator=gen)}


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
            got["adj"] = adj.grad if adj.grad is not None else torch.zeros_like(adj)     # K = 0
        if not dense and inp["edge_weight"] is not None:
            got["edge_weight"] = ew.grad if ew.grad is not None else torch.zeros_like(ew)
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
