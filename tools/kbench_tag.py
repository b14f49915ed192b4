#!/usr/bin/env python3
"""Micro-benchmark of the TAG layers (csrc/tagconv.hip) beside their eager formula on the same device and parameters
(torch.bmm / index_add), and beside the same reach built from what existed before: K stacked DenseGCNConv / GCNConv
layers at the same width.  F = 32, K in {1, 3}.  Dense: gcm.nn.DenseTAGConv(32, 32, K) at cfg2's shape (B = 256, N =
128) on two patterns, the sparse and the full end of the sweep: TemporalBackedge([1, 2, 4])'s band (three entries per
row) and DenseEdge's lower triangle.  Sparse: gcm.nn.TAGConv(32, 32, K) at cfg4's (512 graphs x 512 nodes,
TemporalEdge([1]) edges, the kind of CSR index SparseGCM attaches, built once).  Forward alone and forward + backward
(gradients to x and every parameter), timed with device events after a warm-up; the sides alternate round by round in
one process and the median (and minimum) of the rounds is reported.  GCM_TAG_NO_SKIP=1 in the environment makes the
dense kernels visit the empty 32 x 32 tiles of the adjacency too (the record says which was measured).  Prints one
JSON object per (leg, K, mode) and writes them to --out (default profiles/tag_kbench.jsonl; --append adds to it).
Dev / reporting tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops, nn as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tag_kbench.jsonl"))
ap.add_argument("--append", action="store_true")
ap.add_argument("--dense-only", action="store_true")
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "10"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "5"))
SKIP = os.environ.get("GCM_TAG_NO_SKIP", "0") != "1"
torch.manual_seed(0)
lines = []


def once(fn):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / ITERS * 1e3      # us per call


def compare(shape, leg, K, mode, fns):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):                     # alternate: every side sees the same clocks and neighbours
        for k, fn in fns.items():
            t[k].append(once(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    rec = {"bench": "tag_kbench", "shape": shape, "leg": leg, "K": K, "mode": mode, "iters": ITERS, "rounds": ROUNDS,
           "tile_skip": SKIP}
    for k in fns:
        rec[k + "_us"], rec[k + "_min_us"] = round(med[k], 2), round(min(t[k]), 2)
    rec["eager_over_hip"] = round(med["eager"] / med["hip"], 3)
    rec["gcn_stack_over_hip"] = round(med["gcn_stack"] / med["hip"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def legs(shape, leg, K, sides, leaves, g):
    """sides: name -> (() -> out).  Forward alone without a graph, then forward + backward into `leaves`."""
    def fwd(f):
        def run():
            with torch.no_grad():
                f()
        return run

    def fb(f):
        def run():
            for t in leaves:
                t.grad = None
            f().backward(g)
        return run
    a, b = sides["hip"](), sides["eager"]()
    err = float((a - b).detach().abs().max())
    assert err <= 1e-4 * float(b.detach().abs().max()), err       # the two sides compute the same thing
    compare(shape, leg, K, "fwd", {k: fwd(f) for k, f in sides.items()})
    compare(shape, leg, K, "fwd+bwd", {k: fb(f) for k, f in sides.items()})


def inv_sqrt(deg):
    return torch.where(deg > 0, deg.clamp(min=1e-30) ** -0.5, torch.zeros_like(deg))


def eager_dense(conv, x, adj):
    d = inv_sqrt(adj.sum(-1))
    A = d.unsqueeze(-1) * adj * d.unsqueeze(-2)
    h = x
    out = h @ conv.lins[0].weight.t()
    for lin in conv.lins[1:]:
        h = torch.bmm(A, h)
        out = out + h @ lin.weight.t()
    return out + conv.bias


def eager_sparse(conv, x, src, dst):
    M = x.shape[0]
    d = inv_sqrt(torch.zeros(M, device=x.device).index_add_(0, dst, torch.ones(src.numel(), device=x.device)))
    coef = (d[src] * d[dst]).unsqueeze(-1)
    h = x
    out = h @ conv.lins[0].weight.t()
    for lin in conv.lins[1:]:
        h = torch.zeros_like(h).index_add_(0, dst, coef * h[src])
        out = out + h @ lin.weight.t()
    return out + conv.bias


def stack(layers, x, *rest, **kw):
    h = x
    for layer in layers:
        h = layer(h, *rest, **kw)
    return h


C = 32
# ---- dense, cfg2 ----
B, N = 256, 128
x = torch.randn(B, N, C, device=dev, requires_grad=True)
g = torch.randn(B, N, C, device=dev)
band = sum(torch.diag_embed(torch.ones(B, N - h, device=dev), offset=-h) for h in (1, 2, 4))   # node i <- i - h
tril = torch.ones(N, N, device=dev).tril(-1).expand(B, N, N).contiguous()    # node i <- every j < i
for K in (1, 3):
    conv = G.DenseTAGConv(C, C, K).to(dev)
    gcns = torch.nn.ModuleList([G.DenseGCNConv(C, C) for _ in range(K)]).to(dev)
    leaves = [x] + list(conv.parameters()) + list(gcns.parameters())
    for name, adj in (("backedge_1_2_4", band), ("dense_edge_tril", tril)):
        legs("cfg2", "dense_" + name, K, {"hip": lambda: conv(x, adj), "eager": lambda: eager_dense(conv, x, adj),
                                          "gcn_stack": lambda: stack(gcns, x, adj, add_loop=False)}, leaves, g)
del band, tril

# ---- sparse, cfg4 ----
if not args.dense_only:
    Bg, Ns = 512, 512
    M = Bg * Ns
    t = torch.arange(M, device=dev)
    keep = t % Ns != 0
    edges = torch.stack([t[keep] - 1, t[keep]])
    node_off = torch.arange(Bg + 1, device=dev) * Ns
    edges.gcm_graph = _ops.GraphIndex(edges, _ops.ptr_from_sorted(edges[1], M), M, batches=(node_off, Bg, Ns))
    edges.gcm_graph.csc()                                                  # built once, as across SparseGCM's layers
    xs = torch.randn(M, C, device=dev, requires_grad=True)
    gs = torch.randn(M, C, device=dev)
    src, dst = edges[0], edges[1]
    for K in (1, 3):
        sconv = G.TAGConv(C, C, K).to(dev)
        sgcns = torch.nn.ModuleList([G.GCNConv(C, C, add_self_loops=False) for _ in range(K)]).to(dev)
        legs("cfg4", "csr_temporal_edge_1", K,
             {"hip": lambda: sconv(xs, edges), "eager": lambda: eager_sparse(sconv, xs, src, dst),
              "gcn_stack": lambda: stack(sgcns, xs, edges)}, [xs] + list(sconv.parameters()) + list(sgcns.parameters()),
             gs)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as f:
    f.write("\n".join(lines) + "\n")
