#!/usr/bin/env python3
"""Micro-benchmark of the GIN aggregation kernels (csrc/ginconv.hip) beside their eager formulas on the same device
and operands.  Dense: gcm._ops.dense_gin_aggregate vs `(1 + eps) * x + adj @ x` at cfg2's shape (B = 256, N = 128, F =
32, a TemporalBackedge([1])-like adjacency), with gradients to x and eps, and once more with the adjacency's gradient
(what a LearnedEdge adjacency asks for).  Sparse: gcm._ops.csr_gin_aggregate vs `(1 + eps) * x + index_add_` at cfg4's
(512 graphs x 512 nodes, TemporalEdge([1]) edges, F = 32, the kind of CSR index SparseGCM attaches, built once).
Forward alone and forward + backward, timed with device events after a warm-up; the two sides alternate round by
round in one process and the median (and minimum) of the rounds is reported.  Prints one JSON object per (leg, mode)
and writes them to --out (default profiles/gin_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gin_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "200"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "9"))
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


def compare(shape, leg, mode, hip_fn, eager_fn):
    for fn in (hip_fn, eager_fn):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    t = {"hip": [], "eager": []}
    for _ in range(ROUNDS):                     # alternate: both sides see the same clocks and neighbours
        t["hip"].append(once(hip_fn))
        t["eager"].append(once(eager_fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    line = json.dumps({"bench": "gin_kbench", "shape": shape, "leg": leg, "mode": mode, "iters": ITERS,
                       "rounds": ROUNDS, "hip_us": round(med["hip"], 2), "eager_us": round(med["eager"], 2),
                       "hip_min_us": round(min(t["hip"]), 2), "eager_min_us": round(min(t["eager"]), 2),
                       "eager_over_hip": round(med["eager"] / med["hip"], 3)})
    print(line, flush=True)
    lines.append(line)


def legs(shape, leg, hip, eager, leaves, g):
    """hip / eager: () -> h.  Forward alone without a graph, then forward + backward into `leaves`."""
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
    a, b = hip(), eager()
    err = float((a - b).detach().abs().max())
    assert err <= 1e-4 * float(b.detach().abs().max()), err       # the two sides compute the same thing
    compare(shape, leg, "fwd", fwd(hip), fwd(eager))
    compare(shape, leg, "fwd+bwd", fb(hip), fb(eager))


# ---- dense, cfg2 ----
B, N, F = 256, 128, 32
x = torch.randn(B, N, F, device=dev, requires_grad=True)
eps = torch.full((1,), 0.1, device=dev, requires_grad=True)
adj = torch.diag_embed(torch.ones(B, N - 1, device=dev), offset=-1)   # node i <- i - 1
g = torch.randn(B, N, F, device=dev)
legs("cfg2", "dense_aggregate", lambda: _ops.dense_gin_aggregate(x, adj, eps, True),
     lambda: (1 + eps) * x + adj @ x, [x, eps], g)
adj_g = (adj * torch.rand_like(adj)).requires_grad_()                  # a learned adjacency: g_adj as well
legs("cfg2", "dense_aggregate_adj_grad", lambda: _ops.dense_gin_aggregate(x, adj_g, eps, True),
     lambda: (1 + eps) * x + adj_g @ x, [x, eps, adj_g], g)

# ---- sparse, cfg4 ----
Bg, Ns = 512, 512
M = Bg * Ns
t = torch.arange(M, device=dev)
keep = t % Ns != 0
edges = torch.stack([t[keep] - 1, t[keep]])
node_off = torch.arange(Bg + 1, device=dev) * Ns
graph = _ops.GraphIndex(edges, _ops.ptr_from_sorted(edges[1], M), M, batches=(node_off, Bg, Ns))
graph.csc()                                                            # built once, as across SparseGCM's layers
xs = torch.randn(M, F, device=dev, requires_grad=True)
gs = torch.randn(M, F, device=dev)
src, dst = edges[0], edges[1]
legs("cfg4", "csr_aggregate", lambda: _ops.csr_gin_aggregate(xs, eps, graph),
     lambda: (1 + eps) * xs + torch.zeros_like(xs).index_add_(0, dst, xs[src]), [xs, eps], gs)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
