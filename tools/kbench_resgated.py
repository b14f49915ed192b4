#!/usr/bin/env python3
"""Micro-benchmark of the residual gated layers (csrc/resgatedconv.hip) beside their eager formula on the same device
and parameters, and beside the GAT layers at the same width.  Dense: gcm.nn.DenseResGatedGraphConv(32, 32) at cfg2's
shape (B = 256, N = 128) on two patterns, the sparse and the full end of the sweep: TemporalBackedge([1, 2, 4])'s band
(three entries per row) and DenseEdge's full lower triangle; the eager formula materialises the gates [B, N, N, C].
Sparse: gcm.nn.ResGatedGraphConv(32, 32) at cfg4's (512 graphs x 512 nodes, TemporalEdge([1]) edges, the kind of CSR
index SparseGCM attaches, built once) against the gather / index_add formula.  Forward alone and forward + backward
(gradients to x and every parameter), timed with device events after a warm-up; the sides alternate round by round in
one process and the median (and minimum) of the rounds is reported.  Prints one JSON object per (leg, mode) and writes
them to --out (default profiles/resgated_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gcm import _ops, nn as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resgated_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "20"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "7"))
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


def compare(shape, leg, mode, fns):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):                     # alternate: every side sees the same clocks and neighbours
        for k, fn in fns.items():
            t[k].append(once(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    rec = {"bench": "resgated_kbench", "shape": shape, "leg": leg, "mode": mode, "iters": ITERS, "rounds": ROUNDS}
    for k in fns:
        rec[k + "_us"], rec[k + "_min_us"] = round(med[k], 2), round(min(t[k]), 2)
    rec["eager_over_hip"] = round(med["eager"] / med["hip"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def legs(shape, leg, sides, leaves, g):
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
    compare(shape, leg, "fwd", {k: fwd(f) for k, f in sides.items()})
    compare(shape, leg, "fwd+bwd", {k: fb(f) for k, f in sides.items()})


def eager_dense(conv, x, adj):
    k, q, v = conv.lin_key(x), conv.lin_query(x), conv.lin_value(x)
    gate = torch.sigmoid(k.unsqueeze(2) + q.unsqueeze(1))             # [B, N, N, C]
    return (adj.unsqueeze(-1) * gate * v.unsqueeze(1)).sum(2) + conv.lin_skip(x) + conv.bias


def eager_sparse(conv, x, src, dst):
    k, q, v = conv.lin_key(x), conv.lin_query(x), conv.lin_value(x)
    msg = torch.sigmoid(k[dst] + q[src]) * v[src]
    return torch.zeros_like(k).index_add_(0, dst, msg) + conv.lin_skip(x) + conv.bias


# ---- dense, cfg2 ----
B, N, Fi, C = 256, 128, 32, 32
conv = G.DenseResGatedGraphConv(Fi, C).to(dev)
gat = G.DenseGATConv(Fi, C).to(dev)
x = torch.randn(B, N, Fi, device=dev, requires_grad=True)
g = torch.randn(B, N, C, device=dev)
band = sum(torch.diag_embed(torch.ones(B, N - h, device=dev), offset=-h) for h in (1, 2, 4))   # node i <- i - h
tril = torch.ones(N, N, device=dev).tril().expand(B, N, N).contiguous()     # node i <- every j <= i
leaves = [x] + list(conv.parameters()) + list(gat.parameters())
for name, adj in (("backedge_1_2_4", band), ("dense_edge_tril", tril)):
    legs("cfg2", "dense_" + name, {"hip": lambda: conv(x, adj), "eager": lambda: eager_dense(conv, x, adj),
                                   "gat": lambda: gat(x, adj, add_loop=False)}, leaves, g)
del band, tril

# ---- sparse, cfg4 ----
Bg, Ns = 512, 512
M = Bg * Ns
t = torch.arange(M, device=dev)
keep = t % Ns != 0
edges = torch.stack([t[keep] - 1, t[keep]])
node_off = torch.arange(Bg + 1, device=dev) * Ns
edges.gcm_graph = _ops.GraphIndex(edges, _ops.ptr_from_sorted(edges[1], M), M, batches=(node_off, Bg, Ns))
edges.gcm_graph.csc()                                                  # built once, as across SparseGCM's layers
sconv = G.ResGatedGraphConv(Fi, C).to(dev)
sgat = G.GATConv(Fi, C, add_self_loops=False).to(dev)
xs = torch.randn(M, Fi, device=dev, requires_grad=True)
gs = torch.randn(M, C, device=dev)
src, dst = edges[0], edges[1]
legs("cfg4", "csr_temporal_edge_1", {"hip": lambda: sconv(xs, edges), "eager": lambda: eager_sparse(sconv, xs, src, dst),
                                     "gat": lambda: sgat(xs, edges)},
     [xs] + list(sconv.parameters()) + list(sgat.parameters()), gs)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
