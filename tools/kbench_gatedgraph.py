#!/usr/bin/env python3
"""Micro-benchmark of the gated graph layers (csrc/gatedgraphconv.hip) beside their eager formula on the same device
and parameters (torch.bmm / index_add + torch.nn.GRUCell), and beside L stacked GraphConv layers at the same width:
the yardstick for "one round is about one GraphConv layer plus a GRU".  C = 32, L in {1, 3}.  Dense:
gcm.nn.DenseGatedGraphConv(32, L) at cfg2's shape (B = 256, N = 128) on two patterns, the sparse and the full end of
the sweep: TemporalBackedge([1, 2, 4])'s band (three entries per row) and DenseEdge's lower triangle.  Sparse:
gcm.nn.GatedGraphConv(32, L) at cfg4's (512 graphs x 512 nodes, TemporalEdge([1]) edges, the kind of CSR index
SparseGCM attaches, built once) against the gather / index_add formula.  Forward alone and forward + backward
(gradients to x and every parameter), timed with device events after a warm-up; the sides alternate round by round in
one process and the median (and minimum) of the rounds is reported.  Prints one JSON object per (leg, L, mode) and
writes them to --out (default profiles/gatedgraph_kbench.jsonl).  Dev / reporting tool."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gatedgraph_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "10"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "5"))
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


def compare(shape, leg, L, mode, fns):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):                     # alternate: every side sees the same clocks and neighbours
        for k, fn in fns.items():
            t[k].append(once(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    rec = {"bench": "gatedgraph_kbench", "shape": shape, "leg": leg, "L": L, "mode": mode, "iters": ITERS,
           "rounds": ROUNDS}
    for k in fns:
        rec[k + "_us"], rec[k + "_min_us"] = round(med[k], 2), round(min(t[k]), 2)
    rec["eager_over_hip"] = round(med["eager"] / med["hip"], 3)
    rec["graphconv_over_hip"] = round(med["graphconv"] / med["hip"], 3)
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def legs(shape, leg, L, sides, leaves, g):
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
    compare(shape, leg, L, "fwd", {k: fwd(f) for k, f in sides.items()})
    compare(shape, leg, L, "fwd+bwd", {k: fb(f) for k, f in sides.items()})


def eager_dense(conv, x, adj):
    B, N, C = x.shape
    h = x
    for l in range(conv.num_layers):
        m = torch.bmm(adj, h @ conv.weight[l])
        h = conv.rnn(m.view(B * N, C), h.reshape(B * N, C)).view(B, N, C)
    return h


def eager_sparse(conv, x, src, dst):
    h = x
    for l in range(conv.num_layers):
        m = torch.zeros_like(h).index_add_(0, dst, (h @ conv.weight[l])[src])
        h = conv.rnn(m, h)
    return h


def stack(layers, *args):
    h = args[0]
    for layer in layers:
        h = layer(h, *args[1:])
    return h


C = 32
# ---- dense, cfg2 ----
B, N = 256, 128
x = torch.randn(B, N, C, device=dev, requires_grad=True)
g = torch.randn(B, N, C, device=dev)
band = sum(torch.diag_embed(torch.ones(B, N - h, device=dev), offset=-h) for h in (1, 2, 4))   # node i <- i - h
tril = torch.ones(N, N, device=dev).tril(-1).expand(B, N, N).contiguous() / N    # node i <- every j < i, scaled
for L in (1, 3):
    conv = G.DenseGatedGraphConv(C, L).to(dev)
    gcs = torch.nn.ModuleList([G.DenseGraphConv(C, C) for _ in range(L)]).to(dev)
    leaves = [x] + list(conv.parameters()) + list(gcs.parameters())
    for name, adj in (("backedge_1_2_4", band), ("dense_edge_tril", tril)):
        legs("cfg2", "dense_" + name, L, {"hip": lambda: conv(x, adj), "eager": lambda: eager_dense(conv, x, adj),
                                          "graphconv": lambda: stack(gcs, x, adj)}, leaves, g)
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
xs = torch.randn(M, C, device=dev, requires_grad=True)
gs = torch.randn(M, C, device=dev)
src, dst = edges[0], edges[1]
for L in (1, 3):
    sconv = G.GatedGraphConv(C, L).to(dev)
    sgcs = torch.nn.ModuleList([G.GraphConv(C, C) for _ in range(L)]).to(dev)
    legs("cfg4", "csr_temporal_edge_1", L,
         {"hip": lambda: sconv(xs, edges), "eager": lambda: eager_sparse(sconv, xs, src, dst),
          "graphconv": lambda: stack(sgcs, xs, edges)}, [xs] + list(sconv.parameters()) + list(sgcs.parameters()), gs)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
