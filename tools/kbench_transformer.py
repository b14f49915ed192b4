#!/usr/bin/env python3
"""Micro-benchmark of the TransformerConv layers (csrc/transformerconv.hip) beside the GAT and GCN layers on the same
operands.  Dense: DenseTransformerConv (heads 1 and 4, H*C = 32) vs DenseGATConv and DenseGCNConv at cfg2's shape (B =
256, N = 128, F = 32, a TemporalBackedge([1])-like adjacency).  Sparse: TransformerConv (heads 1 and 4) vs GATConv and
GCNConv at cfg4's (512 graphs x 512 nodes, TemporalEdge([1]) edges, F = 32, the kind of CSR index SparseGCM attaches,
built once).  Forward alone and forward + backward per layer, timed with device events.  Prints one JSON object per
(layer, mode) and writes them to --out (default profiles/transformer_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops  # noqa: E402
from gcm import nn as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "50"))
torch.manual_seed(0)
lines = []


def timeit(fn, iters=ITERS):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters * 1e3      # us per call


def report(shape, layer, mode, us):
    line = json.dumps({"bench": "transformer_kbench", "shape": shape, "layer": layer, "mode": mode,
                       "us": round(us, 2)})
    print(line, flush=True)
    lines.append(line)


def run(shape, name, conv, *inputs):
    conv = conv.to(dev)
    with torch.no_grad():
        report(shape, name, "fwd", timeit(lambda: conv(*inputs)))

    def fb():
        conv(*inputs).sum().backward()
    report(shape, name, "fwd+bwd", timeit(fb))


# ---- dense, cfg2 ----
B, N, F = 256, 128, 32
x = torch.randn(B, N, F, device=dev, requires_grad=True)
adj = torch.diag_embed(torch.ones(B, N - 1, device=dev), offset=-1)   # node i <- i - 1
run("cfg2", "DenseTransformerConv_h1", G.DenseTransformerConv(F, F), x, adj)
run("cfg2", "DenseTransformerConv_h4", G.DenseTransformerConv(F, F // 4, heads=4), x, adj)
run("cfg2", "DenseTransformerConv_h4_beta", G.DenseTransformerConv(F, F // 4, heads=4, beta=True), x, adj)
run("cfg2", "DenseGATConv_h1", G.DenseGATConv(F, F), x, adj)
run("cfg2", "DenseGATConv_h4", G.DenseGATConv(F, F // 4, heads=4), x, adj)
run("cfg2", "DenseGCNConv", G.DenseGCNConv(F, F), x, adj)

# ---- sparse, cfg4 ----
Bg, Ns = 512, 512
M = Bg * Ns
t = torch.arange(M, device=dev)
keep = t % Ns != 0
edges = torch.stack([t[keep] - 1, t[keep]])
w = torch.ones(edges.shape[1], device=dev)
w.gcm_unit_weights = True
node_off = torch.arange(Bg + 1, device=dev) * Ns
edges.gcm_graph = _ops.GraphIndex(edges, _ops.ptr_from_sorted(edges[1], M), M, batches=(node_off, Bg, Ns))
xs = torch.randn(M, F, device=dev, requires_grad=True)
run("cfg4", "TransformerConv_h1", G.TransformerConv(F, F), xs, edges, w)
run("cfg4", "TransformerConv_h4", G.TransformerConv(F, F // 4, heads=4), xs, edges, w)
run("cfg4", "GATConv_h1", G.GATConv(F, F), xs, edges, w)
run("cfg4", "GATConv_h4", G.GATConv(F, F // 4, heads=4), xs, edges, w)
run("cfg4", "GCNConv", G.GCNConv(F, F), xs, edges, w)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
