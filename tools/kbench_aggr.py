#!/usr/bin/env python3
"""Micro-benchmark of the mean / max layers (csrc/aggrconv.hip) beside the sum and GCN layers on the same operands, in
one process.  Dense: DenseGraphConv(aggr=mean|max) and DenseSAGEConv vs DenseGraphConv (add) and DenseGCNConv at cfg2's
shape (B = 256, N = 128, F = 32).  Two adjacencies: the TemporalBackedge([1])-like chain tools/kbench_gcn.py uses and
a DenseEdge-like lower triangle (every node sees all earlier ones: what a max has to scan).  Sparse: GraphConv(aggr=
mean|max) and SAGEConv vs GraphConv (add) and GCNConv at cfg4's (512 graphs x 512 nodes, TemporalEdge([1]) edges,
F = 32, SparseGCM's unit weights and the kind of CSR index it attaches) and on the same graph at F = 128.  Forward
alone and forward + backward per layer, timed with device events; every figure is measured KBENCH_REPEATS times and
reported as the median with the spread (max - min) / median of those repeats.  Writes one JSON object per (shape,
layer, mode) to the file given as the first argument (default profiles/aggr_kbench.jsonl) and to stdout."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops  # noqa: E402
from gcm import nn as G  # noqa: E402

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "50"))
REPEATS = int(os.environ.get("KBENCH_REPEATS", "5"))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "aggr_kbench.jsonl")
torch.manual_seed(0)
out_file = open(OUT, "w")


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


def report(shape, layer, mode, fn):
    us = [timeit(fn) for _ in range(REPEATS)]
    med = statistics.median(us)
    line = json.dumps({"bench": "aggr_kbench", "shape": shape, "layer": layer, "mode": mode, "us": round(med, 2),
                       "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                       "spread": round((max(us) - min(us)) / med, 4), "repeats": REPEATS})
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()


def bench(shape, layers, args):
    for name, conv, n_args in layers:
        conv = conv.to(dev)
        call = args[:n_args]
        with torch.no_grad():
            report(shape, name, "fwd", lambda: conv(*call))

        def fb():
            conv(*call).sum().backward()
        report(shape, name, "fwd+bwd", fb)


def dense_layers(F):
    return [("DenseGraphConv(add)", G.DenseGraphConv(F, F), 2), ("DenseGCNConv", G.DenseGCNConv(F, F), 2),
            ("DenseGraphConv(mean)", G.DenseGraphConv(F, F, aggr="mean"), 2), ("DenseSAGEConv", G.DenseSAGEConv(F, F), 2),
            ("DenseGraphConv(max)", G.DenseGraphConv(F, F, aggr="max"), 2)]


def sparse_layers(F):
    return [("GraphConv(add)", G.GraphConv(F, F), 3), ("GCNConv", G.GCNConv(F, F), 3),
            ("GraphConv(mean)", G.GraphConv(F, F, aggr="mean"), 3), ("SAGEConv(mean)", G.SAGEConv(F, F), 2),
            ("GraphConv(max)", G.GraphConv(F, F, aggr="max"), 3), ("SAGEConv(max)", G.SAGEConv(F, F, aggr="max"), 2)]


# ---- dense, cfg2 ----
B, N, F = 256, 128, 32
x = torch.randn(B, N, F, device=dev, requires_grad=True)
chain = torch.diag_embed(torch.ones(B, N - 1, device=dev), offset=-1)   # node i <- i - 1
bench("cfg2", dense_layers(F), (x, chain))
tril = torch.ones(N, N, device=dev).tril(-1).expand(B, N, N).contiguous()  # node i <- every j < i
bench("cfg2_tril", dense_layers(F), (x, tril))

# ---- sparse, cfg4 ----
Bg, Ns = 512, 512
M = Bg * Ns
t = torch.arange(M, device=dev)
keep = t % Ns != 0
edges = torch.stack([t[keep] - 1, t[keep]])
w = torch.ones(edges.shape[1], device=dev)
w.gcm_unit_weights = True
# the index SparseGCM attaches (sparse_edges_to_csr): edges already in CSR order (csr_perm None), grouped by
# graph (batches set, so the backward's CSC view is built without a sort)
node_off = torch.arange(Bg + 1, device=dev) * Ns
edges.gcm_graph = _ops.GraphIndex(edges, _ops.ptr_from_sorted(edges[1], M), M, batches=(node_off, Bg, Ns))
xs = torch.randn(M, F, device=dev, requires_grad=True)
bench("cfg4", sparse_layers(F), (xs, edges, w))

# ---- sparse, cfg4's graph at F = 128 ----
Fw = 128
xw = torch.randn(M, Fw, device=dev, requires_grad=True)
bench("cfg4_f128", sparse_layers(Fw), (xw, edges, w))
out_file.close()
