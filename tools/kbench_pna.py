#!/usr/bin/env python3
"""Micro-benchmark of the PNA layers (csrc/pnaconv.hip) with the paper's lists - mean, min, max, std x identity,
amplification, attenuation - in one process, against (a) the eager restatement of the same layer on the GPU
(tests/_pna_restate.py) and (b) the two existing single-aggregator layers, GraphConv(aggr="mean") and
GraphConv(aggr="max"), run one after the other on the same operands: the question is whether four aggregators in one
pass cost less than two in two.  Dense: cfg2's shape (B = 256, N = 128, F = 32) on the TemporalBackedge([1])-like
chain and the DenseEdge-like lower triangle of tools/kbench_aggr.py.  Sparse: cfg4's (512 graphs x 512 nodes,
TemporalEdge([1]) edges, F = 32, the kind of CSR index SparseGCM attaches, built once).  Forward alone and forward +
backward, timed with device events; every figure is measured KBENCH_REPEATS times and reported as the median with the
spread (max - min) / median of those repeats.  Writes one JSON object per (shape, layer, mode) to the file given as
the first argument (default profiles/pna_kbench.jsonl) and to stdout."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import _pna_restate as R  # noqa: E402
from gcm import _ops  # noqa: E402
from gcm import nn as G  # noqa: E402

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "50"))
REPEATS = int(os.environ.get("KBENCH_REPEATS", "5"))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pna_kbench.jsonl")
torch.manual_seed(0)
out_file = open(OUT, "w")
AGGREGATORS, SCALERS = R.PAPER


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
    line = json.dumps({"bench": "pna_kbench", "shape": shape, "layer": layer, "mode": mode, "us": round(med, 2),
                       "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                       "spread": round((max(us) - min(us)) / med, 4), "repeats": REPEATS})
    print(line, flush=True)
    out_file.write(line + "\n")
    out_file.flush()


def bench(shape, layers):
    for name, fwd in layers:
        with torch.no_grad():
            report(shape, name, "fwd", fwd)
        report(shape, name, "fwd+bwd", lambda: fwd().sum().backward())


def dense_layers(F, deg, x, adj):
    pna = G.DensePNAConv(F, F, AGGREGATORS, SCALERS, deg).to(dev)
    ref = R.DensePNARef(F, F, AGGREGATORS, SCALERS, deg).to(dev)
    mean, mx = G.DenseGraphConv(F, F, aggr="mean").to(dev), G.DenseGraphConv(F, F, aggr="max").to(dev)
    return [("DensePNAConv(paper)", lambda: pna(x, adj)), ("eager restatement", lambda: ref(x, adj)),
            ("DenseGraphConv(mean)+DenseGraphConv(max)", lambda: mean(x, adj) + mx(x, adj))]


# ---- dense, cfg2 ----
B, N, F = 256, 128, 32
x = torch.randn(B, N, F, device=dev, requires_grad=True)
chain = torch.diag_embed(torch.ones(B, N - 1, device=dev), offset=-1)   # node i <- i - 1
bench("cfg2", dense_layers(F, G.degree_histogram(chain[0]), x, chain))
tril = torch.ones(N, N, device=dev).tril(-1).expand(B, N, N).contiguous()  # node i <- every j < i
bench("cfg2_tril", dense_layers(F, G.degree_histogram(tril[0]), x, tril))

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
deg = G.degree_histogram(edges, M)
pna = G.PNAConv(F, F, AGGREGATORS, SCALERS, deg).to(dev)
ref = R.PNARef(F, F, AGGREGATORS, SCALERS, deg).to(dev)
mean, mx = G.GraphConv(F, F, aggr="mean").to(dev), G.GraphConv(F, F, aggr="max").to(dev)
bench("cfg4", [("PNAConv(paper)", lambda: pna(xs, edges)), ("eager restatement", lambda: ref(xs, edges)),
               ("GraphConv(mean)+GraphConv(max)", lambda: mean(xs, edges, w) + mx(xs, edges, w))])
out_file.close()
