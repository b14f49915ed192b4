#!/usr/bin/env python3
"""Micro-benchmark of the GCN layers (csrc/gcnconv.hip) beside the GraphConv layers on the same operands.
Dense: DenseGCNConv vs DenseGraphConv at cfg2's shape (B = 256, N = 128, F = 32, a TemporalBackedge([1])-like
adjacency).  Sparse: GCNConv vs GraphConv at cfg4's (512 graphs x 512 nodes, TemporalEdge([1]) edges, F = 32,
SparseGCM's unit weights and the kind of CSR index SparseGCM attaches; built once, so its lazily built CSC view is
reused across calls, where SparseGCM builds one per call).  Forward alone and forward + backward per layer, timed with device events.
Prints one JSON object per (layer, mode).  Dev / reporting tool."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops  # noqa: E402
from gcm import nn as G  # noqa: E402

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "50"))
torch.manual_seed(0)


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
    print(json.dumps({"bench": "gcn_kbench", "shape": shape, "layer": layer, "mode": mode, "us": round(us, 2)}),
          flush=True)


# ---- dense, cfg2 ----
B, N, F = 256, 128, 32
x = torch.randn(B, N, F, device=dev, requires_grad=True)
adj = torch.diag_embed(torch.ones(B, N - 1, device=dev), offset=-1)   # node i <- i - 1
for name, conv in (("DenseGCNConv", G.DenseGCNConv(F, F)), ("DenseGraphConv", G.DenseGraphConv(F, F))):
    conv = conv.to(dev)
    with torch.no_grad():
        report("cfg2", name, "fwd", timeit(lambda: conv(x, adj)))

    def fb():
        conv(x, adj).sum().backward()
    report("cfg2", name, "fwd+bwd", timeit(fb))

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
for name, conv in (("GCNConv", G.GCNConv(F, F)), ("GraphConv", G.GraphConv(F, F))):
    conv = conv.to(dev)
    with torch.no_grad():
        report("cfg4", name, "fwd", timeit(lambda: conv(xs, edges, w)))

    def fb():
        conv(xs, edges, w).sum().backward()
    report("cfg4", name, "fwd+bwd", timeit(fb))

# ---- sparse, cfg4 graph at F = 128: the widest instantiation (k_gcn_csr_fwd<4>, 81 KB of LDS per workgroup) ----
Fw = 128
xw = torch.randn(M, Fw, device=dev, requires_grad=True)
for name, conv in (("GCNConv", G.GCNConv(Fw, Fw)), ("GraphConv", G.GraphConv(Fw, Fw))):
    conv = conv.to(dev)
    with torch.no_grad():
        report("cfg4_f128", name, "fwd", timeit(lambda: conv(xw, edges, w)))

    def fb():
        conv(xw, edges, w).sum().backward()
    report("cfg4_f128", name, "fwd+bwd", timeit(fb))
