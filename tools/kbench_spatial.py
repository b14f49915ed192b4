#!/usr/bin/env python3
"""Micro-benchmark of the sparse spatial selectors (csrc/spatial.hip) at cfg4's shape: B = 512 graphs of 512 nodes,
F = 32 node features of which P = 2 are the position.  Back-to-back selector calls (count + the one readback +
fill) timed with device events, beside the count launch alone and a cfg4 SparseGCM call (TemporalEdge([1]), one
shot, forward + backward) for the share.  Legs: one shot (T = 0, tau = 512) and stepwise (T = 256, tau = 1);
SpatialRadiusEdge(radius 0.1: ~7.4 edges per sink one shot) and SpatialKNNEdge(k = 8).
Prints one JSON object per leg.  Dev / reporting tool."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _hip, _ops  # noqa: E402
from gcm import nn as G  # noqa: E402
from gcm.sparse_edge_selectors.spatial import SpatialKNNEdge, SpatialRadiusEdge  # noqa: E402
from gcm.sparse_edge_selectors.temporal import TemporalEdge  # noqa: E402
from gcm.sparse_gcm import SparseGCM  # noqa: E402

B, N, F, H = 512, 512, 32, 32
dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "50"))
torch.manual_seed(0)
nodes = torch.rand(B, N, F, device=dev)


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


def count_only(T, taus, mode, radius, k):
    lib, p = _hip.lib(), _hip.ptr
    arr = (ctypes.c_int32 * 2)(0, 1)
    row_off = torch.empty(B, N, dtype=torch.int32, device=dev)
    kth = torch.empty(B, N, dtype=torch.int64, device=dev)
    edge_off = torch.empty(B + 2, dtype=torch.int64, device=dev)
    st = _hip.stream()
    return lambda: lib.gcm_spatial_count(p(nodes), p(T), p(taus), ctypes.addressof(arr), 2, mode, radius, k,
                                         p(row_off), p(kth), p(edge_off), B, N, F, st)


# cfg4 SparseGCM call (one shot, fwd + bwd): the denominator of the share
g = G.Sequential("x, edges, weights", [(G.GraphConv(F, H), "x, edges, weights -> x"), torch.nn.Tanh(),
                                       (G.GraphConv(H, H), "x, edges, weights -> x"), torch.nn.Tanh()]).to(dev)
mem = SparseGCM(g, edge_selectors=TemporalEdge([1]), graph_size=N)
x = torch.rand(B, N, F, device=dev)
full = torch.full((B,), N, dtype=torch.long, device=dev)


def gcm_call():
    out, _ = mem(x, full, None)
    out.sum().backward()


gcm_us = timeit(gcm_call, iters=max(10, ITERS // 5))

legs = [("oneshot", torch.zeros(B, dtype=torch.long, device=dev), full),
        ("stepwise", torch.full((B,), 256, dtype=torch.long, device=dev), torch.ones(B, dtype=torch.long, device=dev))]
sels = [("radius", SpatialRadiusEdge(slice(0, 2), 0.1), _hip.SPATIAL_RADIUS_CAUSAL, 0.1, 0),
        ("knn", SpatialKNNEdge(slice(0, 2), 8), _hip.SPATIAL_KNN, 0.0, 8)]
for leg, T, taus in legs:
    for name, sel, mode, radius, k in sels:
        E = sel(nodes, T, taus, B)._nnz()
        call_us = timeit(lambda: sel(nodes, T, taus, B))
        cnt_us = timeit(count_only(T, taus, mode, radius, k))
        # pair evaluations: count (kNN: every candidate of [0, n); radius: j < i) + fill (j < i)
        n_new, n_tot = int(taus[0]), int(T[0] + taus[0])
        t0 = int(T[0])
        causal_pairs = sum(range(t0, n_tot))
        count_pairs = B * (n_new * n_tot if name == "knn" else causal_pairs)
        print(json.dumps({"leg": leg, "selector": name, "B": B, "N": N, "T": t0, "tau": n_new, "edges": E,
                          "edges_per_sink": E / (B * n_new), "us_per_call": round(call_us, 2),
                          "us_count_launches": round(cnt_us, 2), "count_pairs": count_pairs,
                          "fill_pairs": B * causal_pairs, "cfg4_sparse_gcm_call_us": round(gcm_us, 1),
                          "share_of_cfg4_call": round(call_us / gcm_us, 4)}))
