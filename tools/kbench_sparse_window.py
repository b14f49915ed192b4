#!/usr/bin/env python3
"""Micro-benchmark of SparseGCM's sliding window (csrc/sparse_window.hip) at the cfg4 shape (B = 512
graphs of N = 512 nodes, F = H = 32), written to profiles/sparse_window_kbench.jsonl:

  drop      the kernels of one drop (k = 1, full graphs, TemporalEdge [1] and [1, 2, 4]) back to back, timed with
            device events, beside copy_ of the same byte count; and SparseGCM.drop_oldest as called (host path and
            the one readback included, wall clock)
  step      the stepwise step past N (x [B, 1, F], overflow="wrap", steady state) beside the same memory with
            stepwise_cache=False at T = N - 1, the last step that fits; alternating blocks in one process

Dev tool: python tools/kbench_sparse_window.py [--iters 50] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _hip, nn as G  # noqa: E402
from gcm.sparse_edge_selectors.temporal import TemporalEdge  # noqa: E402
from gcm.sparse_gcm import SparseGCM  # noqa: E402

B, N, F, H = 512, 512, 32, 32
DEV = "cuda:0"
PEAK_TBS = 8.0


def events_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters * 1e3


def wall_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def summary(samples):
    med = statistics.median(samples)
    return {"us": round(med, 2), "min_us": round(min(samples), 2), "max_us": round(max(samples), 2),
            "spread": round((max(samples) - min(samples)) / med, 4), "repeats": len(samples)}


def gnn():
    return G.Sequential("x, edges, weights", [(G.GraphConv(F, H), "x, edges, weights -> x"), torch.nn.Tanh(),
                                               (G.GraphConv(H, H), "x, edges, weights -> x"), torch.nn.Tanh()]).to(DEV)


def bench_drop(hops, args, rows):
    lib, p, st = _hip.lib(), _hip.ptr, _hip.stream()
    zeros = torch.zeros(B, dtype=torch.long, device=DEV)
    T = torch.full((B,), N, dtype=torch.long, device=DEV)
    adj = TemporalEdge(hops)(None, zeros, T, B).coalesce()
    idx, val = adj.indices().contiguous(), adj.values().contiguous()
    nodes = torch.rand(B, N, F, device=DEV)
    k = torch.ones(B, dtype=torch.long, device=DEV)
    E = idx.shape[1]
    n_chunks = -(-E // _hip.SPARSE_DROP_CHUNK)
    chunk_off = torch.empty(n_chunks + 1, dtype=torch.long, device=DEV)
    T_out, nodes_out, bptr = torch.empty_like(T), torch.empty_like(nodes), torch.empty(B + 1, dtype=torch.long, device=DEV)
    mem = SparseGCM(gnn(), edge_selectors=TemporalEdge(hops), graph_size=N)
    E_new = mem.drop_oldest((nodes, adj, T), k)[1]._nnz()
    idx_out = torch.empty(3, E_new, dtype=torch.long, device=DEV)
    val_out = torch.empty(E_new, device=DEV)
    src_pos = torch.empty(E_new, dtype=torch.long, device=DEV)

    def kernels():
        lib.gcm_sparse_drop_plan(p(idx), p(k), p(T), p(T_out), p(chunk_off), E, B, N, st)
        lib.gcm_sparse_drop_nodes(p(nodes), p(k), p(T), p(nodes_out), B, N, F, 0, st)
        lib.gcm_sparse_drop_edges(p(idx), p(val), p(k), p(T), p(chunk_off), p(idx_out), p(val_out), p(src_pos),
                                  p(bptr), E, E_new, B, N, st)

    node_bytes = 2 * nodes.numel() * 4
    # count pass: batch + source rows; compaction: three index rows + values in, three rows + values + positions out
    edge_bytes = E * 16 + E * 28 + E_new * 36
    nbytes = node_bytes + edge_bytes
    src = torch.empty(nbytes // 8, dtype=torch.float32, device=DEV)
    dst = torch.empty_like(src)
    base = {"bench": "sparse_window_kbench", "shape": "cfg4", "hops": hops, "E": E, "E_new": E_new,
            "node_bytes": node_bytes, "edge_bytes": edge_bytes}
    for what, fn, timer in (("drop kernels (4 launches)", kernels, events_us),
                            ("copy_ of the same bytes", lambda: dst.copy_(src), events_us),
                            ("SparseGCM.drop_oldest (host + readback)", lambda: mem.drop_oldest((nodes, adj, T), k),
                             wall_us)):
        s = summary([timer(fn, args.iters) for _ in range(args.repeats)])
        s["tb_per_s"] = round(nbytes / s["us"] / 1e6, 3)
        s["share_of_peak"] = round(s["tb_per_s"] / PEAK_TBS, 3)
        rows.append({**base, "what": what, **s})
        print(json.dumps(rows[-1]))


def bench_step(hops, args, rows):
    g = gnn()
    x = torch.rand(B, 1, F, device=DEV)
    one = torch.ones(B, dtype=torch.long, device=DEV)
    wrap = SparseGCM(g, edge_selectors=TemporalEdge(hops), graph_size=N, overflow="wrap")
    last = SparseGCM(g, edge_selectors=TemporalEdge(hops), graph_size=N)
    last.stepwise_cache = False
    with torch.no_grad():
        _, h_full = wrap.rollout(torch.rand(B, N, F, device=DEV))
        _, h_last = last.rollout(torch.rand(B, N - 1, F, device=DEV))
        state = [h_full]

        def step_wrap():
            state[0] = wrap(x, one, state[0])[1]

        def step_last():            # (functional: the same state N - 1 every time)
            last(x, one, h_last)

        a, b = [], []
        for _ in range(args.repeats):       # alternating blocks
            a.append(wall_us(step_wrap, args.iters))
            b.append(wall_us(step_last, args.iters))
    base = {"bench": "sparse_window_kbench", "shape": "cfg4", "hops": hops}
    rows.append({**base, "what": "stepwise step past N (overflow=wrap, steady state)", **summary(a)})
    rows.append({**base, "what": "stepwise step at T = N - 1 (stepwise_cache=False)", **summary(b)})
    rows.append({**base, "what": "ratio wrap / last fitting step", "ratio": round(rows[-2]["us"] / rows[-1]["us"], 3)})
    for r in rows[-3:]:
        print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_window_kbench.jsonl"))
    ap.add_argument("--parts", default="drop,step", help="which measurements to run (a profiler run takes one)")
    args = ap.parse_args()
    SparseGCM.did_warn = True
    rows = []
    for hops in ([1], [1, 2, 4]):
        if "drop" in args.parts:
            bench_drop(hops, args, rows)
    for hops in ([1], [1, 2, 4]):
        if "step" in args.parts:
            bench_step(hops, args, rows)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
