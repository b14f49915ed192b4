#!/usr/bin/env python3
"""Micro-benchmark of episode resets inside one SparseGCM call (csrc/sparse_segments.hip) at the cfg4
shape (B = 512 graphs of N = 512 nodes, F = H = 32, TemporalEdge [1, 2, 4]), t = 128 columns from empty graphs, every
mask entry true with p = 1/32; written to profiles/sparse_segments_kbench.jsonl:

  calls     (a) rollout(x, reset=mask), (b) rollout(x) and (c) the per-step loop with reset_hidden between the calls
            (the only way to these values without the keyword), wall clock, forward under no_grad; (a) and (b) also
            forward + backward; alternating blocks in one process, median of the repeats, spread stated.  (a) from
            hidden=None (no stored state to expand) and from an explicit zero state (nodes' [B', N, F] is built)
  kernels   the expansion and the collection kernels back to back, timed with device events, beside copy_ of the
            same byte count; the size of nodes'

Dev tool: python tools/kbench_sparse_segments.py [--iters 10] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _hip, _ops, nn as G  # noqa: E402
from gcm.sparse_edge_selectors.temporal import TemporalEdge  # noqa: E402
from gcm.sparse_gcm import SparseGCM  # noqa: E402

B, N, F, H, T_COLS = 512, 512, 32, 32, 128
HOPS = [1, 2, 4]
DEV = "cuda:0"
PEAK_TBS = 8.0


def events_us(fn, iters):
    for _ in range(3):
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


def bench_calls(args, rows, x, mask):
    g = gnn()
    mem = SparseGCM(g, edge_selectors=TemporalEdge(HOPS), graph_size=N)
    one = torch.ones(B, dtype=torch.long, device=DEV)
    cols = [mask[:, s].contiguous() for s in range(T_COLS)]
    any_reset = mask.any(0).tolist()

    def with_reset():
        mem.rollout(x, reset=mask)

    def with_reset_zero_state():
        mem.rollout(x, mem.get_initial_hidden_state(x), reset=mask)

    def plain():
        mem.rollout(x)

    def loop():
        hidden = None
        for s in range(T_COLS):
            if hidden is not None and any_reset[s]:
                hidden = mem.reset_hidden(hidden, cols[s])
            _, hidden = mem(x[:, s:s + 1], one, hidden)

    def train(fn_reset):
        xg = x.detach().requires_grad_(True)
        out, _ = mem.rollout(xg, reset=mask) if fn_reset else mem.rollout(xg)
        out.mean().backward()

    base = {"bench": "sparse_segments_kbench", "shape": "cfg4", "t": T_COLS, "p_reset": 1 / 32}
    names = ["(a) rollout(x, reset=mask), hidden=None", "(a') rollout(x, zero state, reset=mask)", "(b) rollout(x)"]
    samples = {n: [] for n in names}
    with torch.no_grad():
        for _ in range(args.repeats):           # alternating blocks
            for n, fn in zip(names, (with_reset, with_reset_zero_state, plain)):
                samples[n].append(wall_us(fn, args.iters))
        loops = [wall_us(loop, 1) for _ in range(min(args.repeats, 3))]
    for n in names:
        rows.append({**base, "what": n, "mode": "forward, no_grad", **summary(samples[n])})
    rows.append({**base, "what": "(c) per-step loop with reset_hidden between calls", "mode": "forward, no_grad",
                 **summary(loops)})
    tr = {True: [], False: []}
    for _ in range(args.repeats):
        for flag in (True, False):
            tr[flag].append(wall_us(lambda: train(flag), max(1, args.iters // 2)))
    rows.append({**base, "what": "(a) rollout(x, reset=mask), hidden=None", "mode": "forward + backward",
                 **summary(tr[True])})
    rows.append({**base, "what": "(b) rollout(x)", "mode": "forward + backward", **summary(tr[False])})
    a, a0, b, c = (rows[-6]["us"], rows[-5]["us"], rows[-4]["us"], rows[-3]["us"])
    rows.append({**base, "what": "ratios", "a_over_b": round(a / b, 3), "a_zero_state_over_b": round(a0 / b, 3),
                 "c_over_a": round(c / a, 2), "a_over_b_training": round(rows[-2]["us"] / rows[-1]["us"], 3)})
    for r in rows[-7:]:
        print(json.dumps(r))


def bench_kernels(args, rows, x, mask):
    lib, p, st = _hip.lib(), _hip.ptr, _hip.stream()
    mem = SparseGCM(gnn(), edge_selectors=TemporalEdge(HOPS), graph_size=N)
    taus = torch.full((B,), T_COLS, dtype=torch.long, device=DEV)
    nodes, adj, T = mem.get_initial_hidden_state(x)
    m8 = mask.view(torch.uint8)
    plan = _ops.SegmentPlan(m8, taus, T, None)
    Bp, tp, cap = plan.Bp, plan.tp, plan.cap
    totals = torch.empty(4, dtype=torch.long, device=DEV)
    xs = torch.empty(Bp, tp, F, device=DEV)
    nodes_s = torch.empty(Bp, N, F, device=DEV)
    with torch.no_grad():
        out_s, (n2, adj2, T2) = mem(_ops.seg_rows(x, plan, True), plan.row(_hip.SPARSE_SEG_LEN), None)
    idx2, val2 = adj2.indices().contiguous(), adj2.values().contiguous()
    E2 = idx2.shape[1]
    chunk_off = torch.empty(-(-E2 // _hip.SPARSE_SEG_CHUNK) + 1, dtype=torch.long, device=DEV)
    final = plan.row(_hip.SPARSE_SEG_FINAL)
    E_new = _ops.seg_collect_edges(idx2, val2, plan)[0].shape[1]
    out = torch.empty(B, T_COLS, H, device=DEV)
    nodes_f = torch.empty(B, N, F, device=DEV)
    idx_f, val_f = torch.empty(3, E_new, dtype=torch.long, device=DEV), torch.empty(E_new, device=DEV)
    src_pos = torch.empty(E_new, dtype=torch.long, device=DEV)
    T_f = torch.empty(B, dtype=torch.long, device=DEV)

    def expand():
        lib.gcm_sparse_seg_plan(p(m8), p(taus), p(T), None, p(plan.vbase), p(plan.table), cap, p(plan.relabel),
                                p(plan.chunk_off), p(totals), 0, B, T_COLS, st)
        lib.gcm_sparse_seg_rows(p(x), p(plan.table), cap, p(xs), Bp, tp, B, T_COLS, F, 0, st)

    def expand_nodes():
        lib.gcm_sparse_seg_nodes(p(nodes), p(plan.vbase), p(plan.table), cap, p(nodes_s), Bp, B, N, F, 0, 1, st)

    def collect():
        lib.gcm_sparse_seg_rows(p(out_s), p(plan.table), cap, p(out), Bp, tp, B, T_COLS, H, 1, st)
        lib.gcm_sparse_seg_nodes(p(n2), p(plan.vbase), p(plan.table), cap, p(nodes_f), Bp, B, N, F, 1, 0, st)
        lib.gcm_sparse_seg_edges_plan(p(idx2), p(final), p(chunk_off), E2, Bp, st)
        lib.gcm_sparse_seg_edges(p(idx2), p(val2), p(final), p(chunk_off), p(idx_f), p(val_f), p(src_pos), E2, E_new,
                                 Bp, B, st)
        lib.gcm_sparse_seg_final_T(p(T2), p(plan.vbase), p(T_f), Bp, B, st)

    row_bytes = B * T_COLS * F * 4
    groups = (("plan + expand x (4 launches)", expand, B * T_COLS + row_bytes + xs.numel() * 4),
              ("expand nodes (explicit stored state only)", expand_nodes, nodes.numel() * 4 + nodes_s.numel() * 4),
              ("collect outputs, final nodes, final edges, T (6 launches + memset)", collect,
               out_s.numel() * 4 + 2 * out.numel() * 4 + 2 * nodes_f.numel() * 4 + E2 * 8 + E2 * 28 + E_new * 36))
    base = {"bench": "sparse_segments_kbench", "shape": "cfg4", "t": T_COLS, "Bp": Bp, "tp": tp,
            "valid_resets": plan.n_resets, "nodes_s_bytes": nodes_s.numel() * 4, "nodes_bytes": nodes.numel() * 4,
            "E_call": E2, "E_returned": E_new}
    for what, fn, nbytes in groups:
        src = torch.empty(nbytes // 8, dtype=torch.float32, device=DEV)
        dst = torch.empty_like(src)
        for label, f in ((what, fn), ("copy_ of the same bytes as: " + what, lambda: dst.copy_(src))):
            s = summary([events_us(f, args.iters * 5) for _ in range(args.repeats)])
            s["bytes"] = nbytes
            s["tb_per_s"] = round(nbytes / s["us"] / 1e6, 3)
            s["share_of_peak"] = round(s["tb_per_s"] / PEAK_TBS, 3)
            rows.append({**base, "what": label, **s})
            print(json.dumps(rows[-1]))
        del src, dst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_segments_kbench.jsonl"))
    ap.add_argument("--parts", default="calls,kernels", help="which measurements to run (a profiler run takes one)")
    args = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(B, T_COLS, F, generator=gen).to(DEV)
    mask = (torch.rand(B, T_COLS, generator=gen) < 1 / 32).to(DEV)
    rows = []
    if "calls" in args.parts:
        bench_calls(args, rows, x, mask)
    if "kernels" in args.parts:
        bench_kernels(args, rows, x, mask)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
