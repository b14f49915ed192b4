#!/usr/bin/env python3
"""Micro-benchmark of KNNEdge (csrc/knn.hip) beside SpatialEdge (k_pergraph of csrc/distance.hip) in ONE process at
cfg2's shapes (B = 256, N = 128, F = 32, H = 32, T = 128): KNNEdge(k=8, slice(0, 3)) against SpatialEdge(r, slice(0,
3)) on the same observations (positions uniform in the unit cube), r chosen so that the threshold selects as many
edges over the T steps as the k-nearest selection does (~8 per sink).

selector: the selector kernel alone (gcm_edge_distance_ex on a state whose graphs all hold cur = 16 / 64 / 127 nodes) -
          a HIP graph of CALLS back-to-back launches replayed REPS times between device events (a launch from Python
          costs more than the kernel runs), us per launch.
loop:     the DenseGCM per-step loop from empty graphs on a donated state, T steps forward + one backward of the
          summed beliefs, host clock around a device synchronise over several such rollouts, us per step - with
          fused=True (live-row / cached step kernels) and with fused=False (the layered path).
The two selectors alternate, `--reps` times each; every line is one timing (the spread shows in the lines).  Prints
one JSON object per line and writes them to --out (default profiles/knn_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _hip  # noqa: E402
from gcm import nn as G  # noqa: E402
from gcm.edge_selectors.distance import SpatialEdge  # noqa: E402
from gcm.edge_selectors.knn import KNNEdge  # noqa: E402
from gcm.gcm import DenseGCM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_kbench.jsonl"))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--steps", type=int, default=128, help="T of the per-step loops")
ap.add_argument("--batch", type=int, default=256)
args = ap.parse_args()

dev = "cuda:0"
CALLS = int(os.environ.get("KBENCH_CALLS", "200"))     # launches per captured graph
REPS = int(os.environ.get("KBENCH_REPS", "100"))        # replays per timing
B, N, F, H, T, K = args.batch, 128, 32, 32, args.steps, 8
torch.manual_seed(0)
lines = []


def report(**kw):
    line = json.dumps({"bench": "knn_kbench", "B": B, "N": N, "F": F, **kw})
    print(line, flush=True)
    lines.append(line)


def time_events(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters * 1e3      # us per call of fn


def time_kernel(launch):
    """us per launch: CALLS launches captured in one graph, replayed REPS times"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CALLS):
            launch()
    return time_events(graph.replay, REPS) / CALLS


obs = torch.rand(T, B, F, device=dev)

# ---- the radius that selects as many edges as k nearest do: the matching quantile of the causal pair distances ----
pos = obs[:, :, :3].permute(1, 0, 2).contiguous()                        # [B, T, 3]
dist = torch.cdist(pos, pos)                                             # [B, T, T]
causal = torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev), -1)  # sink t, source j < t (no wrap: T <= N)
pairs = dist[:, causal]
knn_edges = B * sum(min(K, t) for t in range(T))
radius = float(pairs.flatten().kthvalue(knn_edges).values)
report(what="radius", radius=round(radius, 5), knn_edges_per_sink=round(knn_edges / (B * T), 3),
       radius_edges_per_sink=round(float((pairs < radius).sum()) / (B * T), 3))

selectors = {"knn": lambda: KNNEdge(K, slice(0, 3)), "spatial": lambda: SpatialEdge(radius, slice(0, 3))}

# ---- the selector kernel alone ----
lib = _hip.lib()
P = _hip.ptr
nodes = torch.rand(B, N, F, device=dev)
adj = torch.zeros(B, N, N, device=dev)
for c in (16, 64, 127):
    cur = torch.full((B,), c, dtype=torch.long, device=dev)
    for rep in range(args.reps):
        for name, make in selectors.items():
            sel = make()
            (a0, a1), (b0, b1) = sel._slices(F)

            def launch(sel=sel, a0=a0, a1=a1, b0=b0, b1=b1):
                return lib.gcm_edge_distance_ex(P(nodes), P(adj), P(cur), sel.mode, float(sel.max_distance), None, a0,
                                                a1, b0, b1, 0, None, None, 0, None, 0, B, N, F, _hip.stream())
            assert launch() == 0
            report(what="selector", selector=name, cur=c, rep=rep, us=round(time_kernel(launch), 3))


# ---- the DenseGCM per-step loop, forward + backward ----
def memory(name, fused):
    torch.manual_seed(1)
    gnn = G.Sequential("x, adj, weights, B, N", [
        (G.DenseGraphConv(F, H), "x, adj -> x"), torch.nn.Tanh(),
        (G.DenseGraphConv(H, H), "x, adj -> x"), torch.nn.Tanh()]).to(dev)
    return DenseGCM(gnn, edge_selectors=selectors[name](), graph_size=N, fused=fused, donate_state=True), gnn


def loop(mem, gnn):
    gnn.zero_grad(set_to_none=True)
    hidden, outs = None, []
    for t in range(T):
        mx, hidden = mem(obs[t], hidden)
        outs.append(mx)
    torch.stack(outs).sum().backward()
    return hidden


for fused in (True, False):
    mems = {name: memory(name, fused) for name in selectors}
    for name, (mem, gnn) in mems.items():                     # warm-up: code objects, configurations, workspaces
        for _ in range(2):
            hidden = loop(mem, gnn)
        torch.cuda.synchronize()
        mem.check_flags()
        report(what="loop_setup", selector=name, fused=fused, rows_steps=mem.rows_steps(),
               cached_launches_per_step=mem.rows_cached_launches_per_step(B),
               edges_per_sink=round(float(hidden[1].sum()) / (B * T), 3))
    loops = 10 if fused else 2                                # rollouts per timing (a longer window than one)
    for rep in range(args.reps):
        for name, (mem, gnn) in mems.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(loops):
                loop(mem, gnn)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / loops
            report(what="loop", selector=name, fused=fused, rep=rep, steps=T, loops=loops,
                   us_per_step=round(dt / T * 1e6, 2), ms_per_rollout=round(dt * 1e3, 3))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
