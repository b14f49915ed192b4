#!/usr/bin/env python3
"""Micro-benchmark of the deterministic LearnedEdge selection (csrc/learned_sparsemax.hip) beside the stochastic one
(csrc/learned.hip) on the same operands.  Kernels: gcm_learned_sparsemax_fwd / _bwd and gcm_learned_select_fwd / _bwd
at cfg5's per-step shape (B = 256, N = 128) with every graph at cur = 16, 64 and 127, logits 3 randn; each timing is a
HIP graph of CALLS back-to-back launches replayed REPS times between device events (a launch from Python costs more
than one of these kernels runs, so a plain loop would time the host), reported per call, with the largest number of
Michelot passes any graph of the batch takes (counted on the host in fp32).  Step: one DenseGCM step (forward +
backward of the belief) with LearnedEdge(32, deterministic=True) against LearnedEdge(32) on the same layered path
(fused=False), from a state of 64 nodes, timed the same way over eager calls.  Prints one JSON object per line and
writes them to --out (default profiles/learned_det_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _hip  # noqa: E402
from gcm import nn as G  # noqa: E402
from gcm.edge_selectors.learned import LearnedEdge  # noqa: E402
from gcm.gcm import DenseGCM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learned_det_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
CALLS = int(os.environ.get("KBENCH_CALLS", "200"))     # launches per captured graph
REPS = int(os.environ.get("KBENCH_REPS", "200"))        # replays per timing
ITERS = int(os.environ.get("KBENCH_ITERS", "200"))      # eager steps per timing
torch.manual_seed(0)
lines = []


def report(**kw):
    line = json.dumps({"bench": "learned_det_kbench", **kw})
    print(line, flush=True)
    lines.append(line)


def time_events(fn, iters):
    for _ in range(5):
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


def michelot_passes(z):
    """passes of the kernel's loop on the rows of z [B, n] (fp32, on the host)"""
    z = z - z.max(-1, keepdim=True).values
    live = torch.ones_like(z, dtype=torch.bool)
    passes = torch.zeros(z.shape[0], dtype=torch.long)
    for _ in range(z.shape[1]):
        k = live.sum(-1)
        tau = ((z * live).sum(-1) - 1) / k
        new = live & (z > tau[:, None])
        passes += 1
        if bool((new.sum(-1) == k).all()):
            break
        live = new
    return int(passes.max())


# ---- kernels, cfg5's per-step shape ----
B, N = 256, 128
lib = _hip.lib()
logits = 3 * torch.randn(B, N, device=dev)
noise = -torch.empty(B, N, device=dev).exponential_().log()
g_adj = torch.randn(B, N, N, device=dev)
adj = torch.zeros(B, N, N, device=dev)
soft_d, soft_s = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
g_logits = torch.empty(B, N, device=dev)
P = _hip.ptr
for c in (16, 64, 127):
    cur = torch.full((B,), c, dtype=torch.long, device=dev)

    def st():
        return _hip.stream()          # (the capture stream while capturing)

    kernels = {
        ("sparsemax", "fwd"): lambda: lib.gcm_learned_sparsemax_fwd(P(logits), P(cur), P(adj), P(soft_d), B, N, st()),
        ("softmax", "fwd"): lambda: lib.gcm_learned_select_fwd(P(logits), P(noise), P(cur), 1 / 6, P(adj), P(soft_s),
                                                               B, N, st()),
        ("sparsemax", "bwd"): lambda: lib.gcm_learned_sparsemax_bwd(P(g_adj), P(soft_d), P(cur), P(g_logits), B, N,
                                                                    st()),
        ("softmax", "bwd"): lambda: lib.gcm_learned_select_bwd(P(g_adj), P(soft_s), P(cur), P(g_logits), B, N, st()),
    }
    passes = michelot_passes(logits[:, :c].cpu())
    for rep in range(2):              # the two forms alternate, twice: the spread shows in the lines
        for (form, mode), fn in kernels.items():
            assert fn() == 0
            extra = {"michelot_passes_max": passes} if (form, mode) == ("sparsemax", "fwd") else {}
            report(shape="cfg5", kernel=f"{form}_{mode}", cur=c, rep=rep, us=round(time_kernel(fn), 3), **extra)

# ---- one DenseGCM step on the layered path ----
F = H = 32


def memory(deterministic):
    torch.manual_seed(1)
    gnn = G.Sequential("x, adj, weights, B, N", [
        (G.DenseGraphConv(F, H), "x, adj -> x"), torch.nn.Tanh(),
        (G.DenseGraphConv(H, H), "x, adj -> x"), torch.nn.Tanh()]).to(dev)
    sel = LearnedEdge(F, deterministic=deterministic).to(dev)
    return DenseGCM(gnn, edge_selectors=sel, graph_size=N, fused=False)


mems = {"deterministic": memory(True), "stochastic": memory(False)}
obs = torch.rand(65, B, F, device=dev)
states = {}
for name, mem in mems.items():
    hidden = None
    with torch.no_grad():
        for t in range(64):
            _, hidden = mem(obs[t], hidden)
    states[name] = tuple(t.detach() for t in hidden)
for rep in range(2):
    for name, mem in mems.items():
        def fwd(mem=mem, name=name):
            with torch.no_grad():
                mem(obs[64], states[name])

        def fwd_bwd(mem=mem, name=name):
            mx, _ = mem(obs[64], states[name])
            mx.sum().backward()
        report(shape="cfg5", step=name, mode="fwd", cur=64, rep=rep, us=round(time_events(fwd, ITERS), 2))
        report(shape="cfg5", step=name, mode="fwd+bwd", cur=64, rep=rep, us=round(time_events(fwd_bwd, ITERS), 2))
for mem in mems.values():
    mem.check_flags()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
