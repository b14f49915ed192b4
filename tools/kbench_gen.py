#!/usr/bin/env python3
"""Micro-benchmark of the GEN softmax-aggregation kernels (csrc/genconv.hip) beside their eager formulas on the same
device and operands.  Dense: gcm._ops.dense_genagg at cfg2's shape (B = 256, N = 128, C = 32, a
TemporalBackedge([1, 2, 4])-like adjacency) against (a) the masked softmax over [B, N, N, C] written out, which is
exact under any shift as the kernel is, and (b) the two contractions adj @ (p * m) / adj @ p with p = exp(t m - the
graph's maximum), the fast eager form, which underflows rows far below their graph's maximum.  Sparse:
gcm._ops.csr_genagg at cfg4's (512 graphs x 512 nodes, TemporalEdge([1]) edges, C = 32, the kind of CSR index SparseGCM
attaches, built once) against scatter-amax / index_add.  Gradients go to xs and t.  Forward alone and forward +
backward, timed with device events after a warm-up; the two sides alternate round by round in one process and the
median (and minimum) of the rounds is reported.  Prints one JSON object per (leg, mode) and writes them to --out
(default profiles/gen_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gen_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "50"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "9"))
EPS = 1e-7
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


def compare(shape, leg, mode, hip_fn, eager_fn):
    for fn in (hip_fn, eager_fn):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {"hip": [], "eager": []}
    for _ in range(ROUNDS):                     # alternate: both sides see the same clocks and neighbours
        t["hip"].append(once(hip_fn))
        t["eager"].append(once(eager_fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    line = json.dumps({"bench": "gen_kbench", "shape": shape, "leg": leg, "mode": mode, "iters": ITERS,
                       "rounds": ROUNDS, "hip_us": round(med["hip"], 2), "eager_us": round(med["eager"], 2),
                       "hip_min_us": round(min(t["hip"]), 2), "eager_min_us": round(min(t["eager"]), 2),
                       "eager_over_hip": round(med["eager"] / med["hip"], 3)})
    print(line, flush=True)
    lines.append(line)


def legs(shape, leg, hip, eager, leaves, g):
    """hip / eager: () -> agg.  Forward alone without a graph, then forward + backward into `leaves`."""
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
    a, b = hip(), eager()
    err = float((a - b).detach().abs().max())
    assert err <= 1e-4 * float(b.detach().abs().max()), err       # the two sides compute the same thing
    compare(shape, leg, "fwd", fwd(hip), fwd(eager))
    compare(shape, leg, "fwd+bwd", fb(hip), fb(eager))


# ---- dense, cfg2 ----
B, N, C = 256, 128, 32
x = torch.randn(B, N, C, device=dev, requires_grad=True)
t = torch.full((1,), 1.0, device=dev, requires_grad=True)
adj = sum(torch.diag_embed(torch.ones(B, N - h, device=dev), offset=-h) for h in (1, 2, 4))   # node i <- i - h
pat = (adj != 0).unsqueeze(-1)
g = torch.randn(B, N, C, device=dev)


def eager_softmax():
    m = torch.relu(x) + EPS
    logit = (t * m).unsqueeze(1).expand(B, N, N, C).masked_fill(~pat, float("-inf"))
    a = torch.softmax(logit, dim=2).nan_to_num(0.0)               # an empty row: 0
    return (a * m.unsqueeze(1)).sum(2)


def eager_contraction():
    m = torch.relu(x) + EPS
    logit = t * m
    p = torch.exp(logit - logit.amax(dim=1, keepdim=True).detach())
    return adj @ (p * m) / (adj @ p).clamp(min=1e-30)


legs("cfg2", "dense_genagg_vs_masked_softmax", lambda: _ops.dense_genagg(x, adj, t, EPS), eager_softmax, [x, t], g)
legs("cfg2", "dense_genagg_vs_two_contractions", lambda: _ops.dense_genagg(x, adj, t, EPS), eager_contraction,
     [x, t], g)

# ---- sparse, cfg4 ----
Bg, Ns = 512, 512
M = Bg * Ns
n = torch.arange(M, device=dev)
keep = n % Ns != 0
edges = torch.stack([n[keep] - 1, n[keep]])
node_off = torch.arange(Bg + 1, device=dev) * Ns
graph = _ops.GraphIndex(edges, _ops.ptr_from_sorted(edges[1], M), M, batches=(node_off, Bg, Ns))
graph.csc()                                                            # built once, as across SparseGCM's layers
xs = torch.randn(M, C, device=dev, requires_grad=True)
gs = torch.randn(M, C, device=dev)
src, dst = edges[0], edges[1]
dst_c = dst.unsqueeze(-1).expand(-1, C)


def eager_csr():
    m = torch.relu(xs) + EPS
    mj = m[src]
    logit = t * mj
    top = torch.full((M, C), float("-inf"), device=dev).scatter_reduce(0, dst_c, logit.detach(), reduce="amax")
    p = torch.exp(logit - top[dst])
    s = torch.zeros(M, C, device=dev).index_add_(0, dst, p)
    w = torch.zeros(M, C, device=dev).index_add_(0, dst, p * mj)
    return w / s.clamp(min=1e-30)


legs("cfg4", "csr_genagg", lambda: _ops.csr_genagg(xs, t, graph, EPS), eager_csr, [xs, t], gs)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
