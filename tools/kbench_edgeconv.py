#!/usr/bin/env python3
"""Micro-benchmark of the EdgeConv edge-stage kernels (csrc/edgeconv.hip) beside the eager formula on the same device
and operands.  The edge stage alone: from the node-level products P, Q [.., H] to out = max_j (W2 leaky_relu(P_i + Q_j)
+ b2), H = C = 32.  Dense: gcm._ops.dense_edgemax at cfg2's shape (B = 256, N = 128) with the
TemporalBackedge([1, 2, 4]) pattern (3 entries a row) and with the DenseEdge pattern (the strict lower triangle, 63.5
entries a row on average) against the eager form, which materialises h [B, N, N, H] and m [B, N, N, C] (0.5 GB each)
and takes a masked amax.  Sparse: gcm._ops.csr_edgemax at cfg4's (512 graphs x 512 nodes, TemporalEdge([1]) edges, the
kind of CSR index SparseGCM attaches, built once) against gather / scatter-amax.  Gradients go to P, Q, W2 and b2.
Forward alone and forward + backward, timed with device events after a warm-up; the two sides alternate round by round
in one process and the median (and minimum) of the rounds is reported.  The eager forms fit at the full batch on a
288 GB device, so nothing is scaled ("eager_batch" in the record is the batch the eager side ran at).  Prints one JSON
object per (leg, mode) and writes them to --out (default profiles/edgeconv_kbench.jsonl).  Dev / reporting tool."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edgeconv_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "20"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "7"))
SLOPE = 0.0
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


def compare(shape, leg, mode, hip_fn, eager_fn, extra):
    for fn in (hip_fn, eager_fn):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {"hip": [], "eager": []}
    for _ in range(ROUNDS):                     # alternate: both sides see the same clocks and neighbours
        t["hip"].append(once(hip_fn))
        t["eager"].append(once(eager_fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    line = json.dumps({"bench": "edgeconv_kbench", "shape": shape, "leg": leg, "mode": mode, "iters": ITERS,
                       "rounds": ROUNDS, "hip_us": round(med["hip"], 2), "eager_us": round(med["eager"], 2),
                       "hip_min_us": round(min(t["hip"]), 2), "eager_min_us": round(min(t["eager"]), 2),
                       "eager_over_hip": round(med["eager"] / med["hip"], 3), **extra})
    print(line, flush=True)
    lines.append(line)


def legs(shape, leg, hip, eager, leaves, g, extra):
    """hip / eager: () -> out.  Forward alone without a graph, then forward + backward into `leaves`."""
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
    del a, b
    compare(shape, leg, "fwd", fwd(hip), fwd(eager), extra)
    compare(shape, leg, "fwd+bwd", fb(hip), fb(eager), extra)


H = C = 32
W2 = (torch.randn(C, H, device=dev) * H ** -0.5).requires_grad_()
b2 = (0.1 * torch.randn(C, device=dev)).requires_grad_()

# ---- dense, cfg2 ----
B, N = 256, 128
P = torch.randn(B, N, H, device=dev, requires_grad=True)
Q = torch.randn(B, N, H, device=dev, requires_grad=True)
g = torch.randn(B, N, C, device=dev)
hops = sum(torch.diag_embed(torch.ones(B, N - h, device=dev), offset=-h) for h in (1, 2, 4))   # node i <- i - h
lower = torch.tril(torch.ones(N, N, device=dev), -1).expand(B, N, N).contiguous()              # DenseEdge


def eager_dense(adj):
    pat = (adj != 0).unsqueeze(-1)
    has = pat.any(dim=2)

    def run():
        h = torch.nn.functional.leaky_relu(P.unsqueeze(2) + Q.unsqueeze(1), SLOPE)     # [B,N,N,H]
        m = torch.nn.functional.linear(h, W2, b2).masked_fill(~pat, float("-inf"))     # [B,N,N,C]
        return torch.where(has, m.amax(dim=2), torch.zeros((), device=dev))
    return run


for name, adj in (("temporal_backedge_1_2_4", hops), ("dense_edge", lower)):
    legs("cfg2", "dense_edgemax_" + name, lambda adj=adj: _ops.dense_edgemax(P, Q, adj, W2, b2, SLOPE),
         eager_dense(adj), [P, Q, W2, b2], g, {"entries": int((adj != 0).sum()), "eager_batch": B})
del hops, lower

# ---- sparse, cfg4 ----
Bg, Ns = 512, 512
M = Bg * Ns
n = torch.arange(M, device=dev)
keep = n % Ns != 0
edges = torch.stack([n[keep] - 1, n[keep]])
node_off = torch.arange(Bg + 1, device=dev) * Ns
graph = _ops.GraphIndex(edges, _ops.ptr_from_sorted(edges[1], M), M, batches=(node_off, Bg, Ns))
graph.csc()                                                            # built once, as across SparseGCM's layers
Ps = torch.randn(M, H, device=dev, requires_grad=True)
Qs = torch.randn(M, H, device=dev, requires_grad=True)
gs = torch.randn(M, C, device=dev)
src, dst = edges[0], edges[1]
dst_c = dst.unsqueeze(-1).expand(-1, C)


def eager_csr():
    m = torch.nn.functional.linear(torch.nn.functional.leaky_relu(Ps[dst] + Qs[src], SLOPE), W2, b2)   # [E,C]
    top = torch.full((M, C), float("-inf"), device=dev).scatter_reduce(0, dst_c, m, reduce="amax")
    return torch.where(torch.isinf(top), torch.zeros((), device=dev), top)


legs("cfg4", "csr_edgemax_temporal_edge_1", lambda: _ops.csr_edgemax(Ps, Qs, W2, b2, SLOPE, graph), eager_csr,
     [Ps, Qs, W2, b2], gs, {"entries": int(edges.shape[1]), "eager_batch": Bg})

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
