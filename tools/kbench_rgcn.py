#!/usr/bin/env python3
"""Micro-benchmark of the relational kernels (csrc/rgcnconv.hip) beside their torch forms on the same device and
operands, at cfg2's shape: B = 256, N = 128, F = H = 32, R = 3.  The relation planes: the TemporalBackedge([1, 2, 4])
band, a random 8-neighbour relation among the earlier nodes, and the DenseEdge triangle (with the diagonal).

  dense layer   gcm.nn.DenseRGCNConv forward + backward (gradients to x and the parameters; once more with the
                adjacency's gradient, what a LearnedEdge child asks for) vs R masked bmm + linear in torch
  merge         gcm._ops.typed_merge (TypedEdge's one launch: rel | bits, adj = diff_or) vs the elementwise torch ops

Timed with device events after a warm-up; the two sides alternate round by round in one process and the median (and
minimum) of the rounds is reported, with the device launches of one call counted by torch.profiler.  Prints one JSON
object per (leg, mode) and writes them to --out (default profiles/rgcn_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops, nn as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgcn_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "100"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "9"))
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


def launches(fn):
    """Device kernels (and memsets / copies) of one call, or None when the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA"))
        return n or None
    except Exception:
        return None


def compare(leg, mode, hip_fn, torch_fn):
    for fn in (hip_fn, torch_fn):
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    n = {"hip": launches(hip_fn), "torch": launches(torch_fn)}
    t = {"hip": [], "torch": []}
    for _ in range(ROUNDS):                     # alternate: both sides see the same clocks and neighbours
        t["hip"].append(once(hip_fn))
        t["torch"].append(once(torch_fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    line = json.dumps({"bench": "rgcn_kbench", "shape": "cfg2 B256 N128 F32 H32 R3", "leg": leg, "mode": mode,
                       "iters": ITERS, "rounds": ROUNDS, "hip_us": round(med["hip"], 2),
                       "torch_us": round(med["torch"], 2), "hip_min_us": round(min(t["hip"]), 2),
                       "torch_min_us": round(min(t["torch"]), 2), "hip_launches": n["hip"],
                       "torch_launches": n["torch"], "torch_over_hip": round(med["torch"] / med["hip"], 3)})
    print(line, flush=True)
    lines.append(line)


B, N, F, H, R = 256, 128, 32, 32, 3
i, j = torch.arange(N, device=dev)[:, None], torch.arange(N, device=dev)[None, :]
band = ((i - j == 1) | (i - j == 2) | (i - j == 4)).float().expand(B, N, N)
rank = torch.rand(B, N, N, device=dev).masked_fill(j >= i, 2.0)
knn = ((rank <= rank.sort(-1).values[..., 7:8]) & (j < i)).float()          # 8 random earlier nodes per row
tri = (j <= i).float().expand(B, N, N)
planes = [band, knn, tri]
rel = sum(p * (1 << r) for r, p in enumerate(planes)).contiguous()
adj = (rel > 0).float()
masks = [(p > 0).float() for p in planes]
inv = [1.0 / m.sum(-1, keepdim=True).clamp(min=1) for m in masks]

conv = G.DenseRGCNConv(F, H, R).to(dev)
x = torch.randn(B, N, F, device=dev, requires_grad=True)
g = torch.randn(B, N, H, device=dev)


def torch_layer(a):
    out = x @ conv.root + conv.bias
    for r in range(R):
        out = out + (torch.bmm(masks[r] * a, x) * inv[r]) @ conv.weight[r]
    return out


def legs(leg, a):
    leaves = [x] + list(conv.parameters()) + ([a] if a.requires_grad else [])
    hip, eager = (lambda: conv(x, a, rel)), (lambda: torch_layer(a))
    err = float((hip() - eager()).detach().abs().max())
    assert err <= 1e-4 * float(eager().detach().abs().max()), err       # the two sides compute the same thing

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
    compare(leg, "fwd", fwd(hip), fwd(eager))
    compare(leg, "fwd+bwd", fb(hip), fb(eager))


legs("dense_layer", adj)
legs("dense_layer_adj_grad", (adj * torch.rand_like(adj)).requires_grad_())

# ---- TypedEdge's merge: the three planes as what the children selected, onto an earlier state ----
adj0 = (torch.rand(B, N, N, device=dev) < 0.05).float()
rel0 = adj0 * 4.0
bits = [0, 1, 2]


def torch_merge():
    a, code = adj0, rel0.long()
    for r, p in zip(bits, planes):
        a = a + p - a * p
        code = code | ((p > 0).long() << r)
    return a, code.float()


a1, r1 = _ops.typed_merge(adj0, rel0, planes, bits, True)
a2, r2 = torch_merge()
assert torch.equal(a1, a2) and torch.equal(r1, r2)
compare("typed_merge", "fwd", lambda: _ops.typed_merge(adj0, rel0, planes, bits, True), torch_merge)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
