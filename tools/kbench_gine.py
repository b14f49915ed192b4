#!/usr/bin/env python3
"""Micro-benchmark of the fused GINE kernels (csrc/gineconv.hip) beside the project's own unfused forms on the same
device and operands.

  sparse   cfg4's graph: M = 262144 (512 graphs of 512 nodes), TemporalEdge([1, 2, 4]), F = 32, edge features D = 3
           from gcm.gine.RelativeEdgeAttr.  gcm.gine.GINEConv vs the same layer written out on gcm.nn.MessagePassing,
           which materialises lin(edge_attr) [E,F] and the messages [E,F].
  dense    cfg2's band through the dense twin: B = 256, N = 128, F = 32, D = 3.  gcm.gine.DenseGINEConv vs the torch form
           (masked broadcast + relu + sum over [B,N,N,F]).

`nn` is the identity on both sides: the aggregation and `lin` are what is timed, forward alone and forward + backward
(gradients to x, edge_attr, eps and lin).  Timed with device events after a warm-up; the two sides alternate round by
round in one process and the median (and minimum) of the rounds is reported, with the device launches of one call
counted by torch.profiler.  Prints one JSON object per (leg, mode) and writes them to --out (default
profiles/gine_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops, gine as GE, nn as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gine_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "50"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "7"))
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


def compare(leg, shape, mode, hip_fn, ref_fn):
    for fn in (hip_fn, ref_fn):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    n = {"hip": launches(hip_fn), "ref": launches(ref_fn)}
    t = {"hip": [], "ref": []}
    for _ in range(ROUNDS):                     # alternate: both sides see the same clocks and neighbours
        t["hip"].append(once(hip_fn))
        t["ref"].append(once(ref_fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    line = json.dumps({"bench": "gine_kbench", "shape": shape, "leg": leg, "mode": mode, "iters": ITERS,
                       "rounds": ROUNDS, "hip_us": round(med["hip"], 2), "ref_us": round(med["ref"], 2),
                       "hip_min_us": round(min(t["hip"]), 2), "ref_min_us": round(min(t["ref"]), 2),
                       "hip_launches": n["hip"], "ref_launches": n["ref"],
                       "ref_over_hip": round(med["ref"] / med["hip"], 3)})
    print(line, flush=True)
    lines.append(line)


class Identity(torch.nn.Identity):
    def __init__(self, in_features):
        super().__init__()
        self.in_features = in_features


class UnfusedGINE(G.MessagePassing):
    """GINEConv as one writes it on the base class: [E,F] edge projections and [E,F] messages in memory."""

    def __init__(self, conv):
        super().__init__(aggr="add")
        self.conv = conv

    def forward(self, x, edge_index, edge_attr):
        out = self.propagate(edge_index, x=x, edge_attr=self.conv.lin(edge_attr))
        return (1 + self.conv.eps) * x + out

    def message(self, x_j, edge_attr):
        return torch.relu(x_j + edge_attr)


def legs(leg, shape, hip, ref, leaves, g):
    a, b = hip().detach(), ref().detach()
    err = float((a - b).abs().max())
    assert err <= 1e-4 * float(b.abs().max()), err            # the two sides compute the same thing

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
    compare(leg, shape, "fwd", fwd(hip), fwd(ref))
    compare(leg, shape, "fwd+bwd", fb(hip), fb(ref))


F, D = 32, 3
rel = GE.RelativeEdgeAttr(pose_slice=slice(0, 2), time_scale=0.25)

# ---- sparse: cfg4's graph ----
Bg, n = 512, 512
M = Bg * n
t = torch.arange(n, device=dev)
src, dst = [], []
for h in (1, 2, 4):
    src.append(t[h:] - h), dst.append(t[h:])
src, dst = torch.cat(src), torch.cat(dst)
order = torch.argsort(dst * n + src)                          # (sink, source): the CSR order SparseGCM emits
src, dst = src[order], dst[order]
off = (torch.arange(Bg, device=dev) * n).view(Bg, 1)
ei = torch.stack([(src + off).reshape(-1), (dst + off).reshape(-1)]).contiguous()
ei.gcm_graph = _ops.GraphIndex(ei, _ops.ptr_from_sorted(ei[1].contiguous(), M), M,
                               batches=(torch.arange(Bg + 1, device=dev) * n, Bg, n))
x = torch.randn(M, F, device=dev, requires_grad=True)
ea = rel(x.detach(), ei).requires_grad_()
conv = GE.GINEConv(Identity(F), eps=0.1, train_eps=True, edge_dim=D).to(dev)
unfused = UnfusedGINE(conv)
g = torch.randn(M, F, device=dev)
legs("sparse_layer", f"cfg4 M{M} E{ei.shape[1]} F{F} D{D}", lambda: conv(x, ei, ea), lambda: unfused(x, ei, ea),
     [x, ea] + list(conv.parameters()), g)
del x, ea, g, ei

# ---- dense: cfg2's band ----
B, N = 256, 128
i, j = torch.arange(N, device=dev)[:, None], torch.arange(N, device=dev)[None, :]
adj = ((i - j == 1) | (i - j == 2) | (i - j == 4)).float().expand(B, N, N).contiguous()
x = torch.randn(B, N, F, device=dev, requires_grad=True)
ea = rel(x.detach(), adj).requires_grad_()
dconv = GE.DenseGINEConv(Identity(F), eps=0.1, train_eps=True, edge_dim=D).to(dev)
g = torch.randn(B, N, F, device=dev)


def torch_dense():
    msg = torch.relu(x.unsqueeze(1) + dconv.lin(ea))          # [B,N,N,F]
    return (1 + dconv.eps) * x + (adj.unsqueeze(-1) * msg).sum(2)


legs("dense_layer", f"cfg2 B{B} N{N} F{F} D{D}", lambda: dconv(x, adj, ea), torch_dense,
     [x, ea] + list(dconv.parameters()), g)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
