#!/usr/bin/env python3
"""Micro-benchmark of the fused GATv2 kernels (csrc/gatv2conv.hip) beside the project's own unfused forms on the same
device and operands.

  sparse   cfg4's graph: M = 262144 (512 graphs of 512 nodes), TemporalEdge([1, 2, 4]), F = 32, H = 4, C = 8; once
           without edge features and once with D = 3 from gcm.gine.RelativeEdgeAttr.  gcm.gatv2.GATv2Conv vs the same
           layer written out on gcm.nn.MessagePassing, which materialises x_l[j], x_r[i], lin_edge(edge_attr), the
           pre-activations and the messages as [E, 32] arrays (and the scores [E, 4]).  For context only, gcm.nn.GATConv
           (GAT v1: per-node scores, no edge features) on the same graph is timed in the same rounds.
  dense    cfg2's band through the dense twin: B = 256, N = 128, same widths, D = 3.  gcm.gatv2.DenseGATv2Conv vs the
           torch broadcast form over [B,N,N,H,C].

Forward alone and forward + backward (gradients to x, edge_attr and every parameter).  Timed with device events after a
warm-up; the sides alternate round by round in one process and the median (and minimum) of the rounds is reported, with
the device launches of one call counted by torch.profiler.  Prints one JSON object per (leg, mode) and writes them to
--out (default profiles/gatv2_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops, gatv2 as GV, gine as GE, nn as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gatv2_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "30"))
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


def compare(leg, shape, mode, fns):
    """fns: {"hip": fused, "ref": unfused, further sides for context}; they alternate round by round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    n = {k: launches(fn) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):                     # alternate: every side sees the same clocks and neighbours
        for k, fn in fns.items():
            t[k].append(once(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    rec = {"bench": "gatv2_kbench", "shape": shape, "leg": leg, "mode": mode, "iters": ITERS, "rounds": ROUNDS}
    for k in fns:
        rec.update({f"{k}_us": round(med[k], 2), f"{k}_min_us": round(min(t[k]), 2), f"{k}_launches": n[k]})
    rec["ref_over_hip"] = round(med["ref"] / med["hip"], 3)
    rec["hip_median_below_ref_min"] = bool(med["hip"] < min(t["ref"]))          # the acceptance for speed
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


class UnfusedGATv2(G.MessagePassing):
    """GATv2Conv (add_self_loops=False) as one writes it on the base class, sharing the fused layer's parameters."""

    def __init__(self, conv):
        super().__init__(aggr="add", node_dim=0)
        self.conv = conv

    def forward(self, x, edge_index, edge_attr=None):
        c = self.conv
        H, C = c.heads, c.out_channels
        x_l, x_r = c.lin_l(x).view(-1, H, C), c.lin_r(x).view(-1, H, C)
        e = None if c.lin_edge is None else c.lin_edge(edge_attr).view(-1, H, C)
        out = self.propagate(edge_index, x=(x_l, x_r), e=e)
        return out.reshape(-1, H * C) + c.bias

    def message(self, x_j, x_i, e, index, ptr, size_i):
        z = x_i + x_j if e is None else x_i + x_j + e
        z = torch.nn.functional.leaky_relu(z, self.conv.negative_slope)
        alpha = G.softmax((z * self.conv.att).sum(dim=-1), index, ptr, size_i)
        return x_j * alpha.unsqueeze(-1)


def legs(leg, shape, sides, leaves, g):
    """sides: {"hip": f, "ref": f, ...}; hip and ref must compute the same thing."""
    a, b = sides["hip"]().detach(), sides["ref"]().detach()
    err = float((a - b).abs().max())
    assert err <= 1e-4 * float(b.abs().max()), err

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
    compare(leg, shape, "fwd", {k: fwd(f) for k, f in sides.items()})
    compare(leg, shape, "fwd+bwd", {k: fb(f) for k, f in sides.items()})


F, H, C, D = 32, 4, 8, 3
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
g = torch.randn(M, H * C, device=dev)
gat = G.GATConv(F, C, heads=H, add_self_loops=False).to(dev)
for edge_dim in (None, D):
    ea = None if edge_dim is None else rel(x.detach(), ei).requires_grad_()
    conv = GV.GATv2Conv(F, C, heads=H, add_self_loops=False, edge_dim=edge_dim).to(dev)
    unfused = UnfusedGATv2(conv)
    legs("sparse_layer" if edge_dim is None else "sparse_layer_edge_attr",
         f"cfg4 M{M} E{ei.shape[1]} F{F} H{H} C{C} D{edge_dim or 0}",
         {"hip": lambda: conv(x, ei, ea), "ref": lambda: unfused(x, ei, ea), "gat_v1": lambda: gat(x, ei)},
         [x] + ([] if ea is None else [ea]) + list(conv.parameters()) + list(gat.parameters()), g)
del x, ea, g, ei

# ---- dense: cfg2's band ----
B, N = 256, 128
i, j = torch.arange(N, device=dev)[:, None], torch.arange(N, device=dev)[None, :]
adj = ((i - j == 1) | (i - j == 2) | (i - j == 4)).float().expand(B, N, N).contiguous()
x = torch.randn(B, N, F, device=dev, requires_grad=True)
ea = rel(x.detach(), adj).requires_grad_()
dconv = GV.DenseGATv2Conv(F, C, heads=H, edge_dim=D).to(dev)
g = torch.randn(B, N, H * C, device=dev)
eye = torch.eye(N, device=dev, dtype=torch.bool)
pat = (adj != 0) | eye                                         # add_loop: the diagonal is a term


def torch_dense():
    """The broadcast form with the "mean" loop feature: every [B,N,N,H,C] tensor is written out."""
    x_l, x_r = dconv.lin_l(x).view(B, N, H, C), dconv.lin_r(x).view(B, N, H, C)
    a = ea * (adj != 0).unsqueeze(-1)
    loop = a.sum(2) / (adj != 0).sum(2).clamp(min=1).unsqueeze(-1)
    a = a + eye.view(1, N, N, 1) * loop.unsqueeze(2)
    z = x_l.unsqueeze(1) + x_r.unsqueeze(2) + dconv.lin_edge(a).view(B, N, N, H, C)
    s = (torch.nn.functional.leaky_relu(z, dconv.negative_slope) * dconv.att.view(1, 1, 1, H, C)).sum(-1)
    alpha = torch.softmax(s.masked_fill(~pat.unsqueeze(-1), float("-inf")), dim=2)
    return torch.einsum("bijh,bjhc->bihc", alpha, x_l).reshape(B, N, H * C) + dconv.bias


legs("dense_layer", f"cfg2 B{B} N{N} F{F} H{H} C{C} D{D}", {"hip": lambda: dconv(x, adj, ea), "ref": torch_dense},
     [x, ea] + list(dconv.parameters()), g)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
