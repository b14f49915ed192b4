#!/usr/bin/env python3
"""Micro-benchmark of the fused TransformerConv kernels with edge features (csrc/transformer_edge.hip) beside the
project's own unfused forms and beside the edge-free gcm.nn layers, on the same device and operands.

  sparse   cfg4's graph: M = 262144 (512 graphs of 512 nodes), TemporalEdge([1, 2, 4]), F = 32, H = 4, C = 8, D = 3
           from gcm.gine.RelativeEdgeAttr.  gcm.transformer.TransformerConv vs the same layer written out on
           gcm.nn.MessagePassing, which materialises q[i], k[j], v[j], lin_edge(edge_attr), the keys and the messages as
           [E, 32] arrays (and the scores [E, 4]).  gcm.nn.TransformerConv (no edge features) on the same graph is timed
           in the same rounds: the cost of the edge terms is the ratio hip / edge_free.
  dense    cfg2's band through the dense twin: B = 256, N = 128, same widths.  gcm.transformer.DenseTransformerConv vs
           the torch broadcast form over [B,N,N,H,C]; gcm.nn.DenseTransformerConv in the same rounds.

Forward alone and forward + backward (gradients to x, edge_attr and every parameter).  Timed with device events after a
warm-up; the sides alternate round by round in one process and the median (and minimum) of the rounds is reported, with
the device launches of one call counted by torch.profiler.  Prints one JSON object per (leg, mode) and writes them to
--out (default profiles/transformer_edge_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops, gine as GE, nn as G, transformer as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer_edge_kbench.jsonl"))
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
    """fns: {"hip": fused, "ref": unfused, "edge_free": the gcm.nn layer}; they alternate round by round."""
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
    rec = {"bench": "transformer_edge_kbench", "shape": shape, "leg": leg, "mode": mode, "iters": ITERS,
           "rounds": ROUNDS}
    for k in fns:
        rec.update({f"{k}_us": round(med[k], 2), f"{k}_min_us": round(min(t[k]), 2), f"{k}_launches": n[k]})
    rec["ref_over_hip"] = round(med["ref"] / med["hip"], 3)
    rec["hip_over_edge_free"] = round(med["hip"] / med["edge_free"], 3)         # what the edge terms cost
    rec["hip_median_below_ref_min"] = bool(med["hip"] < min(t["ref"]))          # the acceptance for speed
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


class UnfusedTransformer(G.MessagePassing):
    """TransformerConv(edge_dim) as one writes it on the base class (PyG's message body), sharing the fused layer's
    parameters."""

    def __init__(self, conv):
        super().__init__(aggr="add", node_dim=0)
        self.conv = conv

    def forward(self, x, edge_index, edge_attr):
        c = self.conv
        H, C = c.heads, c.out_channels
        q, k, v = (lin(x).view(-1, H, C) for lin in (c.lin_query, c.lin_key, c.lin_value))
        out = self.propagate(edge_index, query=q, key=k, value=v, e=c.lin_edge(edge_attr).view(-1, H, C))
        return out.reshape(-1, H * C) + c.lin_skip(x)

    def message(self, query_i, key_j, value_j, e, index, ptr, size_i):
        alpha = (query_i * (key_j + e)).sum(-1) / math.sqrt(self.conv.out_channels)
        alpha = G.softmax(alpha, index, ptr, size_i)
        return (value_j + e) * alpha.unsqueeze(-1)


def legs(leg, shape, sides, leaves, g):
    """sides: {"hip": f, "ref": f, "edge_free": f}; hip and ref must compute the same thing."""
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
ea = rel(x.detach(), ei).requires_grad_()
conv = T.TransformerConv(F, C, heads=H, edge_dim=D).to(dev)
plain = G.TransformerConv(F, C, heads=H).to(dev)
unfused = UnfusedTransformer(conv)
legs("sparse_layer", f"cfg4 M{M} E{ei.shape[1]} F{F} H{H} C{C} D{D}",
     {"hip": lambda: conv(x, ei, ea), "ref": lambda: unfused(x, ei, ea), "edge_free": lambda: plain(x, ei)},
     [x, ea] + list(conv.parameters()) + list(plain.parameters()), g)
del x, ea, g, ei

# ---- dense: cfg2's band ----
B, N = 256, 128
i, j = torch.arange(N, device=dev)[:, None], torch.arange(N, device=dev)[None, :]
adj = ((i - j == 1) | (i - j == 2) | (i - j == 4)).float().expand(B, N, N).contiguous()
x = torch.randn(B, N, F, device=dev, requires_grad=True)
ea = rel(x.detach(), adj).requires_grad_()
dconv = T.DenseTransformerConv(F, C, heads=H, edge_dim=D).to(dev)
dplain = G.DenseTransformerConv(F, C, heads=H).to(dev)
g = torch.randn(B, N, H * C, device=dev)
pat = (adj != 0).unsqueeze(-1)


def torch_dense():
    """The broadcast form: lin_edge(edge_attr), the keys and the messages are [B,N,N,H,C] tensors."""
    q, k, v = (lin(x).view(B, N, H, C) for lin in (dconv.lin_query, dconv.lin_key, dconv.lin_value))
    e = dconv.lin_edge(ea * pat).view(B, N, N, H, C)
    s = (q.unsqueeze(2) * (k.unsqueeze(1) + e)).sum(-1) / math.sqrt(C)
    alpha = torch.nan_to_num(torch.softmax(s.masked_fill(~pat, float("-inf")), dim=2))   # rows without a term: 0
    o = (alpha.unsqueeze(-1) * (v.unsqueeze(1) + e)).sum(2)
    return o.reshape(B, N, H * C) + dconv.lin_skip(x)


legs("dense_layer", f"cfg2 B{B} N{N} F{F} H{H} C{C} D{D}",
     {"hip": lambda: dconv(x, adj, ea), "ref": torch_dense, "edge_free": lambda: dplain(x, adj)},
     [x, ea] + list(dconv.parameters()) + list(dplain.parameters()), g)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
