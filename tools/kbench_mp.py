#!/usr/bin/env python3
"""Micro-benchmark of the message-passing primitives (csrc/message_passing.hip) beside the eager torch op each one
replaces, on the same device and tensors, at cfg4's one-shot shape: 512 graphs x 512 nodes (M = 262 144), C = 32,
with TemporalEdge([1]) edges (E = 261 632) and the [1, 2, 4] list (E = 782 848), in CSR order with the kind of index
SparseGCM attaches (built once, its CSC view too).

  gather_j / gather_i   gcm._ops.mp_gather            against x[idx]            (backward: index_add_)
  reduce sum / mean     gcm._ops.mp_reduce            against index_add_        (mean: / count)
  reduce max            gcm._ops.mp_reduce            against scatter_reduce("amax", include_self=False)
  softmax               gcm._ops.mp_softmax           against a sort-free softmax written out (scatter amax, exp,
                                                      index_add_, divide)
  graphconv             a GraphConv written as a gcm.nn.MessagePassing subclass against gcm.nn.GraphConv (fused), same
                        weights

Forward alone and forward + backward, timed with device events after a warm-up; the two sides alternate round by round
in one process and the median, minimum and maximum of the rounds are reported.  "eff_GBps" is the forward's bytes
(rows read + rows written + index) over its median time: an EFFECTIVE rate - these working sets (33 - 100 MB a tensor)
fit the 256 MB Infinity Cache, so it is no HBM bandwidth.  Prints one JSON object per (shape, leg, mode) and writes
them to --out (default profiles/mp_kbench.jsonl).  Two more shapes frame the figures: the same reduce on 8 rows (the
host floor of a forward + backward through torch's autograd engine) and a skewed list (1024 sinks of degree 512 beside
degree-1 sinks).  Dev / reporting tool."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mp_kbench.jsonl"))
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


def compare(shape, leg, mode, hip_fn, eager_fn, nbytes=None):
    for fn in (hip_fn, eager_fn):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {"hip": [], "eager": []}
    for _ in range(ROUNDS):                     # alternate: both sides see the same clocks and neighbours
        t["hip"].append(once(hip_fn))
        t["eager"].append(once(eager_fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    rec = {"bench": "mp_kbench", "shape": shape, "leg": leg, "mode": mode, "iters": ITERS, "rounds": ROUNDS,
           "hip_us": round(med["hip"], 2), "eager_us": round(med["eager"], 2),
           "hip_min_us": round(min(t["hip"]), 2), "hip_max_us": round(max(t["hip"]), 2),
           "eager_min_us": round(min(t["eager"]), 2), "eager_max_us": round(max(t["eager"]), 2),
           "eager_over_hip": round(med["eager"] / med["hip"], 3)}
    if nbytes is not None:
        rec["hip_eff_GBps"] = round(nbytes / med["hip"] * 1e-3, 1)
        rec["eager_eff_GBps"] = round(nbytes / med["eager"] * 1e-3, 1)
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def legs(shape, leg, hip, eager, leaves, g, nbytes=None, tol=1e-4):
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
    assert err <= tol * max(1.0, float(b.detach().abs().max())), (leg, err)     # the two sides compute the same thing
    compare(shape, leg, "fwd", fwd(hip), fwd(eager), nbytes)
    compare(shape, leg, "fwd+bwd", fb(hip), fb(eager))


class GraphConvMP(G.MessagePassing):
    """gcm.nn.GraphConv's parameters and formula, written the PyG way."""

    def __init__(self, in_channels, out_channels):
        super().__init__(aggr="add")
        self.lin_rel = torch.nn.Linear(in_channels, out_channels)
        self.lin_root = torch.nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, x, edge_index):
        return self.lin_rel(self.propagate(edge_index, x=x)) + self.lin_root(x)


Bg, Ns, C = 512, 512, 32
M = Bg * Ns
n = torch.arange(M, device=dev)
node_off = torch.arange(Bg + 1, device=dev) * Ns
x = torch.randn(M, C, device=dev, requires_grad=True)
g_m = torch.randn(M, C, device=dev)


def bench_list(shape, ei, batches, full):
    """Every primitive over the CSR-ordered list ei [2, E]; full: the gathers and the GraphConv pair as well."""
    E = ei.shape[1]
    graph = _ops.GraphIndex(ei, _ops.ptr_from_sorted(ei[1].contiguous(), M), M, batches=batches)
    ei.gcm_graph = graph
    by_sink = _ops.Segments.by_sink(graph)                                                # built once
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    dst_c = dst.unsqueeze(-1).expand(-1, C)
    rows = torch.randn(E, C, device=dev, requires_grad=True)
    g_e = torch.randn(E, C, device=dev)
    count = torch.bincount(dst, minlength=M).clamp(min=1).unsqueeze(-1).float()
    row_b, out_b, idx_b = E * C * 4, M * C * 4, E * 8

    if full:
        by_source = _ops.Segments.by_source(graph)
        legs(shape, "gather_j", lambda: _ops.mp_gather(x, by_source), lambda: x[src], [x], g_e, 2 * row_b + idx_b)
        legs(shape, "gather_i", lambda: _ops.mp_gather(x, by_sink), lambda: x[dst], [x], g_e, 2 * row_b + idx_b)
    legs(shape, "reduce_sum", lambda: _ops.mp_reduce(rows, by_sink, "sum"),
         lambda: torch.zeros(M, C, device=dev).index_add_(0, dst, rows), [rows], g_m, row_b + out_b + (M + 1) * 8)
    legs(shape, "reduce_mean", lambda: _ops.mp_reduce(rows, by_sink, "mean"),
         lambda: torch.zeros(M, C, device=dev).index_add_(0, dst, rows) / count, [rows], g_m,
         row_b + out_b + (M + 1) * 8)
    legs(shape, "reduce_max", lambda: _ops.mp_reduce(rows, by_sink, "max"),
         lambda: torch.zeros(M, C, device=dev).scatter_reduce(0, dst_c, rows, "amax", include_self=False), [rows], g_m,
         row_b + out_b + (M + 1) * 8)

    def eager_softmax():
        top = torch.full((M, C), float("-inf"), device=dev).scatter_reduce(0, dst_c, rows.detach(), "amax")
        p = torch.exp(rows - top[dst])
        return p / torch.zeros(M, C, device=dev).index_add_(0, dst, p)[dst]

    legs(shape, "softmax", lambda: _ops.mp_softmax(rows, by_sink), eager_softmax, [rows], g_e,
         2 * row_b + (M + 1) * 8)

    if full:
        torch.manual_seed(1)
        sub, fused = GraphConvMP(C, C).to(dev), G.GraphConv(C, C).to(dev)
        fused.load_state_dict(sub.state_dict())
        params = list(sub.parameters()) + list(fused.parameters())
        legs(shape, "graphconv_subclassed_vs_fused(eager=fused)", lambda: sub(x, ei), lambda: fused(x, ei),
             [x] + params, g_m, tol=1e-3)


# the host floor of one forward + backward through torch's autograd engine: the same calls on 8 rows, where no kernel
# takes longer than its launch - what the fwd+bwd legs below cannot go under, whatever the kernels do
tiny = torch.randn(8, C, device=dev, requires_grad=True)
tiny_dst = torch.arange(8, device=dev)
tiny_seg = _ops.Segments(tiny_dst, torch.arange(9, device=dev), None, 8)
legs("host floor M=8 E=8 C=32", "reduce_sum", lambda: _ops.mp_reduce(tiny, tiny_seg, "sum"),
     lambda: torch.zeros(8, C, device=dev).index_add_(0, tiny_dst, tiny), [tiny], torch.randn(8, C, device=dev))

for hops in ([1], [1, 2, 4]):
    # node i of every graph receives i - h: sorted by (sink, source), as SparseGCM's flat list
    cols = [torch.stack([n[n % Ns >= h] - h, n[n % Ns >= h]]) for h in hops]
    ei = torch.cat(cols, 1)
    ei = ei[:, torch.argsort(ei[1] * M + ei[0])].contiguous()
    bench_list(f"cfg4-oneshot hops={hops} M={M} E={ei.shape[1]} C={C}", ei, (node_off, Bg, Ns), True)

# skew: 1024 hub sinks with 512 in-edges each beside 261 120 sinks with one - about the [1, 2, 4] list's size, but a
# hub's segment is walked serially by the 8 lanes of its row
hubs = torch.arange(1024, device=dev) * 256
deg = torch.ones(M, dtype=torch.long, device=dev)
deg[hubs] = 512
sk_dst = torch.repeat_interleave(n, deg)
sk = torch.stack([torch.randint(0, M, (sk_dst.numel(),), device=dev), sk_dst]).contiguous()
bench_list(f"skewed 1024 sinks of degree 512, the others 1: M={M} E={sk.shape[1]} C={C}", sk, None, False)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
