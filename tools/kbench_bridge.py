#!/usr/bin/env python3
"""Micro-benchmark of the dense <-> sparse bridge (csrc/dense_sparse.hip) beside its torch form, in one process on one
device, at cfg2's shape: B = 256 graphs of N = 128 nodes, F = 32, with the two adjacencies a full memory holds there -
the band of TemporalBackedge([1, 2, 4]) (E = 96 512) and DenseEdge's triangle (E = 2 080 768).

  dense_to_sparse   gcm.gcm.DenseToSparse (edge list + the attached GraphIndex with its CSC view: three kernels and the
                    host read of E) against what the parent commit would run for the same result: torch.nonzero, the
                    offsets and the stack of the reference, GraphIndex.from_edge_index (a device-wide stable sort) and
                    its csc() (a second sort)
  sparse_to_dense   gcm.gcm.SparseToDense on the attached index against the scatter form (index_put, accumulate=True,
                    which adds with float atomics on a device)

Both sides of dense_to_sparse read E back, so a call is timed with the host clock around ITERS calls that end in a
device synchronise; the two sides alternate round by round after a warm-up and the median, minimum and maximum of the
rounds are reported.  "launches" counts the device activities (kernels, copies, memsets) of one call in a profiler
pass of its own, outside the timed windows; "hip_device_us" lists them with their device time, in order.  Prints one JSON object per (adjacency, leg) and writes them to --out
(default profiles/bridge_kbench.jsonl).  Dev / reporting tool."""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _ops  # noqa: E402
from gcm.gcm import DenseToSparse, SparseToDense  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bridge_kbench.jsonl"))
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "30"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "7"))
B, N, F = 256, 128, 32
lines = []


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS * 1e6     # us per call


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        evs = sorted((e for e in prof.events() if e.device_time_total > 0), key=lambda e: e.time_range.start)
        def short(name):    # "void (anonymous namespace)::k_bridge_image<float>(...)" -> "k_bridge_image"
            m = re.search(r"\bk_[a-z0-9_]+", name)
            return m.group(0) if m else name[:40].strip()
        return len(evs), [(short(e.name), round(e.device_time_total, 2)) for e in evs]
    except Exception:       # (a box without the tracer: the figures are then absent, not guessed)
        return None, None


def compare(shape, leg, hip_fn, torch_fn):
    for fn in (hip_fn, torch_fn):
        for _ in range(5):
            fn()
    t = {"hip": [], "torch": []}
    for _ in range(ROUNDS):                     # alternate: both sides see the same clocks and neighbours
        t["hip"].append(once(hip_fn))
        t["torch"].append(once(torch_fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    (hip_n, hip_kernels), (torch_n, _) = launches(hip_fn), launches(torch_fn)
    rec = {"bench": "bridge_kbench", "shape": shape, "leg": leg, "iters": ITERS, "rounds": ROUNDS,
           "hip_us": round(med["hip"], 2), "torch_us": round(med["torch"], 2),
           "hip_min_us": round(min(t["hip"]), 2), "hip_max_us": round(max(t["hip"]), 2),
           "torch_min_us": round(min(t["torch"]), 2), "torch_max_us": round(max(t["torch"]), 2),
           "torch_over_hip": round(med["torch"] / med["hip"], 3),
           "hip_launches": hip_n, "torch_launches": torch_n, "hip_device_us": hip_kernels}
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)


def torch_dense_to_sparse(x, adj, transpose):
    """The reference's module (src/gcm/gcm.py:44-53) and the index the layers behind it would build."""
    offset, row, col = torch.nonzero(adj > 0).t()
    row = row + offset * N
    col = col + offset * N
    edge_index = torch.stack([col, row] if transpose else [row, col], dim=0).long()
    x_sp = x.view(B * N, x.shape[-1])
    batch_idx = torch.arange(0, B, device=x.device).view(-1, 1).repeat(1, N).view(-1)
    graph = _ops.GraphIndex.from_edge_index(edge_index, B * N)
    graph.csc()
    edge_index.gcm_graph = graph
    return x_sp, edge_index, batch_idx


i = torch.arange(N, device=dev)
band = torch.zeros(N, N, device=dev)
for h in (1, 2, 4):
    band[i[h:], i[h:] - h] = 1.0
triangle = (i.view(-1, 1) > i.view(1, -1)).float()
x = torch.randn(B, N, F, device=dev)

with torch.no_grad():
    for name, one in (("TemporalBackedge([1,2,4]) band", band), ("DenseEdge triangle", triangle)):
        adj = one.expand(B, N, N).contiguous()
        for transpose in (True, False):
            bridge = DenseToSparse(transpose=transpose)
            got, want = bridge(x, adj), torch_dense_to_sparse(x, adj, transpose)
            assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])        # the same list ...
            g, w = got[1].gcm_graph, want[1].gcm_graph
            assert torch.equal(g.row_ptr, w.row_ptr) and torch.equal(g.col, w.col)      # ... and the same index
            assert all(torch.equal(a, b) for a, b in zip(g.csc(), w.csc()))
            shape = f"{name}: B={B} N={N} E={got[1].shape[1]}"
            compare(shape, f"dense_to_sparse(transpose={transpose}) + index",
                    lambda: bridge(x, adj), lambda: torch_dense_to_sparse(x, adj, transpose))
        x_sp, ei, batch = DenseToSparse(transpose=True)(x, adj)
        back, scatter = SparseToDense(), SparseToDense._torch_forward
        a, b = back(x_sp, ei, batch, B, N), scatter(x_sp, ei, batch, B, N, None)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        compare(f"{name}: B={B} N={N} E={ei.shape[1]} F={F}", "sparse_to_dense",
                lambda: back(x_sp, ei, batch, B, N), lambda: scatter(x_sp, ei, batch, B, N, None))

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
