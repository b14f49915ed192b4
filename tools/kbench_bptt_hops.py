#!/usr/bin/env python3
"""Micro-benchmark of cfg2's parameter backward: the record-walking kernel (gcm_dense_rows_bptt_cached:
k_bptt_cached_graph) against the GEMM form (csrc/rows_bptt_hops.hip) folded (gcm_dense_rows_bptt_cached_hops:
k_bptt_hops_graph_fold) and unfolded (gcm_dense_rows_bptt_cached_hops_unfolded: k_bptt_hops_graph) on the SAME records.  The records of one cfg2 rollout (B = 256, N = T = 128, F = H = 32, TemporalBackedge([1, 2, 4]),
tanh / tanh) are built through the C ABI with gcm_dense_rows_step_cached, as bench.py's time_step_kernel builds them
for the cached step; then each entry - its gcm_sum_slabs_acc launch included - is timed with device events around
KBENCH_ITERS back-to-back calls, the entries alternating round by round in one process; median and minimum of
the rounds.  Prints one JSON object per entry and writes them to --out (default
profiles/bptt_hops_kbench.jsonl).  Dev / reporting tool."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bptt_hops_kbench.jsonl"))
ap.add_argument("--B", type=int, default=256)
ap.add_argument("--N", type=int, default=128)
ap.add_argument("--T", type=int, default=128)
ap.add_argument("--H2", type=int, default=32)
args = ap.parse_args()

dev = "cuda:0"
ITERS = int(os.environ.get("KBENCH_ITERS", "50"))
ROUNDS = int(os.environ.get("KBENCH_ROUNDS", "9"))
B, N, T, H2, F, H1, HOPS = args.B, args.N, args.T, args.H2, 32, 32, [1, 2, 4]
IMG_V4 = _hip.STEP_IMG_V4
lib = _hip.lib()
p, st = _hip.ptr, _hip.stream()

g = torch.Generator().manual_seed(0)
P = lib.gcm_dense_gnn2_param_count(F, H1, H2)
params = (torch.randn(P, generator=g) * 0.2).to(dev)
obs = torch.rand(T, B, F, generator=g).to(dev)
img = torch.empty(lib.gcm_dense_rows_cached_weight_image_floats(), device=dev)
assert lib.gcm_dense_rows_cached_weight_image(p(params), p(img), F, H1, H2, st) == 0
lay = (ctypes.c_size_t * 5)()
assert lib.gcm_dense_rows_cached_layout(B, N, F, H1, H2, ctypes.addressof(lay)) == 0
d = _hip.SelectorDesc(kind=_hip.SEL_TEMPORAL, n_hops=len(HOPS), direction=_hip.DIR["forward"])
for i, h in enumerate(HOPS):
    d.hops[i] = h
desc = (_hip.SelectorDesc * 1)(d)
nodes, adj = torch.zeros(B, N, F, device=dev), torch.zeros(B, N, N, device=dev)
count = torch.zeros(B, dtype=torch.int64, device=dev)
cH, cA, cX = (torch.empty(B, N, w, device=dev) for w in (H1, F, F))
flags = torch.zeros(1, dtype=torch.int32, device=dev)
saved = [torch.empty(lay[0], device=dev) for _ in range(T)]
for t in range(T):
    rc = lib.gcm_dense_rows_step_cached(p(obs[t]), p(nodes), p(adj), p(count), ctypes.addressof(desc), 1, p(params), p(img),
                                        3 | IMG_V4, 1, 1, p(cH), p(cA), p(cX), p(saved[t]), 1, t, p(flags), B, N, F, H1,
                                        H2, st)
    assert rc == 0, (t, rc)
torch.cuda.synchronize()
assert int(flags.item()) == 0

g_mx = torch.full((T, B, H2), 1.0 / (T * B * H2), device=dev)
sv = (ctypes.c_void_p * T)(*[s.data_ptr() for s in saved])
gm = (ctypes.c_void_p * T)(*[g_mx[t].data_ptr() for t in range(T)])
cur = (ctypes.c_uint8 * T)(*range(T))
ws_bytes = max(lib.gcm_dense_rows_bptt_workspace_bytes(T, B, F, H1, H2), 4 * P * B)
ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
out = {k: torch.empty(P, device=dev) for k in ("walk", "unfolded", "hops")}


def walk():
    rc = lib.gcm_dense_rows_bptt_cached(sv, gm, T, H2, 1, p(params), 3, 1, 1, p(cX), p(cH), p(cA), None, p(out["walk"]),
                                        p(ws), ws_bytes, B, N, F, H1, H2, st)
    assert rc == 0, rc


def hops():
    rc = lib.gcm_dense_rows_bptt_cached_hops(sv, gm, T, H2, 1, p(params), 3, 1, 1, p(cX), p(cH), p(cA), cur,
                                             ctypes.addressof(desc), 1, T, None, p(out["hops"]), p(ws), ws_bytes, B, N, F,
                                             H1, H2, st)
    assert rc == 0, rc


def unfolded():
    rc = lib.gcm_dense_rows_bptt_cached_hops_unfolded(sv, gm, T, H2, 1, p(params), 3, 1, 1, p(cX), p(cH), p(cA), cur,
                                                      ctypes.addressof(desc), 1, T, None, p(out["unfolded"]), p(ws),
                                                      ws_bytes, B, N, F, H1, H2, st)
    assert rc == 0, rc


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(ITERS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / ITERS


legs = {"walk": walk, "unfolded": unfolded, "hops": hops}
for fn in legs.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
us = {k: [] for k in legs}
for _ in range(ROUNDS):
    for k, fn in legs.items():
        us[k].append(timed(fn))
scale = float(out["walk"].abs().max())
lines = []
for k, entry in (("walk", "gcm_dense_rows_bptt_cached"), ("unfolded", "gcm_dense_rows_bptt_cached_hops_unfolded"),
                 ("hops", "gcm_dense_rows_bptt_cached_hops")):
    diff = float((out["walk"] - out[k if k != "walk" else "hops"]).abs().max())
    lines.append({"bench": "bptt_hops_kbench", "entry": entry, "B": B, "N": N, "T": T, "F": F, "H1": H1, "H2": H2, "hops": HOPS,
                  "with": "gcm_sum_slabs_acc", "iters": ITERS, "rounds": ROUNDS,
                  "us_median": round(statistics.median(us[k]), 3), "us_min": round(min(us[k]), 3),
                  "max_abs_diff_over_scale": diff / scale, "device": torch.cuda.get_device_name(0)})
    print(json.dumps(lines[-1]))
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
