#!/usr/bin/env python3
"""Phase breakdown of the GEMM-form cached backward (csrc/rows_bptt_hops.hip: k_bptt_hops_graph_fold, and with --form
parent the kernel before the fold, k_bptt_hops_graph, behind gcm_dense_rows_bptt_cached_hops_unfolded) on the records of one
cfg2 rollout (B = 256, N = T = 128, F = H = 32, TemporalBackedge([1, 2, 4]), tanh / tanh - built through the C ABI as
tools/kbench_bptt_hops.py builds them) from in-kernel stamps of workgroup 0, wave 0 - in the folded form a layer-2 wave - and, folded form, wave 4, a layer-1 wave (diagnostic build:
make -C graph-conv-memory_amd/csrc stamps12).  Two libraries: the kernel as it ships with stamps at its phase edges,
and one that also waits for every load before it computes (the round trip alone).  Stamps are s_memtime ticks, shown
with each phase's share of the total.  Dev tool; --out appends the table as JSON lines."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "graph-conv-memory_amd", "gcm", "_lib")
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--form", default="fold", choices=["fold", "parent"])
ap.add_argument("--lib", default=None, help="(internal) one library per process: the stamps live in the library")
args = ap.parse_args()

if args.lib is None:   # one child per library (a process binds one libgcm_hip)
    for name in ("libgcm_hip_stamps12.so", "libgcm_hip_stamps12w.so"):
        if args.form == "fold" and name.endswith("12w.so"):
            continue   # (the waiting form is a mark of the unfolded kernel only)
        cmd = [sys.executable, os.path.abspath(__file__), "--form", args.form, "--lib", os.path.join(LIBDIR, name)]
        if args.out:
            cmd += ["--out", args.out]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            sys.exit(rc)
    sys.exit(0)

os.environ["GCM_HIP_LIB"] = args.lib
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import _hip  # noqa: E402

dev = "cuda:0"
B, N, T, H2, F, H1, HOPS = 256, 128, 128, 32, 32, 32, [1, 2, 4]
lib = _hip.lib()
p, st = _hip.ptr, _hip.stream()
waits = args.lib.endswith("12w.so")

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
                                        3 | _hip.STEP_IMG_V4, 1, 1, p(cH), p(cA), p(cX), p(saved[t]), 1, t, p(flags), B, N,
                                        F, H1, H2, st)
    assert rc == 0, (t, rc)
torch.cuda.synchronize()
assert int(flags.item()) == 0

g_mx = torch.full((T, B, H2), 1.0 / (T * B * H2), device=dev)
sv = (ctypes.c_void_p * T)(*[s.data_ptr() for s in saved])
gm = (ctypes.c_void_p * T)(*[g_mx[t].data_ptr() for t in range(T)])
cur = (ctypes.c_uint8 * T)(*range(T))
ws_bytes = 4 * P * B
ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
out = torch.empty(P, device=dev)
lib.gcm_debug_read_stamps.argtypes = [ctypes.c_void_p, ctypes.c_int]

FOLD_EDGES = [(0, 1, "layer-2 wave: stage, every load issued"),
              (1, 2, "layer-2 wave: wait for the step loads; D2 -> LDS; barrier"),
              (2, 3, "layer-2 wave: dW2 / db2 (32 MFMAs)"),
              (3, 5, "layer-2 wave: partial slab -> LDS; barrier"),
              (5, 6, "layer-2 wave: sum of four in wave order, slab stored"),
              (16, 17, "layer-1 wave: stage, every load issued"),
              (17, 18, "layer-1 wave: barrier (D2 of the layer-2 waves)"),
              (18, 19, "layer-1 wave: A operands read from sD2 and summed"),
              (19, 20, "layer-1 wave: tile product (32 MFMAs)"),
              (20, 21, "layer-1 wave: G1, dW1 / db1 (32 MFMAs)"),
              (21, 22, "layer-1 wave: partial slab -> LDS; barrier"),
              (22, 23, "layer-1 wave: sum of four in wave order, slab stored")]
EDGES = [(0, 1, "stage: every load issued"),
         (1, 2, "wait for the step loads; D2, dW2 / db2 (16 MFMAs), D2 -> LDS; barrier"),
         (2, 3, "U = D2 . [W_rel2 | W_root2] (16 MFMAs) -> LDS; barrier"),
         (3, 4, "gather, G1, dW1 / db1 (16 MFMAs); barrier"),
         (4, 5, "partial slabs -> LDS; barrier"),
         (5, 6, "sum of eight in wave order, slab stored")]


if args.form == "fold":
    EDGES = FOLD_EDGES
entry = lib.gcm_dense_rows_bptt_cached_hops if args.form == "fold" else lib.gcm_dense_rows_bptt_cached_hops_unfolded


def run():
    rc = entry(sv, gm, T, H2, 1, p(params), 3, 1, 1, p(cX), p(cH), p(cA), cur,
               ctypes.addressof(desc), 1, T, None, p(out), p(ws), ws_bytes, B, N, F, H1, H2, st)
    assert rc == 0, rc


lines = []
for form in (args.form,):
    R, acc, wait_acc = 20, [0.0] * len(EDGES), 0.0
    for it in range(R + 3):
        torch.cuda.synchronize()
        run()
        torch.cuda.synchronize()
        s = (ctypes.c_ulonglong * 32)()
        assert lib.gcm_debug_read_stamps(s, 32) == 0
        if it >= 3:
            for k, (a, b, _) in enumerate(EDGES):
                acc[k] += (s[b] - s[a]) / R
            if waits:
                wait_acc += (s[8] - s[1]) / R
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        run()
    e1.record()
    torch.cuda.synchronize()
    us_pair = e0.elapsed_time(e1) / 50 * 1e3
    total = sum(a_ for a_, (e0_, _, _) in zip(acc, EDGES) if e0_ < 16)   # (wave 0's edges: begin to end)
    print("k_bptt_hops_graph, %s%s: workgroup 0" % (form, " (waits for its loads before computing)" if waits else ""))
    for k, (a, b, name) in enumerate(EDGES):
        print("  %d -> %d  %-76s %8.1f ticks  %5.1f %%" % (a, b, name, acc[k], 100 * acc[k] / total))
    if waits:
        print("  inside 1 -> 2: the load round trip alone (1 -> vmcnt(0)) %8.1f ticks" % wait_acc)
    print("  total %8.1f ticks;  %.2f us per call (kernel + gcm_sum_slabs_acc), 50 back to back" % (total, us_pair))
    lines.append({"tool": "kstamp_bptt_hops", "form": form, "waits_for_loads": waits, "B": B, "N": N, "T": T, "H2": H2,
                  "ticks": {name: round(acc[k], 1) for k, (_, _, name) in enumerate(EDGES)},
                  "load_round_trip_ticks": round(wait_acc, 1) if waits else None, "total_ticks": round(total, 1),
                  "us_per_call_with_sum_slabs": round(us_pair, 3), "device": torch.cuda.get_device_name(0)})
if args.out:
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")
