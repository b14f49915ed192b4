#!/usr/bin/env python3
"""Benchmark of DenseGCM.rollout with per-graph episode resets at cfg2's shape: B = 256 graphs of 128 nodes, F = H = 32,
TemporalBackedge([1, 2, 4]), T = 128, every entry of `reset` drawn true with probability 1/32 (fixed seed).  Forward +
backward (loss = sum of the beliefs, observations without gradient) of
  (a) mem.rollout(obs, reset=reset)        - the time-parallel forward of csrc/rollout_reset.hip
  (b) mem.rollout(obs)                     - the same call without resets (csrc/rollout_tp.hip)
  (c) the per-step loop `gcm(obs[t], m)` with donate_state=True and the three in-place edits
      `nodes[done] = 0; adj[done] = 0; num_nodes[done] = 0` ahead of every step that has a reset - the only way before
      rollout() took `reset` (which steps have one is known on the host up front: no read-back inside the loop)
timed with device events in alternating rounds (a, b, c, a, b, c, ...) after a warm-up of every leg; reports the
median of the rounds per leg, the spread, belief-states/s and the ratios (a)/(b), (c)/(a).  Before timing, (a) and (c)
are compared: same final state bit for bit, beliefs to 1e-5.  Prints one JSON object; --out appends it to a file.
Dev / reporting tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
from gcm import nn as G  # noqa: E402
from gcm.edge_selectors.temporal import TemporalBackedge  # noqa: E402
from gcm.gcm import DenseGCM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=int(os.environ.get("KBENCH_ROUNDS", "7")))
ap.add_argument("--iters", type=int, default=int(os.environ.get("KBENCH_ITERS", "20")))
ap.add_argument("--out", default=None)
args = ap.parse_args()

B, N, F, H, T, P_RESET = 256, 128, 32, 32, 128, 1.0 / 32
dev = "cuda:0"
torch.manual_seed(0)


def make(donate):
    torch.manual_seed(1)
    g = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(F, H), "x, adj -> x"), torch.nn.Tanh(),
                                               (G.DenseGraphConv(H, H), "x, adj -> x"), torch.nn.Tanh()]).to(dev)
    return g, DenseGCM(g, edge_selectors=TemporalBackedge([1, 2, 4]), graph_size=N, donate_state=donate)


obs = torch.rand(T, B, F, device=dev)
reset_cpu = torch.rand(T, B, generator=torch.Generator().manual_seed(2)) < P_RESET
reset = reset_cpu.to(dev)
steps_with_reset = reset_cpu.any(1).tolist()
g_r, mem_r = make(False)
g_l, mem_l = make(True)


def leg_a():
    out, hid = mem_r.rollout(obs, reset=reset)
    out.sum().backward()
    return out, hid


def leg_b():
    out, hid = mem_r.rollout(obs)
    out.sum().backward()
    return out, hid


def leg_c():
    hid, outs = None, []
    for t in range(T):
        if steps_with_reset[t] and hid is not None:
            done = reset[t]
            hid[0][done] = 0
            hid[1][done] = 0
            hid[3][done] = 0
        mx, hid = mem_l(obs[t], hid)
        outs.append(mx)
    out = torch.stack(outs)
    out.sum().backward()
    return out, hid


def timed(fn, iters):
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return a.elapsed_time(e) / iters * 1e3      # us per call


# results must not change: (a) against (c) on the same inputs
(oa, ha), (oc, hc) = leg_a(), leg_c()
assert all(torch.equal(x, y) for x, y in zip((ha[0], ha[1], ha[3]), (hc[0], hc[1], hc[3]))), "final states differ"
max_diff = float((oa.detach() - oc.detach()).abs().max())
assert max_diff <= 1e-5, max_diff
mem_r.check_flags()
mem_l.check_flags()

legs = {"rollout_reset": (leg_a, args.iters), "rollout": (leg_b, args.iters), "step_loop_edits": (leg_c, max(2, args.iters // 5))}
for fn, _ in legs.values():                     # warm-up of every leg
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in legs}
for _ in range(args.rounds):                    # alternating rounds
    for k, (fn, iters) in legs.items():
        times[k].append(timed(fn, iters))
med = {k: statistics.median(v) for k, v in times.items()}
res = {"bench": "rollout_reset_kbench", "B": B, "N": N, "F": F, "H": H, "T": T, "hops": [1, 2, 4], "p_reset": P_RESET,
       "resets": int(reset_cpu.sum()), "steps_with_reset": int(sum(steps_with_reset)), "rounds": args.rounds,
       "iters": args.iters, "max_abs_diff_a_vs_c": max_diff}
for k, v in times.items():
    res[k + "_us"] = round(med[k], 1)
    res[k + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
    res[k + "_M_belief_states_per_s"] = round(B * T / med[k], 2)
res["ratio_reset_over_plain"] = round(med["rollout_reset"] / med["rollout"], 3)
res["ratio_loop_over_reset"] = round(med["step_loop_edits"] / med["rollout_reset"], 2)
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
