#!/usr/bin/env python3
"""cfg2's per-step loop, FORWARD only, captured as a HIP graph and replayed, in two forms:

  plain    `for t: mx, m = gcm(obs[t], m)` - with DenseGCM.rows_merge_captured the 128 step nodes are one
  foreign  `for t: mx, m = gcm(raw[t] * 2, m)` - a node between every two steps: nothing can merge, the chain of
           step nodes must cost what it cost before the switch existed

One JSON line per form: us per replay, us per step, and merge_stats() where the module has it (so the same file runs
on a tree from before the switch).  --label names the leg; GCM_MERGE_CAPTURED=0 is the switch-off leg, and
GCM_ABSORB_HEAD=0 the leg that merges the steps but keeps the rollout's head launch a node of its own (merge_stats
then reports head_absorbed: 0), and GCM_RUN_MFMA=0 the leg whose merged node runs its layers in the VALU form instead of
on the matrix cores (merge_stats then reports run_mfma: false).  Dev tool."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "graph-conv-memory_amd"))
import torch  # noqa: E402
import bench  # noqa: E402


def measure(form, dev, replays, repeats):
    c = bench.CONFIGS["cfg2"]
    mem, gnn, _ = bench.build_memory(dev, donate=True)
    obs = bench.make_obs(c, 0, dev)
    T = obs.shape[0]

    def loop():
        with torch.no_grad():
            h, outs = None, []
            for t in range(T):
                x = obs[t] * 2 if form == "foreign" else obs[t]
                mx, h = mem(x, h)
                outs.append(mx)
            return torch.stack(outs)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            loop()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loop()
    stats = None
    if hasattr(mem, "merge_stats"):   # (head=True: trees that can absorb the head launch say whether they did)
        if hasattr(mem, "rows_run_mfma"):   # (and which form the merged node's layers run in)
            stats = mem.merge_stats(head=True, form=True)
        else:
            stats = mem.merge_stats(head=True) if hasattr(mem, "rows_absorb_head") else mem.merge_stats()
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    best = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            graph.replay()
        b.record()
        torch.cuda.synchronize()
        best.append(a.elapsed_time(b) * 1e3 / replays)
    mem.check_flags()
    return {"form": form, "T": T, "us_per_replay": [round(v, 3) for v in best],
            "us_per_step_min": round(min(best) / T, 4), "merge_stats": stats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="branch")
    ap.add_argument("--replays", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for form in ("plain", "foreign"):
        r = measure(form, dev, args.replays, args.repeats)
        r["leg"] = args.label
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
