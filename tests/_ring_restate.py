"""The column-write cached step (csrc/rows_colcache.hip) restated in plain torch, and the outlier cases that
tests/test_ring_conditioning_cpu.py and tests/test_ring_conditioning_gpu.py share.

The step keeps ONE layer-1 aggregate per stored node, agg1[j] = sum_k adj[j, k] x[k], and corrects it in place:
`+ x[cur]` for the rows that gain the new node as a source, and past graph_size steps `- x[dropped]` for the rows
that held the dropped node (the ring form).  Two forms of that bookkeeping, on the oracle module's own lin_rel /
lin_root with autograd:

  wide = False  "fp32 ring": the aggregates are kept by fp32 add and subtract, the new row's aggregate is a fresh fp32
                sum.  Once a large observation has been in a row's aggregate, the fp32 sum has rounded away about
                eps x |outlier| of the small terms; subtracting the outlier later removes it exactly and leaves that
                rounding error behind until the row itself is dropped.
  wide = True   "wide ring" (what the kernel does): the aggregates, the new row's sum and the corrections in float64,
                rounded to fp32 where the value enters the layer-1 product.  Sums of at most 128 fp32 values of
                magnitude <= 2^12 are exact in float64 to ~1e-13, so add-then-subtract leaves nothing behind.

Neither form reads the adjacency: like the kernel they follow the selectors by chain index."""
import torch

OUTLIER = 4096.0      # 2^12, on every third feature


def _sel(spec):
    from oracle import dense as od
    return od.DenseEdge() if spec[0] == "dense" else od.TemporalBackedge(spec[1], spec[2])


# name -> selector, B, N, F, H1, H2, T, outlier steps.  The smallest shapes at which each code path of the step can go
# wrong (see tests/test_ring_conditioning_gpu.py for which kernel each one reaches).
CASES = {}
for _F, _H1, _H2 in ((32, 32, 16), (32, 32, 48), (64, 32, 16), (32, 64, 16)):
    # N = 8: one tile; one outlier enters before the ring starts and leaves inside it, one lives in the steady state
    CASES[f"dense-N8-{_F}-{_H1}-{_H2}"] = (("dense",), 2, 8, _F, _H1, _H2, 48, (5, 25))
    # N = 36: crosses the 16-slot and the 32-slot tile edges
    CASES[f"dense-N36-{_F}-{_H1}-{_H2}"] = (("dense",), 2, 36, _F, _H1, _H2, 144, (41,))
# N = 68: crosses the 64-bit word of the row masks
CASES["dense-N68-32-32-16"] = (("dense",), 2, 68, 32, 32, 16, 212, (80,))
# a hop close to N: a row that lost the dropped node as a source is still read
CASES["both-2-7-N8"] = (("temporal", [2, 7], "both"), 2, 8, 32, 32, 32, 48, (5, 25))
# controls: nothing is ever subtracted / the ring of the forward-hop cached step
CASES["backward-1-3-N8"] = (("temporal", [1, 3], "backward"), 2, 8, 32, 32, 32, 48, (5, 25))
CASES["forward-1-2-4-N12"] = (("temporal", [1, 2, 4], "forward"), 2, 12, 32, 32, 32, 72, (5, 37))


def make_inputs(name, outlier=OUTLIER, seed=0):
    """-> (obs [T,B,F], quiet [T] bool, w [T,B,H2]): observations U(-0.5, 0.5) with +-outlier on every third feature
    at the case's outlier steps; quiet[t]: the window of step t (the last N observations) holds no outlier step;
    w: the loss weights, zero on the other steps.  The same draws for every value of `outlier`; seed: other draws."""
    spec, B, N, F, H1, H2, T, steps = CASES[name]
    gen = torch.Generator().manual_seed(1234 + N + F + 2 * H1 + 3 * H2 + 7919 * seed)
    obs = torch.rand(T, B, F, generator=gen) - 0.5
    w = torch.rand(T, B, H2, generator=gen)
    quiet = torch.ones(T, dtype=torch.bool)
    for s in steps:
        sign = torch.randint(0, 2, (B, len(range(0, F, 3))), generator=gen).float() * 2 - 1
        if outlier:
            obs[s, :, ::3] = sign * outlier
        quiet[s:s + N] = False
    return obs, quiet, w * quiet[:, None, None]


def make_modules(name, seed=0):
    """The oracle GNN of a case (its device twin: tests/test_ring_conditioning_gpu.py); seed: other initial weights."""
    from oracle import pyg
    spec, B, N, F, H1, H2, T, steps = CASES[name]
    torch.manual_seed(N + T + 7919 * seed)
    return pyg.Sequential("x, adj, weights, B, N", [
        (pyg.DenseGraphConv(F, H1), "x, adj -> x"), torch.nn.Tanh(),
        (pyg.DenseGraphConv(H1, H2), "x, adj -> x"), torch.nn.Tanh()])


def ring_rollout(ref, obs, graph_size, spec, wide):
    """The per-step loop from empty graphs as the column-write cached step evaluates it -> beliefs [T,B,H2]
    (differentiable in ref's parameters).  spec: ("dense",) | ("temporal", hops, direction)."""
    conv1, act1, conv2, act2 = ref.module_0, ref.module_1, ref.module_2, ref.module_3
    T, B, F = obs.shape
    N = graph_size
    acc = torch.float64 if wide else torch.float32
    agg, src, outs = {}, {}, []      # chain index of a stored node -> its aggregate [B,F] / the set of its sources
    for t in range(T):
        if t >= N:                   # the graph is full: its oldest node goes, and with it a source of some rows
            d = t - N
            del agg[d], src[d]
            for i, s in src.items():
                if d in s:
                    agg[i] = agg[i] - obs[d].to(acc)
                    s.discard(d)
        c = min(t, N - 1)            # the graph row the new node lands in
        new_src, gain = set(), set()
        if spec[0] == "dense":
            new_src = set(range(t - c, t + 1))
            gain = set(range(t - c, t))
        else:
            for h in spec[1]:
                if h > c:
                    continue
                if h == 0:
                    new_src.add(t)
                    continue
                if spec[2] in ("forward", "both"):
                    new_src.add(t - h)
                if spec[2] in ("backward", "both"):
                    gain.add(t - h)
        fresh = torch.zeros(B, F, dtype=acc)
        for k in sorted(new_src):
            fresh = fresh + obs[k].to(acc)
        agg[t], src[t] = fresh, set(new_src)
        for j in gain:
            agg[j] = agg[j] + obs[t].to(acc)
            src[j].add(t)
        live = sorted(new_src | {t})
        a = torch.stack([agg[k].float() for k in live], 1)       # rounded to fp32 where it is used
        xs = torch.stack([obs[k] for k in live], 1)
        h1 = act1(conv1.lin_rel(a) + conv1.lin_root(xs))
        m = torch.tensor([1.0 if k in new_src else 0.0 for k in live])
        agg2 = (h1 * m[None, :, None]).sum(1)
        outs.append(act2(conv2.lin_rel(agg2) + conv2.lin_root(h1[:, live.index(t)])))
    return torch.stack(outs)
