"""Plain-torch restatement of SparseGCM.rollout(x, reset=mask) and the cases its tests share.
TEST INFRASTRUCTURE ONLY: a Python loop per graph, runs on whatever device its tensors live on, differentiable, pinned
against oracle/ by tests/test_sparse_segments_cpu.py."""
import torch

from _sparse_window_restate import random_causal_state, reset_ref
from oracle import sparse as osp


def plan_ref(taus, reset):
    """-> (segments [(owner, first column, length, enters_empty)], vbase [B + 1]) in virtual-graph order."""
    B, t = reset.shape
    tl = [min(max(int(v), 0), t) for v in taus.tolist()]
    rs = reset.cpu()
    segs, vbase = [], [0]
    for b in range(B):
        cols = [s for s in range(tl[b]) if bool(rs[b, s])]
        bounds = [0] + cols + [tl[b]]
        for j in range(len(cols) + 1):
            segs.append((b, bounds[j], bounds[j + 1] - bounds[j], int(j > 0 or (len(cols) > 0 and cols[0] == 0))))
        vbase.append(len(segs))
    return segs, vbase


def _relabelled(adj, relabel, Bp):
    adj = adj.coalesce()
    idx, val = adj.indices(), adj.values()
    nb = relabel.to(idx.device)[idx[0]]
    keep = nb >= 0
    nidx = torch.stack([nb[keep], idx[1][keep], idx[2][keep]])
    return torch.sparse_coo_tensor(nidx, val[keep], size=(Bp,) + tuple(adj.shape[1:]))


def expand_ref(x, taus, hidden, reset):
    """-> (x' [B', t', F], taus' [B'], (nodes', adj', T'), (segments, vbase))."""
    segs, vbase = plan_ref(taus, reset)
    nodes, adj, T = hidden
    dev = x.device
    Bp, tp = len(segs), max([1] + [l for _, _, l, _ in segs])
    xs = x.new_zeros(Bp, tp, x.shape[-1])
    for v, (b, s, l, _) in enumerate(segs):
        if l:
            xs[v, :l] = x[b, s:s + l]
    taus_s = torch.tensor([l for _, _, l, _ in segs], dtype=torch.long, device=dev)
    zero = torch.zeros_like(nodes[0])
    nodes_s = torch.stack([zero if e else nodes[b] for b, _, _, e in segs])
    T_s = torch.stack([torch.zeros_like(T[0]) if e else T[b] for b, _, _, e in segs])
    relabel = torch.tensor([-1 if segs[vbase[b]][3] else vbase[b] for b in range(len(vbase) - 1)])
    return xs, taus_s, (nodes_s, _relabelled(adj, relabel, Bp), T_s), (segs, vbase)


def collect_ref(out_s, hidden_s, plan, B, t):
    """-> (out [B, t, H], (nodes, adj, T)): the outputs back in place, the last virtual graph of every b."""
    segs, vbase = plan
    nodes_s, adj_s, T_s = hidden_s
    out = out_s.new_zeros(B, t, out_s.shape[-1])
    for v, (b, s, l, _) in enumerate(segs):
        if l:
            out[b, s:s + l] = out_s[v, :l]
    last = torch.tensor([vbase[b + 1] - 1 for b in range(B)], device=nodes_s.device)
    final = torch.full((len(segs),), -1, dtype=torch.long)
    final[last.cpu()] = torch.arange(B)
    return out, (nodes_s[last], _relabelled(adj_s, final, B), T_s[last])


def stepwise_ref(x, taus, hidden, reset, gnn, graph_size, **kw):
    """One oracle call per column, reset_ref ahead of it where the mask says so (valid columns only)."""
    B, t, _ = x.shape
    if hidden is None:
        hidden = osp.initial_hidden(x, graph_size)
        hidden = (hidden[0].to(x.dtype), hidden[1], hidden[2])
    outs = []
    for s in range(t):
        live = s < taus
        hidden = reset_ref(hidden, reset[:, s] & live)
        if not bool(live.any()):
            outs.append(None)
            continue
        o, hidden = osp.sparse_step(x[:, s:s + 1], live.long(), hidden, gnn, graph_size=graph_size, **kw)
        outs.append(o)
    H = next(o for o in outs if o is not None).shape[-1]
    outs = [o if o is not None else x.new_zeros(B, 1, H) for o in outs]
    return torch.cat(outs, dim=1), hidden


def oneshot_ref(x, taus, hidden, reset, gnn, graph_size, **kw):
    """expand_ref -> one oracle call over the virtual graphs -> collect_ref."""
    B, t, _ = x.shape
    if hidden is None:
        hidden = osp.initial_hidden(x, graph_size)
        hidden = (hidden[0].to(x.dtype), hidden[1], hidden[2])
    xs, taus_s, hs, plan = expand_ref(x, taus, hidden, reset)
    out_s, hs2 = osp.sparse_step(xs, taus_s, hs, gnn, graph_size=graph_size, **kw)
    return collect_ref(out_s, hs2, plan, B, t)


# ---- the cases the CPU and the GPU tests share ----
# (B, N, F, t, density) of the kernel tests; the last one's stored list spans several 1024-entry chunks per graph
SHAPES = [(1, 1, 1, 1, 0.5), (3, 6, 4, 5, 0.5), (5, 33, 3, 7, 0.5), (4, 64, 8, 16, 0.5), (2, 200, 32, 40, 0.3)]
MASKS = ["none", "all", "column0", "last_valid", "random", "padding_only"]
# seeds of the random cases, chosen so that the drawn (taus, mask) has a graph with two or more valid resets, one with
# none and one with a valid reset in column 0 (tests/test_sparse_segments_cpu.py asserts it)
SEEDS = {(3, 5): 0, (5, 7): 0, (4, 16): 0, (2, 40): 62, (4, 12): 4}


def random_case(B, t, seed):
    """(taus [B] in [0, t], mask [B, t] with p = 0.3)."""
    gen = torch.Generator().manual_seed(seed)
    taus = torch.randint(0, t + 1, (B,), generator=gen)
    return taus, torch.rand(B, t, generator=gen) < 0.3


def mask_case(B, t, pattern):
    """(taus, mask) of a kernel test: ragged taus with a zero (B > 1) and a full graph."""
    taus, mask = random_case(B, t, SEEDS.get((B, t), 0))
    if pattern == "random":
        return taus, mask
    taus = taus.clone()
    taus[-1] = t
    if B > 1:
        taus[0] = 0
    mask = torch.zeros(B, t, dtype=torch.bool)
    if pattern == "all":
        mask[:] = True
    elif pattern == "column0":
        mask[:, 0] = True
    elif pattern == "last_valid":
        for b in range(B):
            if taus[b] > 0:
                mask[b, int(taus[b]) - 1] = True
    elif pattern == "padding_only":
        mask = torch.arange(t)[None, :] >= taus[:, None]
    return taus, mask


def valid_resets(taus, mask):
    return mask & (torch.arange(mask.shape[1])[None, :] < taus[:, None])


def stored_state(B, N, F, density, seed, kind="random"):
    """A stored hidden state for the kernel tests: `random` (one full graph), `empty_graphs` (T = 0 for some),
    `no_edges` (E = 0)."""
    gen = torch.Generator().manual_seed(seed + 17)
    T = torch.full((B,), N) if N == 200 else torch.randint(0, N + 1, (B,), generator=gen)
    T[-1] = N
    if kind == "empty_graphs":
        T[0] = 0
    return random_causal_state(B, N, F, 0.0 if kind == "no_edges" else density, T=T, seed=seed)
