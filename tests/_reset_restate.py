"""Expected values of DenseGCM.rollout(reset=...) / DenseGCM.reset_hidden from the oracle, without changing it: the
per-step loop over oracle.dense.dense_step with the state of the masked graphs multiplied by zero (out of place, so
autograd sees it) before the step, the same computation per episode (every episode of every graph on its own from
hidden = None), and the project's float64 tolerance rule (tests/_golden.py:fp64_rollout_bounds) restated over it."""
import copy

import torch

from oracle import dense as od


def clear_graphs(hidden, mask):
    """hidden with the graphs of mask [B] (bool) emptied: nodes, adj, weights, count times zero, out of place."""
    nodes, adj, weights, count = hidden
    keep = (~mask).to(nodes.dtype)[:, None, None]
    return (nodes * keep, adj * keep, weights * keep if weights.numel() else weights, count * (~mask).to(count.dtype))


def reset_rollout(obs, reset, hidden, ref, **kw):
    """T calls of dense_step over obs [T, B, F]; reset [T, B] (bool): graph b is emptied BEFORE obs[t, b] is inserted.
    -> (stack of mx [T, B, H], hidden)."""
    out = []
    for t in range(obs.shape[0]):
        if hidden is not None and bool(reset[t].any()):
            hidden = clear_graphs(hidden, reset[t])
        mx, hidden = od.dense_step(obs[t], hidden, ref, **kw)
        out.append(mx)
    return torch.stack(out), hidden


def per_episode_rollout(obs, reset, ref, graph_size, sel_factory):
    """The same from hidden = None with every episode of every graph run on its own (B = 1, hidden = None at its first
    step): -> (mx [T, B, H], final hidden).  Per-graph selectors only (no cross-batch EuclideanEdge)."""
    T, B = reset.shape
    outs, finals = [[None] * B for _ in range(T)], []
    for b in range(B):
        starts = [0] + [t for t in range(1, T) if bool(reset[t, b])]
        for s, e in zip(starts, starts[1:] + [T]):
            mx, hid = od.dense_rollout(obs[s:e, b:b + 1], None, ref, graph_size=graph_size,
                                       edge_selectors=sel_factory())
            for t in range(s, e):
                outs[t][b] = mx[t - s, 0]
        finals.append(hid)
    out = torch.stack([torch.stack(row) for row in outs])
    hidden = tuple(torch.cat([h[i] for h in finals]) if finals[0][i].numel() else finals[0][i] for i in range(4))
    return out, hidden


def fp64_reset_bounds(ref, obs, reset, hidden, weight, sel_factory, graph_size, factor=3.0, floor=5e-7):
    """tests/_golden.py:fp64_rollout_bounds over reset_rollout: the oracle in fp32 and in float64, loss =
    sum(out * weight) -> (out32, final hidden32, {param name: (g64, atol)}, (out64, out_atol)) with
    atol = max(factor x |oracle fp32 - oracle fp64|, floor x scale), 2e-6 as the floor of the beliefs.  obs with
    requires_grad (a leaf without a gradient yet): the same bound for its gradient, under "obs"."""
    ref.zero_grad(set_to_none=True)
    h32 = None if hidden is None else tuple(t.clone() for t in hidden)
    out32, hid32 = reset_rollout(obs, reset, h32, ref, graph_size=graph_size, edge_selectors=sel_factory())
    (out32 * weight).sum().backward()
    ref64 = copy.deepcopy(ref).double()
    ref64.zero_grad(set_to_none=True)
    h64 = None if hidden is None else tuple(t.double() if t.is_floating_point() else t.clone() for t in hidden)
    obs64 = obs.detach().double().requires_grad_(obs.requires_grad)
    out64, _ = reset_rollout(obs64, reset, h64, ref64, graph_size=graph_size, edge_selectors=sel_factory())
    (out64 * weight.double()).sum().backward()
    pairs = list(zip(ref.named_parameters(), ref64.named_parameters()))
    if obs.requires_grad:
        pairs.append((("obs", obs), ("obs", obs64)))
    bounds = {}
    for (k, p32), (_, p64) in pairs:
        scale = float(p64.grad.abs().max())
        err = float((p32.grad.double() - p64.grad).abs().max())
        bounds[k] = (p64.grad, max(factor * err, floor * scale))
    err_o = float((out32.detach().double() - out64.detach()).abs().max())
    return out32.detach(), tuple(t.detach() for t in hid32), bounds, (out64.detach(), max(2e-6, factor * err_o))
