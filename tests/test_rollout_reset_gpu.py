"""Per-graph episode resets: DenseGCM.rollout(obs, reset=...) - time-parallel from empty graphs with forward temporal
hops (csrc/rollout_reset.hip), the per-step loop with one masked clear per step that has a reset for everything else
(gcm_state_reset) - and DenseGCM.reset_hidden, against the oracle's per-step loop with the masked graphs' state times
zero before the step (tests/_reset_restate.py): state bit exact, beliefs and gradients inside the float64 bound of
tests/_golden.py:fp64_rollout_bounds.  Needs an MI355X."""
import pytest
import torch

from _reset_restate import clear_graphs, fp64_reset_bounds
from oracle import dense as od
from test_dense_gpu import DEV
from test_rows_gpu import _mk

pytestmark = pytest.mark.gpu

TP_SHAPES = [([1, 2, 4], 37, 16, 32, 32, 32, 40),      # partial tile, T > N
             ([0, 1, 3], 5, 64, 64, 64, 16, 70),       # self loop, wide, narrow H2
             ([2, 5], 64, 12, 32, 64, 64, 11)]         # T < N


def _reset_mask(T, B, N, seed):
    """Random entries at p = 0.1 plus forced graphs: 0 never reset (outgrows the graph where T > N), 1 reset at every
    step, 2 reset at t = 0, at two consecutive steps and at T - 1; where T > N, 3 ends on an episode of exactly N steps
    and 4 on one of N + 1."""
    assert B >= 5
    g = torch.Generator().manual_seed(seed)
    reset = torch.rand(T, B, generator=g) < 0.1
    reset[:, 0] = False
    reset[:, 1] = True
    reset[0, 2] = reset[3, 2] = reset[4, 2] = reset[T - 1, 2] = True
    if T > N:
        reset[:, 3] = False
        reset[T - N, 3] = True
        reset[:, 4] = False
        reset[T - N - 1, 4] = True
    return reset


def _check(mem, g, ref, osel_factory, obs, reset, hidden, w, N, out, hid, obs_d=None):
    """state bit exact, beliefs / parameter (/ observation) gradients inside the float64 bound; prints the figures"""
    out32, hid32, bounds, (out64, out_atol) = fp64_reset_bounds(ref, obs, reset, hidden, w, osel_factory, N)
    assert torch.equal(hid[0].cpu(), hid32[0]) and torch.equal(hid[1].cpu(), hid32[1])
    assert torch.equal(hid[3].cpu(), hid32[3])
    err = float((out.detach().cpu().double() - out64).abs().max())
    print("beliefs", err, out_atol)
    assert err <= out_atol
    grads = dict(g.named_parameters())
    for k, (g64, atol) in bounds.items():
        got = obs_d.grad if k == "obs" else grads[k].grad
        err = float((got.cpu().double() - g64).abs().max())
        print(k, err, atol)
        assert err <= atol, k


@pytest.mark.parametrize("hops,B,N,F,H1,H2,T", TP_SHAPES)
def test_rollout_reset_time_parallel_vs_oracle(hops, B, N, F, H1, H2, T):
    torch.manual_seed(N + T)
    ref, g, mem, osel = _mk(B, N, F, H1, H2, ("temporal", hops, "forward"), False)
    obs, w = torch.rand(T, B, F), torch.rand(T, B, H2)
    reset = _reset_mask(T, B, N, 100 + T)
    out, hid = mem.rollout(obs.to(DEV), reset=reset.to(DEV))
    assert out.grad_fn.name() == "GcmRowsRollout"
    (out * w.to(DEV)).sum().backward()
    mem.check_flags()
    _check(mem, g, ref, lambda: osel, obs, reset, None, w, N, out, hid)


@pytest.mark.parametrize("hops,B,N,F,H1,H2,T", TP_SHAPES)
def test_rollout_all_false_reset_equals_no_reset(hops, B, N, F, H1, H2, T):
    torch.manual_seed(N + T + 1)
    ref, g, mem, osel = _mk(B, N, F, H1, H2, ("temporal", hops, "forward"), False)
    obs, w = torch.rand(T, B, F).to(DEV), torch.rand(T, B, H2).to(DEV)
    res = []
    for reset in (None, torch.zeros(T, B, dtype=torch.bool, device=DEV)):
        g.zero_grad(set_to_none=True)
        out, hid = mem.rollout(obs, reset=reset)
        assert out.grad_fn.name() == "GcmRowsRollout"
        (out * w).sum().backward()
        mem.check_flags()
        res.append((out.detach(), hid, [p.grad.clone() for p in g.parameters()]))
    (oa, ha, ga), (ob, hb, gb) = res
    assert torch.equal(oa, ob)
    assert torch.equal(ha[0], hb[0]) and torch.equal(ha[1], hb[1]) and torch.equal(ha[3], hb[3])
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)


def _staggered(B, N, F):
    count0 = torch.randint(0, N + 1, (B,))
    nodes0 = torch.rand(B, N, F) * (torch.arange(N)[None, :, None] < count0[:, None, None])
    adj0 = torch.zeros(B, N, N)
    for b in range(B):
        for i in range(1, int(count0[b])):
            adj0[b, i, i - 1] = 1.0
    return nodes0, adj0, torch.zeros(0), count0


LOOP_CASES = {
    # name: (selector, B, N, F, H1, H2, T, given hidden, obs.requires_grad)
    "no_tp_form": (("temporal", [3, 7], "forward"), 5, 12, 32, 32, 32, 40, False, False),
    "given_hidden": (("temporal", [1, 2, 4], "forward"), 5, 16, 32, 32, 32, 24, True, False),
    "dense_edge": (("dense", None, None), 5, 20, 12, 40, 8, 26, False, False),
    "both_directions": (("temporal", [1, 3], "both"), 5, 12, 8, 8, 24, 30, False, False),
    "obs_grad": (("temporal", [1, 2, 4], "forward"), 5, 16, 32, 32, 32, 24, False, True),
    "obs_grad_given_hidden": (("temporal", [1, 2], "both"), 5, 16, 32, 32, 32, 20, True, True),
}


@pytest.mark.parametrize("name", sorted(LOOP_CASES))
def test_rollout_reset_loop_path_vs_oracle(name):
    sel, B, N, F, H1, H2, T, given, dx = LOOP_CASES[name]
    torch.manual_seed(len(name) + T)
    ref, g, mem, osel = _mk(B, N, F, H1, H2, sel, False)
    obs, w = torch.rand(T, B, F), torch.rand(T, B, H2)
    reset = _reset_mask(T, B, N, 200 + T)
    hidden = _staggered(B, N, F) if given else None
    obs_d = obs.to(DEV).requires_grad_(dx)
    hidden_d = None if hidden is None else tuple(t.to(DEV) for t in hidden)
    out, hid = mem.rollout(obs_d, hidden_d, reset=reset.to(DEV))
    assert out.grad_fn.name() != "GcmRowsRollout"
    (out * w.to(DEV)).sum().backward()
    mem.check_flags()
    if hidden is not None:      # the caller's state is not touched
        assert all(torch.equal(a.cpu(), b) for a, b in zip(hidden_d, hidden))
    _check(mem, g, ref, lambda: osel, obs.requires_grad_(dx), reset, hidden, w, N, out, hid, obs_d)


def test_rollout_reset_euclidean_edge_vs_oracle():
    """EuclideanEdge (cross-batch mean distance): clustered observations keep every decision far from the threshold."""
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.distance import EuclideanEdge
    B, N, F, H, T = 6, 16, 32, 32, 24
    torch.manual_seed(5)
    centres = 3 * torch.randn(6, F)
    obs = centres[torch.arange(T) % 6][:, None, :] + 0.05 * torch.randn(T, B, F)
    w = torch.rand(T, B, H)
    reset = _reset_mask(T, B, N, 300)
    ref = od.canonical_gnn(F, H)
    g = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(F, H), "x, adj -> x"), torch.nn.Tanh(),
                                               (G.DenseGraphConv(H, H), "x, adj -> x"), torch.nn.Tanh()])
    g.load_state_dict(ref.state_dict())
    g = g.to(DEV)
    mem = DenseGCM(g, edge_selectors=EuclideanEdge(3.0), graph_size=N)
    out, hid = mem.rollout(obs.to(DEV), reset=reset.to(DEV))
    (out * w.to(DEV)).sum().backward()
    mem.check_flags()
    assert float(hid[1].sum()) > 0
    _check(mem, g, ref, lambda: od.EuclideanEdge(3.0), obs, reset, None, w, N, out, hid)


@pytest.mark.parametrize("sel", [("temporal", [1, 2, 4], "forward"), ("dense", None, None)])
def test_rollout_reset_batch_first_and_cpu_mask(sel):
    """batch_first=True takes reset [B, T]; a CPU `reset` and a device `reset` give equal results (time-parallel path
    and loop path)."""
    B, N, F, H, T = 6, 16, 32, 32, 20
    torch.manual_seed(11)
    ref, g, mem, osel = _mk(B, N, F, H, H, sel, False)
    obs, w = torch.rand(T, B, F).to(DEV), torch.rand(T, B, H).to(DEV)
    reset = _reset_mask(T, B, N, 400)
    res = []
    for kind in ("device", "cpu", "batch_first"):
        g.zero_grad(set_to_none=True)
        if kind == "batch_first":
            out, hid = mem.rollout(obs.transpose(0, 1).contiguous(), batch_first=True, reset=reset.t().to(DEV))
            assert out.shape == (B, T, H)
            out = out.transpose(0, 1)
        else:
            out, hid = mem.rollout(obs, reset=reset.to(DEV) if kind == "device" else reset)
            assert (out.grad_fn.name() == "GcmRowsRollout") == (sel[0] == "temporal")
        (out * w).sum().backward()
        mem.check_flags()
        res.append((out.detach().clone(), hid, [p.grad.clone() for p in g.parameters()]))
    for o, h, gr in res[1:]:
        assert torch.equal(o, res[0][0])
        assert all(torch.equal(x, y) for x, y in zip(h, res[0][1]))
        assert all(torch.equal(x, y) for x, y in zip(gr, res[0][2]))      # (ordered sums on both paths)


def test_reset_hidden_in_place_mid_chain_ends_the_cached_steps():
    """donate_state=True, forward hops: a per-step loop that calls reset_hidden at t = 9 of 30.  The cached steps read
    per-chain caches and the host's step count, not the state: the clear must end them (version counters / dropped
    entries) exactly as the caller's own in-place edit does (test_rows_gpu.py) - against the oracle."""
    B, N, F, H, T, t_reset, done = 6, 16, 32, 32, 30, 9, [1, 4]
    torch.manual_seed(77)
    ref, g, mem, osel = _mk(B, N, F, H, H, ("temporal", [1, 2, 4], "forward"), True)
    obs, w = torch.rand(T, B, F), torch.rand(T, B, H)
    reset = torch.zeros(T, B, dtype=torch.bool)
    reset[t_reset, done] = True
    hid, outs = None, []
    for t in range(T):
        if t == t_reset:
            before = hid
            hid = mem.reset_hidden(hid, reset[t].to(DEV))
            assert all(a is b for a, b in zip(hid, before))          # in place: the caller's own tensors
            assert float(hid[0][done].abs().sum()) == 0 and hid[3][done].tolist() == [0, 0]
        mx, hid = mem(obs[t].to(DEV), hid)
        outs.append(mx)
    assert mem.rows_steps() == T
    assert mem.rows_cached_steps_taken() == t_reset      # cached steps up to the clear, the state-reading kernel behind it
    out = torch.stack(outs)
    (out * w.to(DEV)).sum().backward()
    mem.check_flags()
    _check(mem, g, ref, lambda: osel, obs, reset, None, w, N, out, hid)


@pytest.mark.parametrize("weights", [False, True])
def test_reset_hidden_functional_form(weights):
    """Functional by default: new tensors, the inputs untouched; the gradient w.r.t. the cleared graphs' incoming state
    is zero, the others' the identity - directly and through a step behind it.  Odd sizes: the 4-byte kernel."""
    for (B, N, F) in ((5, 16, 32), (3, 7, 5)):
        torch.manual_seed(B)
        ref, g, mem, osel = _mk(B, N, F, 32, 32, ("temporal", [1, 2], "forward"), False)
        nodes0, adj0, _, count0 = _staggered(B, N, F)
        w0 = torch.rand(B, N, N) if weights else torch.zeros(0)
        mask = torch.zeros(B, dtype=torch.bool)
        mask[[0, B - 1]] = True
        hidden = (nodes0.to(DEV).requires_grad_(True), adj0.to(DEV).requires_grad_(True),
                  w0.to(DEV).requires_grad_(weights), count0.to(DEV))
        h2 = mem.reset_hidden(hidden, mask)              # (a CPU mask)
        want = clear_graphs((nodes0, adj0, w0, count0), mask)
        for got, exp, src in zip(h2, want, (nodes0, adj0, w0, count0)):
            assert torch.equal(got.detach().cpu(), exp)
        for t, src in zip(hidden, (nodes0, adj0, w0, count0)):
            assert torch.equal(t.detach().cpu(), src) and t._version == 0
        assert all(a is not b for a, b in zip((h2[0], h2[1], h2[3]), (hidden[0], hidden[1], hidden[3])))
        gn, ga = torch.rand(B, N, F, device=DEV), torch.rand(B, N, N, device=DEV)
        loss = (h2[0] * gn).sum() + (h2[1] * ga).sum()
        if weights:
            gw = torch.rand(B, N, N, device=DEV)
            loss = loss + (h2[2] * gw).sum()
        loss.backward()
        keep = (~mask).float().to(DEV)[:, None, None]
        assert torch.equal(hidden[0].grad, gn * keep) and torch.equal(hidden[1].grad, ga * keep)
        if weights:
            assert torch.equal(hidden[2].grad, gw * keep)
    # ... and through a step behind it (layered path: the node matrix carries a gradient)
    B, N, F = 5, 16, 32
    ref, g, mem, osel = _mk(B, N, F, 32, 32, ("temporal", [1, 2], "forward"), False)
    nodes0, adj0, w0, count0 = _staggered(B, N, F)
    count0 = count0.clamp(min=3, max=N - 1)
    mask = torch.tensor([True, False, False, True, False])
    nd = nodes0.to(DEV).requires_grad_(True)
    h2 = mem.reset_hidden((nd, adj0.to(DEV), w0.to(DEV), count0.to(DEV)), mask.to(DEV))
    mx, h3 = mem(torch.rand(B, F, device=DEV), h2)
    (mx.sum() + h3[0].sum()).backward()
    mem.check_flags()
    assert float(nd.grad[mask].abs().sum()) == 0 and float(nd.grad[~mask].abs().sum()) > 0
    assert h3[3].cpu().tolist() == [1 if m else int(c) + 1 for m, c in zip(mask.tolist(), count0.tolist())]
