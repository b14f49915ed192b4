"""Lean cached steps captured back to back as ONE graph node (csrc/rows_cached_run.hip: k_step_rows_cached_img4_lean_run,
gcm_dense_rows_step_cached_run; DenseGCM.rows_merge_captured, env GCM_MERGE_CAPTURED): every case captures the same
per-step loop with the switch on and off and compares beliefs, final hidden state, flag word and parameter gradients
bit for bit; merge_stats() tells what was merged.

Shapes: the smallest at which the lean kernel runs and its cases differ - F = H1 = 32, B = 3, N = 16, hops [1, 2, 4]
(rows 0 - 3 have empty source slots, later rows none), H2 = 32 and 8.  Beside them: hops [0, 1, 2, 4] at N = T = 128
(the self flag, four slots, rows past 64), hops [1, 2, 4, 20] (one past N), and B = 8200 for records large enough to be
allocations of their own, whose addresses the allocator reuses inside one capture."""
import pytest
import torch

from test_dense_gpu import DEV
from test_rows_gpu import _mk
from test_cached_lean_gpu import _kernels_run

pytestmark = pytest.mark.gpu

B, N, F, H1, T = 3, 16, 32, 32, 16
HOPS = [1, 2, 4]
RUN, LEAN = "k_step_rows_cached_img4_lean_run", "k_step_rows_cached_img4_lean"


def _module(H2, on, cap=None, seed=21, B=B, N=N, hops=HOPS):
    torch.manual_seed(seed)
    ref, g, mem, osel = _mk(B, N, F, H1, H2, ("temporal", hops, "forward"), True)
    mem.rows_merge_captured = on
    mem.rows_merge_cap = cap
    return g, mem


def _data(H2, steps=T, seed=22, B=B):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(steps, B, F, generator=gen).to(DEV), torch.rand(steps, B, H2, generator=gen).to(DEV)


def _loop(mem, obs, w, between=None, grad=True):
    """`for t: mx, m = mem(obs[t], m)` (+ backward); between(t, obs_t, m, mx) -> obs_t runs inside the loop"""
    h, outs, box = None, [], {}
    for t in range(obs.shape[0]):
        x = obs[t]
        if between is not None:
            x = between(t, x, h, outs, box)
        mx, h = mem(x, h)
        outs.append(mx)
    out = torch.stack(outs)
    if grad:
        (out * w).sum().backward()
    return out, h, box.get("extra")


def _snapshot(mem, g, out, hid, extra=None):
    torch.cuda.synchronize()
    flags = [int(f.item()) for f in mem._flags.values()]
    grads = [p.grad.clone() for p in g.parameters() if p.grad is not None]
    return ([out.clone(), hid[0].clone(), hid[1].clone(), hid[3].clone()] + ([extra.clone()] if extra is not None else []),
            flags, grads)


def _same(a, b):
    assert len(a[0]) == len(b[0]) and len(a[2]) == len(b[2])
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert a[1] == b[1]
    for x, y in zip(a[2], b[2]):
        assert torch.equal(x, y)


def _capture(mem, g, body):
    """warm-up on a side stream (no eager autograd graph left alive), then the capture -> (graph, what body returned)"""
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g.zero_grad(set_to_none=True)
            body()
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = body()
    return graph, res


def _replay(graph, g):
    with torch.no_grad():
        for p in g.parameters():
            if p.grad is not None:
                p.grad.zero_()
    graph.replay()


def _captured(H2, on, obs, w, between=None, grad=True, cap=None, **shape):
    """the loop captured and replayed once -> (snapshot, merge_stats, graph, module, mem, captured results)"""
    g, mem = _module(H2, on, cap, **shape)
    if grad:
        graph, res = _capture(mem, g, lambda: _loop(mem, obs, w, between, True))
    else:
        def body():
            with torch.no_grad():
                return _loop(mem, obs, w, between, False)
        graph, res = _capture(mem, g, body)
    stats = mem.merge_stats()
    _replay(graph, g)
    return _snapshot(mem, g, *res), stats, graph, g, mem, res


@pytest.mark.parametrize("H2", [32, 8])
def test_full_merge_replays_and_eager(H2):
    """fwd + bwd in the graph: the T step nodes are ceil(T / cap) = 1; three replays with the static observation buffer
    rewritten in between track its contents; the last one also equals the eager loop."""
    from gcm import _hip
    obs, w = _data(H2)
    cap = _hip.lib().gcm_rows_run_steps_cap()
    on, st_on, graph_on, g_on, mem_on, res_on = _captured(H2, True, obs, w)
    off, st_off, graph_off, g_off, mem_off, res_off = _captured(H2, False, obs, w)
    assert st_on == {"nodes": -(-T // cap), "merged_steps": T - -(-T // cap)}
    assert st_off == {"nodes": 0, "merged_steps": 0}
    _same(on, off)
    seen = [on[0][0]]
    for k in range(3):
        new = torch.rand(T, B, F, generator=torch.Generator().manual_seed(30 + k)).to(DEV)
        obs.copy_(new)
        _replay(graph_on, g_on)
        _replay(graph_off, g_off)
        a, b = _snapshot(mem_on, g_on, *res_on), _snapshot(mem_off, g_off, *res_off)
        _same(a, b)
        assert not any(torch.equal(a[0][0], s) for s in seen)
        seen.append(a[0][0])
    g_e, mem_e = _module(H2, True)
    out_e, hid_e, _ = _loop(mem_e, obs, w)
    _same(a, _snapshot(mem_e, g_e, out_e, hid_e))
    assert mem_e.merge_stats() == {"nodes": 0, "merged_steps": 0}
    for m in (mem_on, mem_off, mem_e):
        m.check_flags()


def test_cap_split():
    """a cap of 5 steps per node: 5 + 5 + 5 + 1, the second to fourth node starting from rows of earlier nodes"""
    obs, w = _data(32)
    on, st_on, *_ = _captured(32, True, obs, w, cap=5)
    off, st_off, *_ = _captured(32, False, obs, w)
    assert st_on == {"nodes": 4, "merged_steps": 12}
    _same(on, off)


def _expect_unmerged(between, H2=32, nodes=T):
    obs, w = _data(H2)
    on, st_on, *_ = _captured(H2, True, obs, w, between)
    off, st_off, *_ = _captured(H2, False, obs, w, between)
    assert st_on == {"nodes": nodes, "merged_steps": T - nodes}
    _same(on, off)


def test_foreign_node_between_steps():
    """obs_t = raw[t] * 2 computed inside the loop: a node between every two steps, nothing merges"""
    _expect_unmerged(lambda t, x, h, outs, box: x * 2)


def test_belief_consumed_between_steps():
    """acc = acc + mx.sum() inside the loop: the previous belief is read before the next step, nothing merges"""
    def between(t, x, h, outs, box):
        if outs:
            box["extra"] = box.get("extra", 0) + outs[-1].detach().sum()
        return x
    _expect_unmerged(between)


def test_state_edited_in_place():
    """one graph's node rows zeroed at t = 7 on the donated state: steps 0 - 6 are one node, from step 7 on the checked
    path runs the general kernel; results as with the switch off"""
    def between(t, x, h, outs, box):
        if t == 7:
            h[0][1].zero_()
        return x
    obs, w = _data(32)
    on, st_on, *_ = _captured(32, True, obs, w, between)
    off, st_off, *_ = _captured(32, False, obs, w, between)
    assert st_on == {"nodes": 1, "merged_steps": 6}
    _same(on, off)


def test_no_grad():
    """torch.no_grad(): the record is the belief alone (rec = 0); merged and identical"""
    obs, w = _data(8)
    on, st_on, *_ = _captured(8, True, obs, w, grad=False)
    off, st_off, *_ = _captured(8, False, obs, w, grad=False)
    assert st_on == {"nodes": 1, "merged_steps": T - 1}
    _same(on, off)


def test_longer_than_graph_size():
    """T = 20 > N: the first 16 steps are one node, the steady-state steps stay launches of their own"""
    obs, w = _data(32, steps=20)
    on, st_on, *_ = _captured(32, True, obs, w)
    off, st_off, *_ = _captured(32, False, obs, w)
    assert st_on == {"nodes": 1, "merged_steps": N - 1}
    _same(on, off)


def _two_captures(on):
    g, mem = _module(32, on)
    (obs_a, w_a), (obs_b, w_b) = _data(32, seed=40), _data(32, seed=41)
    graph_a, res_a = _capture(mem, g, lambda: _loop(mem, obs_a, w_a))
    stats_a = mem.merge_stats()
    graph_b, res_b = _capture(mem, g, lambda: _loop(mem, obs_b, w_b))
    stats_b = mem.merge_stats()
    snaps = []
    for graph, res in ((graph_a, res_a), (graph_b, res_b), (graph_a, res_a), (graph_b, res_b)):
        _replay(graph, g)
        snaps.append(_snapshot(mem, g, *res))
    mem.check_flags()
    return snaps, stats_a, stats_b


def test_two_captures_alternating_replays():
    """two captures of one module, one after the other (the second meets the first one's remembered node, of a capture
    that is over), replayed in turns: each as with the switch off, counters per capture"""
    on, st_a, st_b = _two_captures(True)
    off, _, _ = _two_captures(False)
    assert st_a == st_b == {"nodes": 1, "merged_steps": T - 1}
    for a, b in zip(on, off):
        _same(a, b)
    _same(on[0], on[2])
    _same(on[1], on[3])
    assert not torch.equal(on[0][0][0], on[1][0][0])


def test_second_stream_joined_between_steps():
    """work on a second stream joined into the capture between two steps: the stream then waits for more than the step's
    node, nothing merges"""
    side = torch.cuda.Stream()
    raw = torch.ones(4, device=DEV)

    def between(t, x, h, outs, box):
        if t > 0:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                box["extra"] = raw * float(t)
            torch.cuda.current_stream().wait_stream(side)
        return x
    _expect_unmerged(between)


def test_eager_loop_unchanged():
    """not capturing: the per-step launches of the lean kernel, nothing merged, the multi-step kernel never runs"""
    obs, w = _data(32)
    res = []
    for on in (True, False):
        g, mem = _module(32, on)
        box = {}
        names = _kernels_run(lambda: box.update(r=_loop(mem, obs, w)))
        assert any(LEAN in k and RUN not in k for k in names) and not any(RUN in k for k in names)
        assert mem.merge_stats() == {"nodes": 0, "merged_steps": 0}
        res.append(_snapshot(mem, g, *box["r"][:2]))
        mem.check_flags()
    _same(res[0], res[1])


def test_self_loop_and_rows_past_64():
    """hops [0, 1, 2, 4] at N = T = 128: the self flag, four source slots, and the rows >= 64 of the adjacency entries,
    live list and header (the second mask word), fwd + bwd, one node"""
    n = 128
    obs, w = _data(32, steps=n)
    on, st_on, *_ = _captured(32, True, obs, w, N=n, hops=[0, 1, 2, 4])
    off, st_off, *_ = _captured(32, False, obs, w, N=n, hops=[0, 1, 2, 4])
    assert st_on == {"nodes": 1, "merged_steps": n - 1}
    _same(on, off)


def test_four_hops_one_past_graph_size():
    """hops [1, 2, 4, 20] at N = 16: four distinct hops, the largest never reaches a stored row"""
    obs, w = _data(8)
    on, st_on, *_ = _captured(8, True, obs, w, hops=[1, 2, 4, 20])
    off, st_off, *_ = _captured(8, False, obs, w, hops=[1, 2, 4, 20])
    assert st_on == {"nodes": 1, "merged_steps": T - 1}
    _same(on, off)


def test_belief_fed_back_as_observation():
    """no_grad, obs_t = the belief of step t - 1 (H2 = F): the step reads what the step before it wrote, with no node in
    between - its observation lies on an earlier record, so it starts a new run; results as with the switch off"""
    def between(t, x, h, outs, box):
        return outs[-1] if outs else x
    obs, w = _data(32)
    on, st_on, *_ = _captured(32, True, obs, w, between, grad=False)
    off, st_off, *_ = _captured(32, False, obs, w, between, grad=False)
    assert st_on == {"nodes": T, "merged_steps": 0}
    _same(on, off)
    assert not torch.equal(on[0][0][1], on[0][0][2])


def _last_belief_only(on, big):
    """no_grad, only the last belief kept: every record is freed when the next one exists.  B * H2 * 4 > 1 MB: each record
    is an allocation of its own, and the allocator hands a block freed during the capture out again - records then
    alternate between two addresses, and the later write to an address must win."""
    g, mem = _module(32, on, B=big)
    gen = torch.Generator().manual_seed(50)
    obs = torch.rand(T, big, F, generator=gen).to(DEV)

    def body():
        with torch.no_grad():
            h = mx = None
            for t in range(T):
                mx, h = mem(obs[t], h)
            return mx, h
    graph, (mx, h) = _capture(mem, g, body)
    stats = mem.merge_stats()
    graph.replay()
    torch.cuda.synchronize()
    mem.check_flags()
    return [mx.clone(), h[0].clone(), h[1].clone(), h[3].clone()], stats


def test_recycled_record_addresses():
    """records that reuse an address inside one captured loop: never two of them in one node; the last belief is the last
    step's, as with the switch off and as the eager loop gives it"""
    big = 8200
    on, st_on = _last_belief_only(True, big)
    off, _ = _last_belief_only(False, big)
    assert st_on["nodes"] + st_on["merged_steps"] == T
    for a, b in zip(on, off):
        assert torch.equal(a, b)
    g, mem = _module(32, True, B=big)
    obs = torch.rand(T, big, F, generator=torch.Generator().manual_seed(50)).to(DEV)
    with torch.no_grad():
        h = mx = None
        for t in range(T):
            mx, h = mem(obs[t], h)
    assert torch.equal(mx, on[0])
