"""The rollout's head launch absorbed into the merged step node (csrc/rows_cached_run.hip: the FRESH form of
k_step_rows_cached_img4_lean_run, gcm_dense_rows_head_fused_run; DenseGCM.rows_absorb_head, env GCM_ABSORB_HEAD; DESIGN
3.2.1 "the head absorbed").  Every comparison is torch.equal (or equality of the raw words) against the same loop
captured with rows_absorb_head = False: the same operations, so no tolerance.

Shapes: the smallest at which the lean kernel runs and its cases differ - F = H1 = 32, B = 3, N = 16, hops [1, 2, 4],
H2 = 32 and 8; N = T = 128 for the self entries and the adjacency rows past 64; B = 3 < 32 also takes the further rounds
of the packed vector and the image inside one workgroup."""
import ctypes

import pytest
import torch

from test_dense_gpu import DEV
from test_cached_lean_gpu import _kernels_run
from test_step_run_gpu import _capture, _data, _loop, _module, _replay, _same, _snapshot, F, H1, RUN

pytestmark = pytest.mark.gpu

B, N, T = 3, 16, 16


def _captured(H2, absorb, obs, w, between=None, grad=True, cap=None, hidden0=False, **shape):
    """the loop captured (merging on) and replayed once -> dict(snap, stats, nodes, graph, g, mem, res)"""
    from gcm import _hip
    lib = _hip.lib()
    g, mem = _module(H2, True, cap, **shape)
    mem.rows_absorb_head = absorb
    box = {}

    def body():
        if hidden0:
            h0 = mem.get_initial_hidden_state(obs[0])
            mx, h = mem(obs[0], h0)
            outs = [mx]
            for t in range(1, obs.shape[0]):
                mx, h = mem(obs[t], h)
                outs.append(mx)
            out = torch.stack(outs)
            if grad:
                (out * w).sum().backward()
            res = (out, h, None)
        elif grad:
            res = _loop(mem, obs, w, between, True)
        else:
            with torch.no_grad():
                res = _loop(mem, obs, w, between, False)
        box["nodes"] = lib.gcm_rows_capture_node_count(_hip.stream())
        return res
    graph, res = _capture(mem, g, body)
    stats = mem.merge_stats(head=True)
    _replay(graph, g)
    return dict(snap=_snapshot(mem, g, *res), stats=stats, nodes=box["nodes"], graph=graph, g=g, mem=mem, res=res)


def _on_off(H2, obs, w, **kw):
    on, off = _captured(H2, True, obs, w, **kw), _captured(H2, False, obs, w, **kw)
    assert off["stats"]["head_absorbed"] == 0
    _same(on["snap"], off["snap"])
    on["mem"].check_flags()
    return on, off


@pytest.mark.parametrize("H2", [32, 8])
def test_full_merge_absorbs_the_head(H2):
    """T = N = 16: one node for head and steps, one kernel node fewer in the graph; beliefs, final state and parameter
    gradients over three replays on a rewritten observation buffer"""
    obs, w = _data(H2)
    on, off = _on_off(H2, obs, w)
    assert on["stats"] == {"nodes": 1, "merged_steps": T - 1, "head_absorbed": 1}
    assert off["stats"] == {"nodes": 1, "merged_steps": T - 1, "head_absorbed": 0}
    assert on["nodes"] > 0 and on["nodes"] == off["nodes"] - 1
    seen = [on["snap"][0][0]]
    for k in range(3):
        obs.copy_(torch.rand(T, B, F, generator=torch.Generator().manual_seed(60 + k)).to(DEV))
        snaps = []
        for c in (on, off):
            _replay(c["graph"], c["g"])
            snaps.append(_snapshot(c["mem"], c["g"], *c["res"]))
        _same(*snaps)
        assert not any(torch.equal(snaps[0][0][0], s) for s in seen)
        seen.append(snaps[0][0][0])


@pytest.mark.parametrize("H2", [32, 8])
def test_short_rollout_leaves_the_rest_zero(H2):
    """T = 5 < N: rows 5 .. 15 of nodes and adj are zero, the count is 5"""
    obs, w = _data(H2, steps=5)
    on, off = _on_off(H2, obs, w)
    assert on["stats"] == {"nodes": 1, "merged_steps": 4, "head_absorbed": 1}
    out, nodes, adj, count = on["snap"][0][:4]
    assert not bool(nodes[:, 5:].any()) and not bool(adj[:, 5:].any()) and bool((count == 5).all())
    assert bool(nodes[:, :5].any()) and bool(adj[:, :5].any())


def test_cap_split_first_node_fresh():
    """rows_merge_cap = 5 at T = 16: the first node is fresh with n = 5, the later nodes are the ordinary instantiation
    and start from rows the fresh node wrote"""
    obs, w = _data(32)
    on, off = _on_off(32, obs, w, cap=5)
    assert on["stats"] == {"nodes": 4, "merged_steps": 12, "head_absorbed": 1}
    assert on["nodes"] == off["nodes"] - 1


def test_self_entries_and_rows_past_64():
    """hops [0, 1, 2, 4] at N = T = 128: the self entries of the closed-form adjacency rows, both halves of a row"""
    obs, w = _data(32, steps=128)
    on, _ = _on_off(32, obs, w, N=128, hops=[0, 1, 2, 4])
    assert on["stats"] == {"nodes": 1, "merged_steps": 127, "head_absorbed": 1}


def test_largest_hop_past_graph_size():
    """hops [1, 2, 4, 20] at N = 16: the general source path throughout"""
    obs, w = _data(8)
    on, _ = _on_off(8, obs, w, hops=[1, 2, 4, 20])
    assert on["stats"] == {"nodes": 1, "merged_steps": T - 1, "head_absorbed": 1}


def test_parameters_changed_between_replays():
    """p.add_() under no_grad between two replays: the replay reads the live parameters - beliefs, the packed vector and
    the weight image equal the switch-off graph's after the same edit"""
    obs, w = _data(32)
    on, off = _on_off(32, obs, w)
    first = on["snap"][0][0]
    snaps, held = [], []
    for c in (on, off):
        with torch.no_grad():
            for i, p in enumerate(c["g"].parameters()):
                p.add_(0.03 * (i + 1))
        _replay(c["graph"], c["g"])
        snaps.append(_snapshot(c["mem"], c["g"], *c["res"]))
        pc = c["mem"]._packed_cache
        assert pc[5] is not None
        held.append((pc[1].detach().clone(), pc[5].clone()))
    _same(*snaps)
    assert not torch.equal(snaps[0][0][0], first)
    assert torch.equal(held[0][0].view(torch.int32), held[1][0].view(torch.int32))
    assert torch.equal(held[0][1].view(torch.int32), held[1][1].view(torch.int32))
    for p in on["g"].parameters():   # the vector holds the edited values
        assert bool(torch.isin(p.detach().reshape(-1), held[0][0]).all())


def test_single_step_not_absorbed():
    """T = 1: nothing is appended, the head stays"""
    obs, w = _data(32, steps=1)
    on, off = _on_off(32, obs, w)
    assert on["stats"] == {"nodes": 1, "merged_steps": 0, "head_absorbed": 0} and on["nodes"] == off["nodes"]


def test_node_in_front_of_the_head_is_kept_as_dependency():
    """the first observation computed inside the capture ahead of the call: the head has a dependency, and the merged
    node is added on it"""
    between = lambda t, x, h, outs, box: x * 2 if t == 0 else x   # noqa: E731
    obs, w = _data(32)
    on, off = _on_off(32, obs, w, between=between)
    assert on["stats"] == {"nodes": 1, "merged_steps": T - 1, "head_absorbed": 1} and on["nodes"] == off["nodes"] - 1


def test_foreign_node_behind_the_head_not_absorbed():
    """a strided first observation: forward() makes it contiguous behind the head launch - a copy node between the head
    and step 0, so the head stays"""
    def between(t, x, h, outs, box):
        return torch.stack([x, x], 2)[:, :, 0] if t == 0 else x
    obs, w = _data(32)
    on, off = _on_off(32, obs, w, between=between)
    assert on["stats"] == {"nodes": 1, "merged_steps": T - 1, "head_absorbed": 0} and on["nodes"] == off["nodes"]


def test_callers_state_not_absorbed():
    """hidden is the caller's zero state, not None: no head launch carved it"""
    obs, w = _data(32)
    on, off = _on_off(32, obs, w, hidden0=True)
    assert on["stats"]["head_absorbed"] == 0 and on["nodes"] == off["nodes"]


def test_eager_loop_runs_neither_the_fresh_form_nor_a_graph_edit():
    obs, w = _data(32)
    g, mem = _module(32, True)
    assert mem.rows_absorb_head
    box = {}
    names = _kernels_run(lambda: box.update(r=_loop(mem, obs, w)))
    assert not any(RUN in k for k in names) and any("k_head_fused" in k for k in names)
    assert mem.merge_stats(head=True) == {"nodes": 0, "merged_steps": 0, "head_absorbed": 0}
    g2, mem2 = _module(32, True)
    mem2.rows_absorb_head = False
    out2, hid2, _ = _loop(mem2, obs, w)
    _same(_snapshot(mem, g, *box["r"][:2]), _snapshot(mem2, g2, out2, hid2))


# ---- every word, through the C ABI (the test owns every buffer) ------------------------------------------------------
SENTINEL = 0x7FC0BEEF   # a NaN payload no kernel produces
IMG_V4 = 64


def _pad(n):
    return (n + 63) & ~63


def _abi_rollout(lib, _hip, hops, N, H2, n, record, absorbed):
    """head + n cached steps from row 0 on sentinel-filled buffers: launch by launch (gcm_dense_rows_head_fused,
    gcm_dense_rows_step_cached_ws), or captured through the run entries (one node) and replayed -> the buffers"""
    g = torch.Generator().manual_seed(11 * N + H2 + n)
    shapes = [(H1, F), (H1, F), (H1,), (H2, H1), (H2, H1), (H2,)]
    srcs = [(torch.randn(s, generator=g) * 0.2).to(DEV) for s in shapes]
    obs = torch.rand(n, B, F, generator=g).to(DEV)
    lay = (ctypes.c_size_t * 5)()
    assert lib.gcm_dense_rows_cached_layout(B, N, F, H1, H2, ctypes.addressof(lay)) == 0
    words = int(lay[0]) if record else B * H2

    def fill(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    n_nodes, n_adj = _pad(B * N * F), _pad(B * N * N)
    buf = dict(state=fill(n_nodes + n_adj + 2 * B), packed=fill(sum(t.numel() for t in srcs)),
               image=fill(lib.gcm_dense_rows_cached_weight_image_floats()), cH=fill(B, N, H1), cA=fill(B, N, F),
               cX=fill(B, N, F), saved=fill(n, int(lay[0])), flags=torch.zeros(1, dtype=torch.int32, device=DEV),
               words=words)
    st = buf["state"]
    nodes, adj, count = st[:n_nodes], st[n_nodes:n_nodes + n_adj], st[n_nodes + n_adj:]
    p = _hip.ptr
    d = _hip.SelectorDesc(kind=_hip.SEL_TEMPORAL, n_hops=len(hops), direction=_hip.DIR["forward"])
    for i, h in enumerate(hops):
        d.hops[i] = h
    arr = (_hip.SelectorDesc * 1)(d)
    ptrs = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in srcs])
    lens = (ctypes.c_size_t * 6)(*[t.numel() for t in srcs])
    head = (ptrs, lens, 6, p(buf["packed"]), p(buf["image"]), F, H1, H2, p(st), 4 * st.numel())
    common = lambda t: (p(obs[t]), p(nodes), p(adj), p(count), ctypes.addressof(arr), 1, p(buf["packed"]),  # noqa: E731
                        p(buf["image"]), 3 | IMG_V4, 1, 1, p(buf["cH"]), p(buf["cA"]), p(buf["cX"]), p(buf["saved"][t]),
                        1 if record else 0, t, p(buf["flags"]), None, 0, B, N, F, H1, H2)
    torch.cuda.synchronize()
    if not absorbed:
        assert lib.gcm_dense_rows_head_fused(*head, _hip.stream()) == 0
        for t in range(n):
            assert lib.gcm_dense_rows_step_cached_ws(*common(t), _hip.stream()) == 0, t
    else:
        run = lib.gcm_rows_run_create()
        assert run
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                assert lib.gcm_dense_rows_head_fused_run(run, *head, _hip.stream()) == 0
                for t in range(n):
                    assert lib.gcm_dense_rows_step_cached_run(run, *common(t), _hip.stream()) == 0, t
                assert lib.gcm_rows_capture_node_count(_hip.stream()) == 1
            stats = (ctypes.c_int * 2)()
            assert lib.gcm_rows_run_stats(run, stats) == 0
            assert (stats[0], stats[1]) == (1, n - 1) and lib.gcm_rows_run_absorbed(run) == 1
            # (nothing has run yet: the capture launched nothing)
            assert bool((buf["state"].view(torch.int32) == SENTINEL).all())
            graph.replay()
        finally:
            torch.cuda.synchronize()
            lib.gcm_rows_run_destroy(run)
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("N,short", [(16, 0), (16, 5), (128, 0), (128, 3)])
@pytest.mark.parametrize("record", [True, False])
@pytest.mark.parametrize("self_loop", [True, False])
def test_every_word(self_loop, record, N, short):
    """every word of the state allocation with its paddings, of the packed vector, the image, the caches and the records
    equals what head + per-step launches leave; n = N and n < N"""
    from gcm import _hip
    lib = _hip.lib()
    hops = ([0] if self_loop else []) + [1, 2, 4]
    n = N - short
    want = _abi_rollout(lib, _hip, hops, N, 32, n, record, absorbed=False)
    got = _abi_rollout(lib, _hip, hops, N, 32, n, record, absorbed=True)
    assert int(want["flags"].item()) == 0 and int(got["flags"].item()) == 0
    for k in ("state", "packed", "image", "cH", "cA", "cX", "saved"):
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    assert not bool((got["state"].view(torch.int32) == SENTINEL).any())
    assert not bool((got["image"].view(torch.int32) == SENTINEL).any())
    count = got["state"][_pad(B * N * F) + _pad(B * N * N):].view(torch.int64)
    assert bool((count == n).all())
