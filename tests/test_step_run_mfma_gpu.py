"""The merged step node's layers on the fp32 matrix cores (csrc/rows_cached_run.hip, the MFMA form of
k_step_rows_cached_img4_lean_run; include/gcm_hip_run_mfma.h; DenseGCM.rows_run_mfma, env GCM_RUN_MFMA).

A wave of that form owns the sixteen steps 16 w ... 16 w + 15 of a run as one 16-row tile, so what it can newly get
wrong is a matter of where a run starts and ends against those tiles, which rows feed a row, and which columns are
stored.  Every case runs the same chain of cached steps three ways through the C ABI, on buffers the test owns and has
filled with a sentinel: the per-step launches (uncaptured), and the captured run node replayed once with the switch on
and off.  All three must leave the same words everywhere: beliefs and every other record word, cH / cA / cX, nodes,
adjacency, count, flag word.  F = H1 = 32; the shapes are the smallest that put the boundaries in question inside or
at the edge of a tile."""
import ctypes
import functools

import pytest
import torch

from test_dense_gpu import DEV

pytestmark = pytest.mark.gpu

F = H1 = 32
IMG_V4 = 64
NAN_SENTINEL = 0x7FC0BEEF   # a NaN payload no kernel produces
FINITE_SENTINEL = 0x12345678   # (the NaN case compares isnan masks: its sentinel must not be one)
KEYS = ("nodes", "adj", "cH", "cA", "cX", "saved")


def _chain(form, hops, N, H2, B, T, first=0, record=True, split=None, nan_at=None):
    """Steps 0 ... T - 1 of a chain from empty graphs.  form "steps": one launch each.  "mfma" / "valu": steps
    [0, first) as launches, steps [first, T) captured through the run entry (an unrelated kernel in front of step
    `split`, which no run can extend across) and replayed once.  -> (buffers as int32 words, run stats or None)"""
    from gcm import _hip
    lib = _hip.lib()
    p = _hip.ptr
    g = torch.Generator().manual_seed(1000 * N + 10 * H2 + B)
    P = lib.gcm_dense_gnn2_param_count(F, H1, H2)
    params = (torch.randn(P, generator=g) * 0.2).to(DEV)
    obs = torch.rand(T, B, F, generator=g)
    if nan_at is not None:
        obs[nan_at] = float("nan")
    obs = obs.to(DEV)
    img = torch.empty(lib.gcm_dense_rows_cached_weight_image_floats(), device=DEV)
    assert lib.gcm_dense_rows_cached_weight_image(p(params), p(img), F, H1, H2, _hip.stream()) == 0
    d = _hip.SelectorDesc(kind=_hip.SEL_TEMPORAL, n_hops=len(hops), direction=_hip.DIR["forward"])
    for i, h in enumerate(hops):
        d.hops[i] = h
    arr = (_hip.SelectorDesc * 1)(d)
    lay = (ctypes.c_size_t * 5)()
    assert lib.gcm_dense_rows_cached_layout(B, N, F, H1, H2, ctypes.addressof(lay)) == 0
    sentinel = NAN_SENTINEL if nan_at is None else FINITE_SENTINEL

    def fill(*shape):
        return torch.full(shape, sentinel, dtype=torch.int32, device=DEV).view(torch.float32)

    buf = dict(nodes=fill(B, N, F), adj=fill(B, N, N), cH=fill(B, N, H1), cA=fill(B, N, F), cX=fill(B, N, F),
               saved=fill(T, int(lay[0])), count=torch.zeros(B, dtype=torch.int64, device=DEV),
               flags=torch.zeros(1, dtype=torch.int32, device=DEV))
    other = torch.zeros(64, device=DEV)
    common = lambda t: (p(obs[t]), p(buf["nodes"]), p(buf["adj"]), p(buf["count"]), ctypes.addressof(arr), 1, p(params),  # noqa: E731
                        p(img), 3 | IMG_V4, 1, 1, p(buf["cH"]), p(buf["cA"]), p(buf["cX"]), p(buf["saved"][t]),
                        1 if record else 0, t, p(buf["flags"]), None, 0, B, N, F, H1, H2)
    torch.cuda.synchronize()
    stats = None
    for t in range(T if form == "steps" else first):
        assert lib.gcm_dense_rows_step_cached_ws(*common(t), _hip.stream()) == 0, t
    if form != "steps":
        run = lib.gcm_rows_run_create()
        assert run
        try:
            assert lib.gcm_rows_run_set_mfma(run, 1 if form == "mfma" else 0) == 0
            assert lib.gcm_rows_run_mfma(run) == (1 if form == "mfma" else 0)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for t in range(first, T):
                    if t == split:
                        other.add_(1.0)
                    assert lib.gcm_dense_rows_step_cached_run(run, *common(t), _hip.stream()) == 0, t
            out2 = (ctypes.c_int * 2)()
            assert lib.gcm_rows_run_stats(run, out2) == 0
            stats = (out2[0], out2[1])
            graph.replay()
        finally:
            torch.cuda.synchronize()
            lib.gcm_rows_run_destroy(run)
    torch.cuda.synchronize()
    out = {k: buf[k].view(torch.int32).clone() for k in KEYS}
    out["count"], out["flags"] = buf["count"].clone(), buf["flags"].clone()
    return out, stats


@functools.lru_cache(maxsize=None)
def _reference(hops, N, H2, B, T, record=True, nan_at=None):
    return _chain("steps", list(hops), N, H2, B, T, record=record, nan_at=nan_at)[0]


def _three_ways(hops, N, H2=32, B=3, T=None, first=0, record=True, split=None):
    T = N if T is None else T
    want = _reference(tuple(hops), N, H2, B, T, record)
    runs = 1 if split is None else 2
    for form in ("mfma", "valu"):
        got, stats = _chain(form, hops, N, H2, B, T, first=first, record=record, split=split)
        assert stats == (runs, T - first - runs), (form, stats)
        assert int(got["flags"].item()) == 0 and int(want["flags"].item()) == 0
        assert torch.equal(got["count"], want["count"]) and int(got["count"][0]) == T
        for k in KEYS:
            assert torch.equal(got[k], want[k]), (form, k)
    return want


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 128])
def test_run_lengths_against_the_tiles(n):
    """runs of n steps from row 0 at N = 128: less than a tile, a tile less one, a tile, a tile and a row, two tiles
    and a row, all eight (n = 1 is the per-step kernel's node: nothing was appended)"""
    want = _three_ways([1, 2, 4], 128, T=n)
    assert bool((want["cH"][:, n:] == NAN_SENTINEL).all()) and bool((want["cH"][:, :n] != NAN_SENTINEL).all())


@pytest.mark.parametrize("first", [2, 9, 21])
def test_run_starts_inside_the_graph(first):
    """eager steps first, then the captured run from row cur0 = first of 36: below max(hop) = 4 (the run's first rows
    still have empty slots), beyond it, and with the rows before it spread over two tiles of the earlier steps; the
    source rows before cur0 come from nodes / cH"""
    _three_ways([1, 2, 4], 36, first=first)


@pytest.mark.parametrize("hops", [[1, 2, 4], [1], [0], [0, 3, 5], [1, 2, 40]])
def test_hop_sets(hops):
    """three slots, one, none but the row itself, self and two slots, and a hop past N = 36 that never reaches a row"""
    _three_ways(hops, 36)


@pytest.mark.parametrize("N", [8, 36, 128])
def test_graph_sizes(N):
    _three_ways([0, 1, 2, 4], N)


@pytest.mark.parametrize("H2", [32, 24, 1])
def test_belief_widths(H2):
    """H2 < 32: the zero weight rows of layer 2 and the store mask over both column tiles (24: the second tile half
    stored; 1: one column of the first)"""
    want = _three_ways([1, 2, 4], 36, H2=H2)
    assert bool((want["saved"][:, :3 * H2] != NAN_SENTINEL).all())


@pytest.mark.parametrize("B", [1, 3])
def test_batch_sizes(B):
    _three_ways([1, 2, 4], 20, B=B)


def test_no_record():
    """record = 0 (a no_grad loop): the belief alone is written"""
    want = _three_ways([1, 2, 4], 36, record=False)
    assert bool((want["saved"][:, 3 * 32:] == NAN_SENTINEL).all())


def test_two_runs_in_one_capture():
    """a kernel of someone else's in front of step 17: two nodes, the second starts one row into the second tile"""
    _three_ways([1, 2, 4], 36, split=17)


def test_nan_observation():
    """one NaN in the observation of step 5: the flag word is raised by all three, the same words are NaN, and every
    other word is the same (NaN payloads are not compared)"""
    args = ((1, 2, 4), 36, 32, 3, 36)
    nan_at = (5, 1, 7)
    want = _reference(*args, True, nan_at)
    assert int(want["flags"].item()) != 0
    for form in ("mfma", "valu"):
        got, stats = _chain(form, list(args[0]), *args[1:], nan_at=nan_at)
        assert stats == (1, 35)
        assert torch.equal(got["flags"], want["flags"]) and torch.equal(got["count"], want["count"])
        for k in KEYS:
            a, b = got[k], want[k]
            na, nb = torch.isnan(a.view(torch.float32)), torch.isnan(b.view(torch.float32))
            assert torch.equal(na, nb), (form, k)
            assert torch.equal(a[~na], b[~nb]), (form, k)
    assert bool(torch.isnan(want["cH"].view(torch.float32)).any())


def test_module_switch_and_fresh_form():
    """DenseGCM.rows_run_mfma through the module: the rollout from hidden = None (the head absorbed: the kernel's
    fresh-state form), forward and backward captured, switch on / off / merging off - the same bits, and merge_stats
    reports the form"""
    from test_step_run_gpu import _capture, _data, _loop, _module, _replay, _same, _snapshot
    obs, w = _data(24, steps=20)
    snaps = []
    for merge, mfma in ((True, True), (True, False), (False, True)):
        g, mem = _module(24, merge, N=20)
        mem.rows_run_mfma = mfma
        graph, res = _capture(mem, g, lambda: _loop(mem, obs, w, None, True))
        stats = mem.merge_stats(form=True)
        _replay(graph, g)
        snaps.append(_snapshot(mem, g, *res))
        if merge:
            assert stats == {"nodes": 1, "merged_steps": 19, "run_mfma": mfma}
    _same(snaps[0], snaps[1])
    _same(snaps[0], snaps[2])
