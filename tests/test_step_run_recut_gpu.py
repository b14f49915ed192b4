"""The re-cut multi-step kernel (csrc/rows_cached_run.hip): source rows at fixed distances from row
max(hop) on, the general resolution before it; adjacency entries, live lists, coefficients and headers written eight
lanes per step in closed form; two steps per pass of a wave, one per half-wave.  Every comparison is torch.equal (or
equality of the raw words) against what the per-step launches write.

Shapes: F = H1 = 32, B = 3.  N = T = 16 puts the boundary between the two source paths (row max(hop)) inside one
pass of the waves; hops [1, 2, 4, 20] never leave the general path; hops [1, 2, 4, 100] at N = T = 128 keep it for
more than one pass and past row 64.  Caps of 1 - 17 steps per node give runs that fill no pass, exactly one, and one
plus a step, and later nodes that start inside and past the prefix."""
import ctypes

import pytest
import torch

from test_dense_gpu import DEV
from test_step_run_gpu import _captured, _data, _same, F, H1

pytestmark = pytest.mark.gpu

B = 3
IMG_V4 = 64


def _on_off(H2, hops, n, grad=True, cap=None):
    obs, w = _data(H2, steps=n)
    on, st_on, *_ = _captured(H2, True, obs, w, grad=grad, cap=cap, N=n, hops=hops)
    off, st_off, *_ = _captured(H2, False, obs, w, grad=grad, N=n, hops=hops)
    assert st_off == {"nodes": 0, "merged_steps": 0}
    _same(on, off)
    return st_on


@pytest.mark.parametrize("H2", [32, 8])
@pytest.mark.parametrize("hops", [[3, 7], [1], [1, 2, 4], [0, 1, 2, 4]])
def test_fast_path_boundary_inside_a_pass(hops, H2):
    """N = T = 16: rows below max(hop) resolve their sources step by step, the rows from there on read them at fixed
    distances - both inside the first pass of the waves; one, two, three and four slots, with and without self"""
    assert _on_off(H2, hops, 16) == {"nodes": 1, "merged_steps": 15}


def test_largest_hop_past_graph_size():
    """hops [1, 2, 4, 20] at N = 16: max(hop) >= N, no row ever takes the fixed-distance path"""
    assert _on_off(32, [1, 2, 4, 20], 16) == {"nodes": 1, "merged_steps": 15}


def test_prefix_longer_than_a_pass():
    """hops [1, 2, 4, 100] at N = T = 128: a hundred rows of prefix (more than one pass of all waves), then 28 rows
    with four slots; rows past 64"""
    assert _on_off(32, [1, 2, 4, 100], 128) == {"nodes": 1, "merged_steps": 127}


@pytest.mark.parametrize("cap", [1, 2, 5, 15, 16, 17])
def test_run_lengths_and_starts(cap):
    """T = N = 128, hops [1, 2, 4], ceil(128 / cap) nodes of cap steps: runs shorter than the waves, one pass exactly,
    one pass and a step; every node but the first starts from rows earlier nodes wrote, inside and past the prefix"""
    nodes = -(-128 // cap)
    merged = 128 - nodes if cap > 1 else 0
    assert _on_off(32, [1, 2, 4], 128, cap=cap) == {"nodes": nodes, "merged_steps": merged}


def test_no_grad_narrow_belief():
    """no_grad (the record is the belief alone) at H2 = 8, hops [3, 7], N = T = 16"""
    assert _on_off(8, [3, 7], 16, grad=False) == {"nodes": 1, "merged_steps": 15}


# ---- records word for word, through the C ABI (the test owns every buffer) ------------------------------------------
SENTINEL = 0x7FC0BEEF   # a NaN payload no kernel produces


def _buffers(lib, _hip, N, H2, T, record):
    lay = (ctypes.c_size_t * 5)()
    assert lib.gcm_dense_rows_cached_layout(B, N, F, H1, H2, ctypes.addressof(lay)) == 0
    words = int(lay[0]) if record else B * H2

    def fill(*shape):
        return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)

    return dict(nodes=fill(B, N, F), adj=fill(B, N, N), cH=fill(B, N, H1), cA=fill(B, N, F), cX=fill(B, N, F),
                count=torch.zeros(B, dtype=torch.int64, device=DEV), flags=torch.zeros(1, dtype=torch.int32, device=DEV),
                saved=fill(T, int(lay[0])), words=words)


def _abi_chain(lib, _hip, hops, N, H2, T, record, merged):
    """T cached steps from row 0 on sentinel-filled buffers: one by one through gcm_dense_rows_step_cached_ws, or
    captured through gcm_dense_rows_step_cached_run (one node) and replayed once -> the buffers"""
    g = torch.Generator().manual_seed(7 * N + H2)
    P = lib.gcm_dense_gnn2_param_count(F, H1, H2)
    params = (torch.randn(P, generator=g) * 0.2).to(DEV)
    obs = torch.rand(T, B, F, generator=g).to(DEV)
    img = torch.empty(lib.gcm_dense_rows_cached_weight_image_floats(), device=DEV)
    p = _hip.ptr
    assert lib.gcm_dense_rows_cached_weight_image(p(params), p(img), F, H1, H2, _hip.stream()) == 0
    d = _hip.SelectorDesc(kind=_hip.SEL_TEMPORAL, n_hops=len(hops), direction=_hip.DIR["forward"])
    for i, h in enumerate(hops):
        d.hops[i] = h
    arr = (_hip.SelectorDesc * 1)(d)
    buf = _buffers(lib, _hip, N, H2, T, record)
    common = lambda t: (p(obs[t]), p(buf["nodes"]), p(buf["adj"]), p(buf["count"]), ctypes.addressof(arr), 1, p(params),  # noqa: E731
                        p(img), 3 | IMG_V4, 1, 1, p(buf["cH"]), p(buf["cA"]), p(buf["cX"]), p(buf["saved"][t]),
                        1 if record else 0, t, p(buf["flags"]), None, 0, B, N, F, H1, H2)
    torch.cuda.synchronize()
    if not merged:
        for t in range(T):
            assert lib.gcm_dense_rows_step_cached_ws(*common(t), _hip.stream()) == 0, t
    else:
        run = lib.gcm_rows_run_create()
        assert run
        try:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for t in range(T):
                    assert lib.gcm_dense_rows_step_cached_run(run, *common(t), _hip.stream()) == 0, t
            stats = (ctypes.c_int * 2)()
            assert lib.gcm_rows_run_stats(run, stats) == 0
            assert (stats[0], stats[1]) == (1, T - 1)
            graph.replay()
        finally:
            torch.cuda.synchronize()
            lib.gcm_rows_run_destroy(run)
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("N", [16, 128])
@pytest.mark.parametrize("record", [True, False])
@pytest.mark.parametrize("self_loop", [True, False])
def test_records_and_state_word_for_word(self_loop, record, N):
    """hops [1, 2, 4] (+ 0): every word of every record, of the state and of the caches after the merged node equals
    what the per-step launches leave - the sentinel wherever a step writes nothing, so a stray or missing store of the
    lane-parallel bookkeeping shows"""
    from gcm import _hip
    lib = _hip.lib()
    hops = ([0] if self_loop else []) + [1, 2, 4]
    want = _abi_chain(lib, _hip, hops, N, 32, N, record, merged=False)
    got = _abi_chain(lib, _hip, hops, N, 32, N, record, merged=True)
    assert int(want["flags"].item()) == 0 and int(got["flags"].item()) == 0
    assert torch.equal(got["count"], want["count"]) and int(got["count"][0]) == N
    for k in ("nodes", "adj", "cH", "cA", "cX", "saved"):
        assert torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)), k
    sv = got["saved"].view(torch.int32)
    assert bool((sv[:, got["words"]:] == SENTINEL).all())       # nothing behind the record form's last word
    assert bool((sv[:, :B * 32] != SENTINEL).all())             # the beliefs were written
    assert int((got["adj"].view(torch.int32) != SENTINEL).sum()) == \
        B * sum(sum(1 for h in hops if h <= t) for t in range(N))
