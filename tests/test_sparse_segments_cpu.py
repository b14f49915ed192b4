"""Episode resets inside one SparseGCM call (rollout(x, reset=mask)) without a GPU: the segment
expansion restated in plain torch and pinned against the oracle stepping one node at a time with reset_ref in
between, its own properties, the public signatures and argument checks (raised before any device call), and the ABI
section."""
import inspect

import pytest
import torch

from _sparse_segments_restate import (MASKS, SEEDS, SHAPES, collect_ref, expand_ref, mask_case, oneshot_ref, plan_ref,
                                      random_case, stepwise_ref, valid_resets)
from _sparse_window_restate import is_sorted_coo, random_causal_state, reset_ref, state_equal
from oracle import sparse as osp

B, N, F, H, t = 4, 16, 3, 5, 12


def _incoming(sel, gnn, seed):
    """A non-empty stored state the module could have made: one oracle call of up to 3 nodes per graph."""
    gen = torch.Generator().manual_seed(seed)
    taus0 = torch.tensor([3, 0, 2, 1])
    x0 = torch.rand(B, 3, F, dtype=torch.float64, generator=gen)
    x0 = x0 * (torch.arange(3)[None, :] < taus0[:, None])[:, :, None]
    h0 = osp.initial_hidden(x0, N)
    with torch.no_grad():
        _, hidden = osp.sparse_step(x0, taus0, (h0[0].double(), h0[1], h0[2]), gnn, graph_size=N, edge_selectors=sel)
    return hidden


@pytest.mark.parametrize("incoming", [False, True])
@pytest.mark.parametrize("max_hops", [None, 2])
@pytest.mark.parametrize("hops", [[1], [1, 2, 4]])
def test_expansion_equals_stepping_with_resets(hops, max_hops, incoming):
    """expand_ref -> ONE oracle call -> collect_ref == one oracle call per node with reset_ref between them, float64:
    beliefs and d/dx to 1e-12, the state exactly."""
    torch.manual_seed(len(hops) * 10 + (max_hops or 0))
    gnn = osp.canonical_gnn(F, H).double()
    sel = osp.TemporalEdge(hops)
    taus, mask = random_case(B, t, SEEDS[(B, t)])
    hidden = _incoming(sel, gnn, 3) if incoming else None
    x = torch.rand(B, t, F, dtype=torch.float64)
    x = x * (torch.arange(t)[None, :] < taus[:, None])[:, :, None]
    w = torch.rand(B, t, H, dtype=torch.float64)
    res = []
    for fn in (oneshot_ref, stepwise_ref):
        xi = x.clone().requires_grad_(True)
        out, state = fn(xi, taus, hidden, mask, gnn, N, edge_selectors=sel, max_hops=max_hops)
        (out * w).sum().backward()
        res.append((out.detach(), state, xi.grad))
    (o1, s1, g1), (o2, s2, g2) = res
    torch.testing.assert_close(o1, o2, rtol=0, atol=1e-12)
    torch.testing.assert_close(g1, g2, rtol=0, atol=1e-12)
    assert float(g2.abs().max()) > 0
    assert state_equal((s1[0].detach(), s1[1].detach(), s1[2]), (s2[0].detach(), s2[1].detach(), s2[2]))
    pad = torch.arange(t)[None, :] >= taus[:, None]
    assert not o1[pad].any()


def _state(seed=0, **kw):
    return random_causal_state(4, 9, 3, 0.5, seed=seed, **kw)


def _x(Bx, tx, Fx, seed=0):
    return torch.rand(Bx, tx, Fx, generator=torch.Generator().manual_seed(seed))


def test_no_valid_reset_is_the_identity():
    h = _state()
    x = _x(4, 6, 3)
    taus = torch.tensor([6, 2, 0, 6])
    for mask in (torch.zeros(4, 6, dtype=torch.bool), torch.arange(6)[None, :] >= taus[:, None]):
        xs, taus_s, hs, plan = expand_ref(x, taus, h, mask)
        live = (torch.arange(6)[None, :] < taus[:, None])[:, :, None]
        assert torch.equal(xs, x * live) and torch.equal(taus_s, taus) and state_equal(hs, h)
        out, back = collect_ref(xs, hs, plan, 4, 6)
        assert torch.equal(out, x * live) and state_equal(back, h)


def test_reset_in_every_column_leaves_every_node_alone():
    h = _state()
    taus = torch.tensor([5, 2, 0, 1])
    xs, taus_s, hs, (segs, vbase) = expand_ref(_x(4, 5, 3), taus, h, torch.ones(4, 5, dtype=torch.bool))
    assert vbase == [0, 6, 9, 10, 12] and xs.shape[1] == 1
    # every graph with a node: an empty head of length 0, then one virtual graph per node; graph 2 (tau = 0) is kept
    assert [l for _, _, l, _ in segs] == [0, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1]
    assert [e for _, _, _, e in segs] == [1] * 9 + [0] + [1, 1]
    assert not hs[0][:9].any() and not hs[0][10:].any() and torch.equal(hs[0][9], h[0][2])
    idx = hs[1].coalesce().indices()
    assert set(idx[0].tolist()) <= {9}
    assert hs[2].tolist() == [0] * 9 + [int(h[2][2])] + [0, 0]


def test_reset_in_column_zero_is_reset_hidden_then_the_call():
    torch.manual_seed(0)
    gnn = osp.canonical_gnn(F, H).double()
    sel = osp.TemporalEdge([1, 2])
    hidden = _incoming(sel, gnn, 5)
    x = torch.rand(B, 4, F, dtype=torch.float64)
    taus = torch.tensor([4, 4, 0, 2])
    mask = torch.zeros(B, 4, dtype=torch.bool)
    mask[:, 0] = torch.tensor([True, False, True, True])
    with torch.no_grad():
        got_o, got = oneshot_ref(x * (torch.arange(4)[None, :] < taus[:, None])[:, :, None], taus, hidden, mask, gnn, N,
                                 edge_selectors=sel)
        cleared = reset_ref(hidden, mask[:, 0] & (taus > 0))
        want_o, want = osp.sparse_step(x, taus, cleared, gnn, graph_size=N, edge_selectors=sel)
    torch.testing.assert_close(got_o, want_o, rtol=0, atol=1e-12)
    assert state_equal(got, want)
    assert int(got[2][2]) == int(hidden[2][2]) > 0         # (tau = 0: the flag does not touch graph 2)


def test_padding_flags_and_empty_rows_are_ignored():
    h = _state()
    x = _x(4, 6, 3)
    taus = torch.tensor([3, 0, 6, 9])                       # (9 > t: clamped to t)
    mask = torch.zeros(4, 6, dtype=torch.bool)
    mask[0, 1] = mask[2, 4] = True
    noisy = mask.clone()
    noisy[0, 3:] = True
    noisy[1, :] = True
    a, b = expand_ref(x, taus, h, mask), expand_ref(x, taus, h, noisy)
    assert a[3] == b[3] and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and state_equal(a[2], b[2])
    assert a[3][1] == [0, 2, 3, 5, 6]


@pytest.mark.parametrize("pattern", MASKS)
def test_expanded_list_is_sorted_and_duplicate_free(pattern):
    Bx, Nx, Fx, tx, d = SHAPES[2]
    h = random_causal_state(Bx, Nx, Fx, d, seed=1)
    taus, mask = mask_case(Bx, tx, pattern)
    xs, taus_s, hs, plan = expand_ref(_x(Bx, tx, Fx), taus, h, mask)
    idx = hs[1]._indices()                                  # as built, before any coalesce()
    assert is_sorted_coo(idx, Nx) and torch.equal(hs[1].coalesce().indices(), idx)
    _, back = collect_ref(xs, hs, plan, Bx, tx)
    assert is_sorted_coo(back[1]._indices(), Nx)


def test_gpu_random_masks_cover_the_interesting_graphs():
    """Every random case of the GPU tests has a graph with two or more valid resets, one with none and one with a
    valid reset in column 0.  (B = 1, t = 1 has one graph and one column: it cannot, and is left out.)"""
    cases = [(Bx, tx) for Bx, _, _, tx, _ in SHAPES if Bx > 1] + [(4, 12)]
    assert set(cases) == set(SEEDS)
    for Bx, tx in cases:
        taus, mask = random_case(Bx, tx, SEEDS[(Bx, tx)])
        v = valid_resets(taus, mask)
        n = v.sum(1)
        assert bool((n >= 2).any()) and bool((n == 0).any()) and bool(v[:, 0].any()), (Bx, tx)
        assert torch.equal(mask_case(Bx, tx, "random")[1], mask)
    taus, _ = random_case(4, 12, SEEDS[(4, 12)])
    assert int(taus.max()) + 3 <= N                         # (the end-to-end case fits behind _incoming's 3 nodes)


# ---- the public interface ----

def test_reset_is_the_last_keyword_of_both_signatures():
    from gcm.sparse_gcm import SparseGCM
    for fn, names in ((SparseGCM.rollout, ["self", "x", "hidden", "taus", "reset"]),
                      (SparseGCM.forward, ["self", "x", "taus", "hidden", "reset"])):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == names
        assert sig.parameters["reset"].default is None


def test_reset_argument_checks_come_before_any_launch():
    from gcm.sparse_gcm import SparseGCM
    mem = SparseGCM(torch.nn.Identity(), graph_size=9)
    h = _state()                      # (CPU tensors: a device call would raise HipLibraryError instead)
    x, taus = _x(4, 6, 3), torch.full((4,), 6)
    for call in (lambda r: mem.rollout(x, h, taus, reset=r), lambda r: mem.forward(x, taus, h, reset=r),
                 lambda r: mem.rollout(x, reset=r)):
        for bad in (torch.zeros(4, 6, dtype=torch.uint8), torch.zeros(4, 6), [[True] * 6] * 4, 1):
            with pytest.raises(TypeError, match="bool"):
                call(bad)
        for bad in (torch.zeros(4, dtype=torch.bool), torch.zeros(6, 4, dtype=torch.bool),
                    torch.zeros(4, 6, 1, dtype=torch.bool), torch.zeros(4, 5, dtype=torch.bool)):
            with pytest.raises(ValueError, match="shape"):
                call(bad)


def test_segment_section_of_the_abi():
    """The header section is read like the others, is part of gcm_hip.h, and leaves the ABI revision alone."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_segments.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[A-Za-z0-9_]+)\s*\(", _abi.header("gcm_hip_segments.h")))
    assert declared == set(_hip.SEGMENT_PROTOTYPES) == {
        "gcm_sparse_seg_plan", "gcm_sparse_seg_rows", "gcm_sparse_seg_nodes", "gcm_sparse_seg_edges_plan",
        "gcm_sparse_seg_edges", "gcm_sparse_seg_final_T"}
    assert not declared & set(_hip.PROTOTYPES) and not declared & set(_hip.WINDOW_PROTOTYPES)
    assert _hip._CONSTANTS["GCM_ABI_VERSION"] == 8
    assert _hip.SPARSE_SEG_CHUNK == 1024 and _hip.SPARSE_SEG_ROWS == 6 and _hip.SPARSE_SEG_TOTALS == 4
