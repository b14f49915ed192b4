"""SparseGCM's sliding window (drop_oldest / reset_hidden / overflow="wrap") without a GPU: the
plain-torch restatement of the primitive pinned against oracle/, its own properties, and the argument checks of the
public interface (raised before any device call)."""
import inspect

import pytest
import torch

from _sparse_window_restate import drop_oldest_ref, is_sorted_coo, random_causal_state, state_equal, wrap_k
from oracle import dense as od, sparse as osp

B, N, F, H = 3, 6, 4, 5
HOPS = [[1], [1, 2], [4, 2, 1], [5]]


def _taus(step):
    """Ragged starts (graph b receives nothing before step b) and a pause of graph 1 now and then."""
    t = torch.tensor([1 if step >= b else 0 for b in range(B)])
    if step % 5 == 3:
        t[1] = 0
    return t


@pytest.mark.parametrize("hops", HOPS)
def test_window_equals_fresh_memory(hops):
    """Stepping with the wrap drop ahead of every step == a fresh memory fed each graph's last min(len, N)
    observations in one call: state exactly, the new node's belief to 1e-12 in float64."""
    torch.manual_seed(0)
    gnn = osp.canonical_gnn(F, H).double()
    sel = osp.TemporalEdge(hops)
    steps = 15
    obs = torch.rand(B, steps, F, dtype=torch.float64)
    hidden = (torch.zeros(B, N, F, dtype=torch.float64), torch.zeros((B, N, N), layout=torch.sparse_coo),
              torch.zeros(B, dtype=torch.long))
    seen = [[] for _ in range(B)]
    for s in range(steps):
        taus = _taus(s)
        hidden = drop_oldest_ref(hidden, wrap_k(hidden[2], taus, N))
        out, hidden = osp.sparse_step(obs[:, s:s + 1], taus, hidden, gnn, graph_size=N, edge_selectors=sel)
        for b in range(B):
            if taus[b]:
                seen[b].append(obs[b, s])
        lens = torch.tensor([min(len(v), N) for v in seen])
        xf = torch.zeros(B, int(lens.max()), F, dtype=torch.float64)
        for b in range(B):
            if lens[b]:
                xf[b, :lens[b]] = torch.stack(seen[b][-int(lens[b]):])
        h0 = (torch.zeros(B, N, F, dtype=torch.float64), torch.zeros((B, N, N), layout=torch.sparse_coo),
              torch.zeros(B, dtype=torch.long))
        out_f, fresh = osp.sparse_step(xf, lens, h0, gnn, graph_size=N, edge_selectors=sel)
        assert torch.equal(hidden[0], fresh[0]), s
        assert torch.equal(hidden[1].coalesce().indices(), fresh[1].coalesce().indices()), s
        assert torch.equal(hidden[2], fresh[2]), s
        for b in range(B):
            if taus[b]:
                torch.testing.assert_close(out[b, 0], out_f[b, int(lens[b]) - 1], rtol=0, atol=1e-12)


@pytest.mark.parametrize("hops", HOPS)
def test_sparse_with_wrap_equals_dense(hops):
    """The same loop beside oracle.dense.dense_step + TemporalBackedge(hops), 14 steps, well past N: nodes, edge sets
    and counts exactly, beliefs at the bound of test_sparse_rollout_matches_reference.  The dense graphs are
    independent, so each runs alone from its own (ragged) start and rests while its sparse twin has tau = 0."""
    torch.manual_seed(1)
    sgnn = osp.canonical_gnn(F, H)
    dgnn = od.canonical_gnn(F, H)
    dgnn.load_state_dict(sgnn.state_dict())
    ssel, dsel = osp.TemporalEdge(hops), od.TemporalBackedge(hops)
    steps = 14
    obs = torch.rand(B, steps, F)
    hidden = None
    dense = [None] * B
    worst = 0.0
    for s in range(steps):
        taus = _taus(s)
        if hidden is not None:
            hidden = drop_oldest_ref(hidden, wrap_k(hidden[2], taus, N))
        out, hidden = osp.sparse_step(obs[:, s:s + 1], taus, hidden, sgnn, graph_size=N, edge_selectors=ssel)
        for b in range(B):
            if taus[b]:
                dout, dense[b] = od.dense_step(obs[b:b + 1, s], dense[b], dgnn, graph_size=N, edge_selectors=dsel)
                worst = max(worst, float((dout[0] - out[b, 0]).detach().abs().max()))
                torch.testing.assert_close(out[b, 0], dout[0], rtol=1e-5, atol=1e-5)
            if dense[b] is None:
                assert int(hidden[2][b]) == 0
                continue
            idx = hidden[1].coalesce().indices()
            assert torch.equal(hidden[0][b], dense[b][0][0]), (s, b)
            assert torch.equal(idx[1:, idx[0] == b], dense[b][1][0].nonzero().T), (s, b)
            assert int(hidden[2][b]) == int(dense[b][3][0]), (s, b)
    assert int(hidden[2].max()) == N        # (the loop did run past N)
    print("worst belief difference: %.3g" % worst)


def _state(seed=0, **kw):
    return random_causal_state(4, 9, 3, 0.5, seed=seed, **kw)


def test_zero_is_the_identity():
    h = _state()
    assert state_equal(drop_oldest_ref(h, torch.zeros(4, dtype=torch.long)), h)


def test_all_gives_an_empty_state():
    h = _state(T=torch.tensor([9, 4, 0, 7]))
    nodes, adj, T = drop_oldest_ref(h, h[2].clone())
    assert not nodes.any() and adj.coalesce()._nnz() == 0 and not T.any()


def test_k_clamps_into_zero_to_T():
    h = _state(T=torch.tensor([9, 4, 0, 7]))
    k = torch.tensor([12, -3, 5, 2])
    assert state_equal(drop_oldest_ref(h, k), drop_oldest_ref(h, torch.tensor([9, 0, 0, 2])))


def test_two_drops_compose():
    h = _state(seed=3, T=torch.tensor([9, 5, 2, 8]))
    a, b = torch.tensor([2, 1, 0, 4]), torch.tensor([3, 4, 2, 1])
    assert bool((a + b <= h[2]).all())
    assert state_equal(drop_oldest_ref(drop_oldest_ref(h, a), b), drop_oldest_ref(h, a + b))


def test_output_is_coalesced_and_sorted():
    h = _state(seed=5, T=torch.tensor([9, 9, 3, 6]))
    nodes, adj, T = drop_oldest_ref(h, torch.tensor([1, 4, 1, 0]))
    idx = adj._indices()                      # as built, before any coalesce()
    assert is_sorted_coo(idx, 9)
    assert bool((idx[1] > idx[2]).all()) and bool((idx[2] >= 0).all()) and bool((idx[1] < T[idx[0]]).all())
    assert torch.equal(adj.coalesce().indices(), idx)
    assert not nodes[torch.arange(9)[None, :] >= T[:, None]].any()


# ---- the public interface: argument checks, before any device call ----

def _mem(**kw):
    from gcm.sparse_gcm import SparseGCM
    return SparseGCM(torch.nn.Identity(), graph_size=9, **kw)


def test_overflow_keyword():
    from gcm.sparse_gcm import SparseGCM
    assert _mem().overflow == "raise"
    assert _mem(overflow="wrap").overflow == "wrap"
    for bad in ("roll", "", None, True):
        with pytest.raises(ValueError, match="overflow"):
            _mem(overflow=bad)
    params = list(inspect.signature(SparseGCM.__init__).parameters)
    assert params == ["self", "gnn", "preprocessor", "edge_selectors", "aux_edge_selectors", "graph_size", "max_hops",
                      "positional_encoder", "finite_check", "overflow"]
    assert inspect.signature(SparseGCM.__init__).parameters["overflow"].default == "raise"


def test_drop_oldest_argument_checks():
    mem, h = _mem(), _state()         # (CPU tensors: a device call would raise HipLibraryError instead)
    for bad in (torch.zeros(4, dtype=torch.int32), torch.zeros(4), [0, 0, 0, 0], 1):
        with pytest.raises(TypeError, match="int64"):
            mem.drop_oldest(h, bad)
    for bad in (torch.zeros(3, dtype=torch.long), torch.zeros(4, 1, dtype=torch.long), torch.zeros((), dtype=torch.long)):
        with pytest.raises(ValueError, match="shape"):
            mem.drop_oldest(h, bad)


def test_reset_hidden_argument_checks():
    mem, h = _mem(), _state()
    for bad in (torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.long), [True] * 4, None):
        with pytest.raises(TypeError, match="bool"):
            mem.reset_hidden(h, bad)
    for bad in (torch.zeros(5, dtype=torch.bool), torch.zeros(1, 4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="shape"):
            mem.reset_hidden(h, bad)


def test_window_section_of_the_abi():
    """The header section is read like the others, is part of gcm_hip.h, and leaves the ABI revision alone."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_window.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_window.h")))
    assert declared == set(_hip.WINDOW_PROTOTYPES) == {"gcm_sparse_drop_plan", "gcm_sparse_drop_nodes",
                                                       "gcm_sparse_drop_edges", "gcm_sparse_drop_values_bwd"}
    assert not declared & set(_hip.PROTOTYPES)
    assert _hip._CONSTANTS["GCM_ABI_VERSION"] == 8 and _hip.SPARSE_DROP_CHUNK == 1024
