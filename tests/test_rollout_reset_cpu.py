"""Per-graph episode resets (DenseGCM.rollout(reset=...), DenseGCM.reset_hidden) host side: the restatement the GPU
tests compare against pinned by per-episode oracle runs, the argument checks, and the C ABI section.  No kernel runs."""
import os
import re

import pytest
import torch

from _reset_restate import clear_graphs, per_episode_rollout, reset_rollout
from oracle import dense as od


def _mem(sel, N=8, F=4, H=8, **kw):
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    g = G.Sequential("x, adj, weights, B, N", [(G.DenseGraphConv(F, H), "x, adj -> x"), torch.nn.Tanh(),
                                               (G.DenseGraphConv(H, H), "x, adj -> x"), torch.nn.Tanh()])
    return DenseGCM(g, edge_selectors=sel, graph_size=N, **kw)


# ---- the restatement ------------------------------------------------------------------------------
def test_restatement_equals_per_episode_oracle_runs():
    """reset_rollout (one batched loop, masked graphs times zero before the step) against every episode of every graph
    run on its own from hidden = None: beliefs, final state and counts bit for bit.  B = 5, N = 8, T = 21, hops [1, 3],
    14 resets: episodes longer than the graph (overflow roll), a reset at t = 0, resets at consecutive steps, at T - 1."""
    torch.manual_seed(3)
    B, N, F, H, T = 5, 8, 4, 8, 21
    ref = od.canonical_gnn(F, H)
    obs = torch.rand(T, B, F)
    reset = torch.zeros(T, B, dtype=torch.bool)
    for t, b in [(0, 0), (5, 0), (6, 0), (20, 0), (3, 1), (13, 1), (1, 2), (2, 2), (3, 2), (12, 2), (10, 3), (19, 3),
                 (20, 3), (7, 1)]:
        reset[t, b] = True           # (graph 4 is never reset: 21 steps through a graph of 8)
    assert int(reset.sum()) == 14
    sel = lambda: od.TemporalBackedge([1, 3], "forward")      # noqa: E731
    with torch.no_grad():
        out, hid = reset_rollout(obs, reset, None, ref, graph_size=N, edge_selectors=sel())
        out_e, hid_e = per_episode_rollout(obs, reset, ref, N, sel)
    assert torch.equal(out, out_e)
    assert torch.equal(hid[0], hid_e[0]) and torch.equal(hid[1], hid_e[1]) and torch.equal(hid[3], hid_e[3])
    assert hid[3].tolist() == [1, 8, 8, 1, 8]


def test_clear_graphs_is_out_of_place_and_differentiable():
    nodes = torch.rand(3, 4, 2, requires_grad=True)
    adj, w, count = torch.ones(3, 4, 4), torch.zeros(0), torch.tensor([2, 4, 1])
    mask = torch.tensor([False, True, False])
    n2, a2, w2, c2 = clear_graphs((nodes, adj, w, count), mask)
    assert torch.equal(n2[1], torch.zeros(4, 2)) and torch.equal(n2[0], nodes[0].detach()) and w2 is w
    assert torch.equal(a2[1], torch.zeros(4, 4)) and c2.tolist() == [2, 0, 1] and count.tolist() == [2, 4, 1]
    n2.sum().backward()
    assert torch.equal(nodes.grad[1], torch.zeros(4, 2)) and torch.equal(nodes.grad[0], torch.ones(4, 2))


# ---- argument checks: before any launch (no device here) ----------------------------------------------
def test_rollout_reset_argument_checks():
    from gcm.edge_selectors.temporal import TemporalBackedge
    mem = _mem(TemporalBackedge([1]))
    T, B = 6, 3
    obs = torch.rand(T, B, 4)
    with pytest.raises(TypeError, match="bool"):
        mem.rollout(obs, reset=torch.zeros(T, B))
    with pytest.raises(TypeError, match="bool"):
        mem.rollout(obs, reset=torch.zeros(T, B, dtype=torch.uint8))
    with pytest.raises(TypeError, match="bool"):
        mem.rollout(obs, reset=[[False] * B] * T)
    with pytest.raises(ValueError, match="shape"):
        mem.rollout(obs, reset=torch.zeros(B, T, dtype=torch.bool))
    with pytest.raises(ValueError, match="shape"):
        mem.rollout(obs, reset=torch.zeros(T, dtype=torch.bool))
    with pytest.raises(ValueError, match="shape"):       # batch_first: obs [B, T, F] wants reset [B, T]
        mem.rollout(obs.transpose(0, 1), batch_first=True, reset=torch.zeros(T, B, dtype=torch.bool))
    with pytest.raises(ValueError, match="shape"):
        mem.rollout(obs, reset=torch.zeros(T, B, 1, dtype=torch.bool))


def test_reset_hidden_argument_checks():
    from gcm.edge_selectors.temporal import TemporalBackedge
    mem = _mem(TemporalBackedge([1]))
    hidden = mem.get_initial_hidden_state(torch.zeros(3, 4))
    with pytest.raises(TypeError, match="bool"):
        mem.reset_hidden(hidden, torch.zeros(3))
    with pytest.raises(ValueError, match="shape"):
        mem.reset_hidden(hidden, torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="shape"):
        mem.reset_hidden(hidden, torch.zeros(3, 1, dtype=torch.bool))


def test_learned_edge_with_reset_is_not_implemented():
    from gcm import nn as G
    from gcm.edge_selectors.learned import LearnedEdge
    from gcm.edge_selectors.temporal import TemporalBackedge
    T, B = 4, 2
    obs, reset = torch.rand(T, B, 4), torch.zeros(T, B, dtype=torch.bool)
    chained = G.Sequential("x, adj, weights, num_nodes, B", [
        (TemporalBackedge([1]), "x, adj, weights, num_nodes, B -> adj, weights"),
        (LearnedEdge(4), "x, adj, weights, num_nodes, B -> adj, weights")])
    for mem in (_mem(LearnedEdge(4)), _mem(chained), _mem(LearnedEdge(4, deterministic=True))):
        with pytest.raises(NotImplementedError, match="LearnedEdge"):
            mem.rollout(obs, reset=reset)
        with pytest.raises(NotImplementedError, match="LearnedEdge"):
            mem.reset_hidden(mem.get_initial_hidden_state(obs[0]), reset[0])
    from gcm.gcm import DenseGCM
    aux = DenseGCM(_mem(None).gnn, edge_selectors=TemporalBackedge([1]), aux_edge_selectors=LearnedEdge(4), graph_size=8)
    with pytest.raises(NotImplementedError, match="LearnedEdge"):
        aux.rollout(obs, reset=reset)


def test_no_cpu_fallback():
    from gcm import _hip
    from gcm.edge_selectors.temporal import TemporalBackedge
    mem = _mem(TemporalBackedge([1]))
    hidden = mem.get_initial_hidden_state(torch.zeros(3, 4))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        mem.reset_hidden(hidden, torch.tensor([True, False, True]))


# ---- the C ABI --------------------------------------------------------------------------------------
def test_library_exports_every_symbol_of_the_reset_header():
    """include/gcm_hip_reset.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_reset.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_reset.h")))
    assert declared == set(_hip.RESET_PROTOTYPES) == {"gcm_state_reset", "gcm_episode_start",
                                                      "gcm_dense_rollout_tp_reset_fwd"}
    assert not declared & set(_hip.PROTOTYPES)
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == _hip.RESET_PROTOTYPES[name][1]
    # the reset forward takes gcm_dense_rollout_tp_fwd's arguments plus `start`
    assert len(_hip.RESET_PROTOTYPES["gcm_dense_rollout_tp_reset_fwd"][1]) == \
        len(_hip.PROTOTYPES["gcm_dense_rollout_tp_fwd"][1]) + 1


def test_c_abi_rejects_null_pointers_and_long_rollouts():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_state_reset(*([None] * 9), 1, 1, 1, None) == -1
    assert lib.gcm_episode_start(None, None, 1, 1, None) == -1
    assert lib.gcm_dense_rollout_tp_reset_fwd(*([None] * 2), None, 0, None, 0, 0, 0, *([None] * 7), 0, 0, None, None,
                                              1, 1, 8, 1, 32, 32, 32, None) == -1
