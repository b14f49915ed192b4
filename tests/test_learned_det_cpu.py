"""LearnedEdge(deterministic=True) host side: the restatement the GPU tests compare against (tests/_learned_det_restate.py)
pinned to util.Spardmax on the reference-shaped matrix and to the closed-form gradient, the C ABI section, and the
no-CPU-fallback rule.  No kernel runs."""
import pytest
import torch

from _learned_det_restate import LearnedEdgeDet, closed_form_grad, sparsemax_select
from oracle import dense as od


def _case(seed=0, dtype=torch.float64):
    torch.manual_seed(seed)
    B, N = 3, 7
    num_nodes = torch.tensor([0, 1, 5])
    logits = (3 * torch.randn(B, N, dtype=dtype)).requires_grad_(True)
    adj = torch.zeros(B, N, N, dtype=dtype)
    adj[2, 5, 1], adj[2, 5, 3], adj[2, 2, 0] = 1.0, 0.5, 1.0
    adj.requires_grad_(True)
    g_adj = torch.randn(B, N, N, dtype=dtype)
    return B, N, num_nodes, logits, adj, g_adj


def _reference_shaped(logits, adj, num_nodes):
    """learned.py:78-111 as written: the [B, max n] matrix filled with -1e10, util.Spardmax, the STE'd index_put."""
    from gcm import util
    B, N = logits.shape
    past = torch.nonzero(torch.arange(N)[None, :] < num_nodes[:, None])
    b_idx, j_idx = past[:, 0], past[:, 1]
    i_idx = num_nodes[b_idx]
    shaped = torch.full((B, int(num_nodes.max())), -1e10, dtype=logits.dtype)
    shaped = shaped.index_put((b_idx, j_idx), logits[b_idx, j_idx])
    edges = util.Spardmax()(shaped)
    assert edges.dtype == logits.dtype
    return adj.clone().index_put((b_idx, i_idx, j_idx), od._STE.apply(edges[b_idx, j_idx] + adj[b_idx, i_idx, j_idx]))


def test_restatement_equals_spardmax_on_the_reference_shaped_matrix():
    B, N, num_nodes, logits, adj, g_adj = _case()
    new_adj, soft, margin = sparsemax_select(logits, adj, num_nodes)
    new_adj.backward(g_adj)
    new_adj, soft = new_adj.detach(), soft.detach()
    got = (new_adj, logits.grad.clone(), adj.grad.clone())
    logits.grad = adj.grad = None
    want = _reference_shaped(logits, adj, num_nodes)
    want.backward(g_adj)
    assert torch.equal(got[0], want.detach())
    torch.testing.assert_close(got[1], logits.grad, rtol=0, atol=1e-15)
    assert torch.equal(got[2], adj.grad)
    # n = 0 and n = 1: nothing / the single candidate; the rewrite keeps 1, lifts 0.5 to 1, touches row cur only
    assert torch.equal(new_adj[0], adj[0].detach()) and float(soft[0].abs().sum()) == 0
    assert float(soft[1, 0]) == 1.0 and float(new_adj[1, 1, 0]) == 1.0
    assert float(new_adj[2, 5, 1]) == 1.0 and float(new_adj[2, 5, 3]) == 1.0 and float(new_adj[2, 2, 0]) == 1.0
    assert set(new_adj.unique().tolist()) <= {0.0, 1.0}
    torch.testing.assert_close(soft.sum(-1), torch.tensor([0.0, 1.0, 1.0], dtype=soft.dtype))
    assert float(soft[:, 5:].abs().sum()) == 0 and margin > 0


def test_restatement_gradient_is_the_closed_form():
    for seed in range(4):
        B, N, num_nodes, logits, adj, g_adj = _case(seed)
        new_adj, soft, _ = sparsemax_select(logits, adj, num_nodes)
        new_adj.backward(g_adj)
        want = closed_form_grad(soft.detach(), g_adj, num_nodes)
        torch.testing.assert_close(logits.grad, want, rtol=0, atol=1e-15)
        assert float(logits.grad[0].abs().sum()) == 0                 # n = 0
        assert float(logits.grad[1].abs().sum()) == 0                 # n = 1: |S| = 1, g - mean(g) = 0
        assert torch.equal(adj.grad, g_adj)                           # both STEs are identities


def test_restatement_selector_runs_in_the_oracle_step():
    torch.manual_seed(1)
    B, N, F, H, T = 3, 8, 4, 8, 11
    gnn = od.canonical_gnn(F, H).double()
    sel = LearnedEdgeDet(od.build_edge_network(F).double())
    obs = torch.rand(T, B, F, dtype=torch.float64)
    out, hid = od.dense_rollout(obs, None, gnn, graph_size=N, edge_selectors=sel)
    out.mean().backward()
    adj = hid[1].detach()
    assert set(adj.unique().tolist()) <= {0.0, 1.0} and float(adj.triu().sum()) == 0
    assert bool((adj[:, N - 1].sum(-1) >= 1).all())                   # the last row written: the support is never empty
    assert 0 < sel.margin < float("inf")
    assert all(p.grad is not None for p in sel.net.parameters())


def test_library_exports_every_symbol_of_the_learned_det_header():
    """include/gcm_hip_learned_det.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    import os
    import re
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_learned_det.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_learned_det.h")))
    assert declared == set(_hip.LEARNED_DET_PROTOTYPES) == {"gcm_learned_sparsemax_fwd", "gcm_learned_sparsemax_bwd"}
    assert not declared & set(_hip.PROTOTYPES) and not declared & set(_hip.AGGR_PROTOTYPES)
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert fn.argtypes == _hip.LEARNED_DET_PROTOTYPES[name][1]


def test_c_abi_rejects_null_pointers_and_wide_graphs():
    from gcm import _hip
    lib = _hip.lib()
    one = 8        # a non-null address; validation returns before any launch
    assert lib.gcm_learned_sparsemax_fwd(None, one, one, one, 1, 4, None) != 0
    assert lib.gcm_learned_sparsemax_bwd(one, None, one, one, 1, 4, None) != 0
    assert lib.gcm_learned_sparsemax_fwd(one, one, one, one, 0, 4, None) != 0
    assert lib.gcm_learned_sparsemax_fwd(one, one, one, one, 1, 1025, None) == _hip.GCM_EUNSUPPORTED
    assert lib.gcm_learned_sparsemax_bwd(one, one, one, one, 1, 1025, None) == _hip.GCM_EUNSUPPORTED


@pytest.mark.parametrize("custom", [False, True])
def test_deterministic_selector_has_no_cpu_fallback(custom):
    from gcm import _hip
    from gcm.edge_selectors.learned import LearnedEdge
    F, B, N = 4, 2, 6
    model = torch.nn.Sequential(torch.nn.Linear(2 * F, 6), torch.nn.Tanh(), torch.nn.Linear(6, 1)) if custom else None
    sel = LearnedEdge(F, model=model, deterministic=True)
    assert sel.deterministic and sel.noise_fn is None
    with pytest.raises(_hip.HipLibraryError):
        sel(torch.randn(B, N, F), torch.zeros(B, N, N), torch.zeros(0), torch.tensor([1, 3]), B)
