"""The algebra of the GEMM-form cached backward (csrc/rows_bptt_hops.hip), pinned without a GPU: its float64
restatement (tests/_bptt_hops_restate.py) against autograd through the oracle's rollout, on the cases the GPU tests use."""
import copy
import os
import re

import pytest
import torch

from oracle import dense as od
from oracle import pyg
import _bptt_hops_restate as R


def _gnn(F, H1, H2):
    return pyg.Sequential("x, adj, weights, B, N", [
        (pyg.DenseGraphConv(F, H1), "x, adj -> x"), torch.nn.Tanh(),
        (pyg.DenseGraphConv(H1, H2), "x, adj -> x"), torch.nn.Tanh()])


@pytest.mark.parametrize("part", ["all", "third", "last"])
@pytest.mark.parametrize("H2", [16, 32])
@pytest.mark.parametrize("hops,N,T", R.CASES)
def test_restatement_matches_autograd(hops, N, T, H2, part):
    """Closed-form forward and the formulas' gradient against the oracle in float64: T < N and T = N, self loop with and
    without, a duplicate hop, a chain shorter than its largest hop, a loss on all / every third / the last belief."""
    B, F, H1 = 3, 32, 32
    torch.manual_seed(N + T + H2)
    ref = _gnn(F, H1, H2).double()
    assert {k for k, _ in ref.named_parameters()} == set(R.PARAM_KEYS)
    obs = torch.rand(T, B, F, dtype=torch.float64)
    w = torch.rand(T, B, H2, dtype=torch.float64)
    steps = {"all": list(range(T)), "third": list(range(0, T, 3)), "last": [T - 1]}[part]
    out, hid = od.dense_rollout(obs, None, ref, graph_size=N, edge_selectors=od.TemporalBackedge(hops, "forward"))
    sum((out[t] * w[t]).sum() for t in steps).backward()
    params = {k: p.detach() for k, p in ref.named_parameters()}
    cX, cA, cH, v, mx = R.forward_empty(obs, params, hops)
    assert float((mx - out.detach()).abs().max()) < 1e-13
    assert torch.equal(cX, hid[0][:, :T])
    got = R.backward(mx[steps], v[steps], w[steps], steps, cH, cA, cX, params[R.PARAM_KEYS[3]], params[R.PARAM_KEYS[4]],
                     hops)
    for k, p in ref.named_parameters():
        assert float((got[k] - p.grad).abs().max()) <= 1e-12 * max(1.0, float(p.grad.abs().max())), k


def test_library_exports_every_symbol_of_the_bptt_hops_header():
    """include/gcm_hip_bptt_hops.h is a section gcm_hip.h includes: every function it declares is exported and bound."""
    from gcm import _abi, _hip
    inc = _abi.INCLUDE
    assert '#include "gcm_hip_bptt_hops.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_bptt_hops.h")))
    assert declared == {"gcm_dense_rows_bptt_cached_hops"} == set(_hip.BPTT_HOPS_PROTOTYPES)
    lib = _hip.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == _hip.BPTT_HOPS_PROTOTYPES[name][1]


def test_debug_library_still_loads():
    """libgcm_hip_debug.so (bench.py's launch floor and event cross-checks, tools/gcm_debuglib.py) is linked from a hand-kept
    object list: every symbol it needs must be inside it (ctypes resolves all of them at load)."""
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    sys.path.insert(0, tools)
    try:
        import gcm_debuglib
        assert gcm_debuglib.lib() is not None
    finally:
        sys.path.remove(tools)
