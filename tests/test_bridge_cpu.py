"""gcm.gcm.DenseToSparse / SparseToDense without a GPU: the import path of the reference, the torch path of both modules
against the restatement (tests/_bridge_restate.py), the restatement against a plain loop, the two additions to
gcm.nn.Sequential the reference's own GNN needs, and the C ABI section (include/gcm_hip_bridge.h)."""
import pytest
import torch

import _bridge_restate as R


def test_import_path_of_the_reference():
    from gcm.gcm import DenseGCM, DenseToSparse, SparseToDense      # noqa: F401  (tests/test_gcm.py:11 of the reference)
    assert issubclass(DenseToSparse, torch.nn.Module) and issubclass(SparseToDense, torch.nn.Module)
    assert not list(DenseToSparse().parameters()) and not list(SparseToDense().parameters())
    assert "transpose=True" in repr(DenseToSparse(transpose=True))


def _x(B, N, F=3):
    return torch.arange(B * N * F, dtype=torch.float32).view(B, N, F) / 7


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("B,N", R.SHAPES)
def test_dense_to_sparse_torch_path(B, N, transpose):
    from gcm.gcm import DenseToSparse
    x = _x(B, N)
    for kind in R.PATTERNS:
        adj = R.pattern(kind, B, N)
        want = R.dense_to_sparse(x, adj, transpose, edge_values=True)
        got = DenseToSparse(transpose=transpose, edge_values=True)(x, adj)
        assert len(got) == 4
        for g, w in zip(got, want):
            assert g.shape == w.shape and torch.equal(g, w.to(g.dtype)), kind
        assert got[1].dtype == got[2].dtype == torch.int64 and got[3].dtype == torch.float32
        assert got[0].data_ptr() == x.data_ptr()                         # a view
        three = DenseToSparse(transpose=transpose)(x, adj)
        assert len(three) == 3 and torch.equal(three[1], want[1])
        # the orientation: row -> column by default (the reference), column -> row transposed, same list order
        b, r, c = torch.nonzero(adj > 0).t()
        assert torch.equal(got[1][1 if transpose else 0], b * N + r)
        assert torch.equal(got[1][0 if transpose else 1], b * N + c)


def test_dense_to_sparse_values_carry_the_gradient_of_adj():
    from gcm.gcm import DenseToSparse
    adj = R.pattern("values", 3, 5).requires_grad_(True)
    *_, w = DenseToSparse(edge_values=True)(_x(3, 5), adj)
    g = torch.arange(1, w.numel() + 1, dtype=torch.float32)
    (w * g).sum().backward()
    want = torch.zeros(3, 5, 5)
    want[adj.detach() > 0] = g                                          # (b, r, c) order on both sides
    assert torch.equal(adj.grad, want)


def test_mask_raises_as_in_the_reference():
    from gcm.gcm import DenseToSparse
    with pytest.raises(NotImplementedError):
        DenseToSparse()(_x(2, 3), torch.ones(2, 3, 3), mask=torch.ones(2, 3, dtype=torch.bool))


def _ragged(seed=0):
    """Graphs of 4, 0, 7 and 2 nodes (B = 4) with duplicates, loops and an edge between two graphs."""
    gen = torch.Generator().manual_seed(seed)
    sizes = [4, 0, 7, 2]
    batch = torch.cat([torch.full((n,), b) for b, n in enumerate(sizes)])
    first = [0, 4, 4, 11]
    ei = []
    for b, n in enumerate(sizes):
        if n:
            ei.append(torch.randint(0, n, (2, 3 * n), generator=gen) + first[b])
    ei = torch.cat(ei + [torch.tensor([[0, 0, 5, 5], [1, 1, 5, 12]])], dim=1)   # 0->1 twice, a loop, graph 2 -> 3
    ei = ei[:, torch.randperm(ei.shape[1], generator=gen)]
    return batch, ei, torch.randn(13, 5, generator=gen)


def test_restatement_agrees_with_the_plain_loop():
    batch, ei, _ = _ragged()
    w = torch.randn(ei.shape[1], dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    for N in (3, 7, 9):
        for weight in (None, w):
            _, adj = R.sparse_to_dense(torch.zeros(13, 1), ei, batch, 4, N, weight)
            loop = R.dense_adj_loop(ei, batch, 4, N, weight)
            assert torch.allclose(adj.double(), loop, rtol=0, atol=1e-12)
    _, adj = R.sparse_to_dense(torch.zeros(13, 1), ei, batch, 4, 7)
    assert adj[0, 0, 1] == 2 and adj[2, 1, 1] >= 1                      # the duplicate added, the loop kept
    assert adj.sum() == ei.shape[1] - 1                                 # only the edge between two graphs is gone


@pytest.mark.parametrize("N", [3, 7, 9])
@pytest.mark.parametrize("weighted", [False, True])
def test_sparse_to_dense_torch_path(N, weighted):
    from gcm.gcm import SparseToDense
    batch, ei, x = _ragged(1)
    gen = torch.Generator().manual_seed(3)
    w = torch.randint(-4, 5, (ei.shape[1],), generator=gen).float() / 4 if weighted else None   # (exact sums)
    got_x, got_adj = SparseToDense()(x, ei, batch, 4, N, w)
    want_x, want_adj = R.sparse_to_dense(x, ei, batch, 4, N, w)
    assert got_x.shape == (4, N, 5) and got_adj.shape == (4, N, N) and got_adj.dtype == torch.float32
    assert torch.equal(got_x, want_x) and torch.equal(got_adj, want_adj)
    assert torch.equal(got_x[1], torch.zeros(N, 5))                     # the graph without nodes


def test_round_trip_torch_path():
    from gcm.gcm import DenseToSparse, SparseToDense
    for B, N in R.SHAPES[:5]:
        x = _x(B, N)
        for kind in R.PATTERNS:
            adj = R.pattern(kind, B, N)
            for transpose in (False, True):
                x_d, adj_d = SparseToDense()(*DenseToSparse(transpose=transpose)(x, adj), B, N)
                want = (adj > 0).float()
                assert torch.equal(x_d, x) and torch.equal(adj_d, want.transpose(1, 2) if transpose else want)


# ---- gcm.nn.Sequential -----------------------------------------------------------------------------------------
def test_sequential_takes_a_plain_callable_stage():
    from gcm import nn as G
    lin = torch.nn.Linear(3, 3)
    seq = G.Sequential("x, adj", [(lin, "x -> x"), (lambda x: 2 * x, "x -> y"), torch.nn.Tanh()])
    assert list(seq.state_dict()) == ["module_0.weight", "module_0.bias"]       # numbering and keys as before
    assert [n for n, _ in seq.named_children()] == ["module_0", "module_2"]
    x = torch.randn(4, 3)
    assert torch.equal(seq(x, None), torch.tanh(2 * lin(x)))
    assert len(seq.stages()) == 3 and seq.stages()[1][1:] == (["x"], ["y"])
    with pytest.raises(TypeError):
        G.Sequential("x", [(3, "x -> x")])


def test_sequential_ignores_the_empty_name_of_a_trailing_comma():
    from gcm import nn as G
    seq = G.Sequential("x, adj,", [(lambda x, adj: (x + 1, adj), "x, adj, -> x, adj,"), (lambda x: x, "x -> x")])
    assert seq.arg_names == ["x", "adj"] and seq.stages()[0][1:] == (["x", "adj"], ["x", "adj"])
    assert torch.equal(seq(torch.zeros(2), torch.ones(2)), torch.ones(2))


def test_the_reference_gnn_builds_and_runs():
    """tests/test_gcm.py:448-460 of the reference, verbatim but for the module names."""
    from gcm import nn as G
    from gcm.gcm import DenseToSparse, SparseToDense

    class Conv(torch.nn.Module):            # (a stand-in on the CPU: gcm.nn.GCNConv is a HIP kernel)
        def __init__(self, cin, cout):
            super().__init__()
            self.lin = torch.nn.Linear(cin, cout)

        def forward(self, x, edge_index):
            return self.lin(x).index_add(0, edge_index[1], x[edge_index[0]])

    feats, batches, N = 11, 5, 10
    g = G.Sequential(
        "x, adj, weights, B, N",
        [
            (DenseToSparse(), "x, adj, -> x_sp, edge_index, batch_idx"),
            (Conv(feats, feats), "x_sp, edge_index -> x_sp"),
            (torch.nn.ReLU()),
            (Conv(feats, feats), "x_sp, edge_index -> x_sp"),
            (torch.nn.ReLU()),
            (SparseToDense(), "x_sp, edge_index, batch_idx, B, N -> x, adj"),
            # Return only x not adj
            (lambda x: x, "x -> x"),
        ],
    )
    assert sorted(g.state_dict()) == ["module_1.lin.bias", "module_1.lin.weight", "module_3.lin.bias",
                                      "module_3.lin.weight"]
    nodes = torch.arange(batches * N * feats, dtype=torch.float).reshape(batches, N, feats)
    adj = torch.zeros(batches, N, N, dtype=torch.long)
    adj[:, 0:2, 3:4] = 1
    out = g(nodes, adj, torch.ones(batches, N, N), batches, N)
    assert out.shape == (batches, N, feats) and out.requires_grad


# ---- the C ABI -------------------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_bridge_image", "gcm_bridge_scan", "gcm_bridge_fill", "gcm_bridge_values_bwd",
              "gcm_bridge_dense_nodes", "gcm_bridge_dense_nodes_bwd", "gcm_bridge_dense_adj",
              "gcm_bridge_dense_adj_bwd"}


def test_library_exports_every_symbol_of_the_bridge_header():
    """include/gcm_hip_bridge.h is a section gcm_hip.h includes: declared == bound == exported, disjoint from the rest."""
    import os
    import re
    from gcm import _abi, _hip, _ops
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_bridge.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_bridge.h")))
    assert declared == set(_hip.BRIDGE_PROTOTYPES) == _FUNCTIONS
    for key, section in vars(_hip).items():
        if key.endswith("PROTOTYPES") and key != "BRIDGE_PROTOTYPES":
            assert not declared & set(section)
    lib = _hip.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, fn.argtypes) == _hip.BRIDGE_PROTOTYPES[name]
    assert lib.gcm_abi_version() == 8                                   # the section is additive
    assert _hip.BRIDGE_MAX_N == _ops.BRIDGE_MAX_N == 512


def test_c_abi_rejects_null_pointers_and_sizes_beyond_the_bound():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_bridge_image(None, 0, None, None, None, None, 1, 1, None) == -1
    assert lib.gcm_bridge_scan(None, None, 1, None) == -1
    assert lib.gcm_bridge_fill(None, 0, None, None, None, None, None, None, None, None, None, None, None, 1, 1, 0,
                               0, None) == -1
    assert lib.gcm_bridge_values_bwd(None, None, None, 1, 1, 0, 0, None) == -1
    assert lib.gcm_bridge_dense_nodes(None, None, None, 1, 1, 1, 1, None) == -1
    assert lib.gcm_bridge_dense_nodes_bwd(None, None, None, None, 1, 1, 1, 1, None) == -1
    assert lib.gcm_bridge_dense_adj(None, None, None, None, None, None, None, 1, 1, 1, 1, None) == -1
    assert lib.gcm_bridge_dense_adj_bwd(None, None, None, None, None, 1, 1, 1, 1, None) == -1
    # checked before anything is launched: N beyond the bound is unsupported, not an error of the arguments
    import ctypes
    word = ctypes.c_int64(0)
    p = ctypes.addressof(word)
    assert lib.gcm_bridge_image(p, 0, p, p, p, p, 1, _hip.BRIDGE_MAX_N + 1, None) == _hip.GCM_EUNSUPPORTED
    assert lib.gcm_bridge_fill(None, 0, p, p, p, p, None, p, p, None, None, None, None, 1, _hip.BRIDGE_MAX_N + 1, 0,
                               0, None) == _hip.GCM_EUNSUPPORTED
    # nothing to do: nothing is launched and empty tensors may come as NULL
    assert lib.gcm_bridge_dense_nodes_bwd(None, None, None, None, 0, 1, 1, 1, None) == 0
    assert lib.gcm_bridge_dense_adj_bwd(None, None, None, None, None, 0, 0, 1, 1, None) == 0


def test_the_capture_branch_raises_before_any_launch():
    """The host read of E cannot run inside a stream capture.  No test starts a capture to see the error: the branch
    is read here - it sits before the first kernel call of the function and names the reason."""
    import inspect
    from gcm import _ops
    src = inspect.getsource(_ops.dense_to_sparse)
    guard, first_call = src.index("is_current_stream_capturing()"), src.index("_call(")
    assert guard < first_call
    assert "raise RuntimeError" in src[guard:first_call] and "stream capture" in src[guard:first_call]
