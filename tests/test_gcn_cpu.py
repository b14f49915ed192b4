"""DenseGCNConv / GCNConv host side: parameters, argument checks, the C ABI's validation and the
restatement the GPU tests compare against, pinned by hand-computed answers.  No kernel runs."""
import math

import pytest
import torch

from _gcn_restate import dense_gcn, gcn


def test_state_dict_layout_and_interchange():
    from gcm import nn as G
    d, s = G.DenseGCNConv(3, 5), G.GCNConv(3, 5)
    for m in (d, s):
        sd = m.state_dict()
        assert set(sd) == {"lin.weight", "bias"}
        assert sd["lin.weight"].shape == (5, 3) and sd["bias"].shape == (5,)
        assert torch.count_nonzero(sd["bias"]) == 0
        bound = math.sqrt(6.0 / (3 + 5))          # glorot
        assert float(sd["lin.weight"].abs().max()) <= bound
    s.load_state_dict(d.state_dict())
    assert torch.equal(s.lin.weight, d.lin.weight)
    d.load_state_dict(G.GCNConv(3, 5).state_dict())
    assert set(G.DenseGCNConv(3, 5, bias=False).state_dict()) == {"lin.weight"}


def test_not_graphconv_subclasses():
    from gcm import nn as G
    assert not isinstance(G.DenseGCNConv(2, 2), (G.DenseGraphConv, G.GraphConv))
    assert not isinstance(G.GCNConv(2, 2), (G.DenseGraphConv, G.GraphConv))


def test_argument_errors():
    from gcm import nn as G, _hip
    with pytest.raises(NotImplementedError):
        G.GCNConv(2, 2, cached=True)
    conv = G.GCNConv(2, 2)
    ei = torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="edge_weight"):
        conv(torch.zeros(3, 2), ei, torch.ones(3))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        G.DenseGCNConv(2, 2)(torch.zeros(1, 3, 2), torch.zeros(1, 3, 3))
    with pytest.raises(TypeError):
        G.DenseGCNConv(2, 2)(torch.zeros(1, 3, 2), torch.zeros(1, 3, 3, dtype=torch.float64))


def test_c_abi_rejects_null_pointers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_gcnconv_fwd(*([None] * 9), 1, 1, 1, 1, 1, 1.0, None) == -1
    assert lib.gcm_dense_gcnconv_bwd(*([None] * 13), 0, 1, 1, 1, 1, 1, 1.0, None) == -1
    assert lib.gcm_gcn_norm(*([None] * 9), 1, 0, 1, 1, 1.0, None) == -1
    assert lib.gcm_csr_gcnconv_fwd(*([None] * 9), 1, 0, 1, 1, None) == -1
    assert lib.gcm_csr_gcnconv_bwd(*([None] * 21), 0, 1, 0, 1, 1, 1, 1, None) == -1
    assert lib.gcm_dense_gcnconv_bwd_workspace_bytes(256, 128, 32, 32) > 0
    assert lib.gcm_csr_gcnconv_bwd_workspace_bytes(1000, 900, 32, 32) > 0
    assert lib.gcm_dense_gcnconv_bwd_workspace_bytes(0, 128, 32, 32) == 0


# ---- the restatement against hand-computed answers (identity weight, no bias) ----------------
def _eye(n):
    return torch.eye(n, dtype=torch.float64)


def test_restatement_path():
    # 0 -> 1 -> 2 with self-loops: deg = [1, 2, 2]
    x = torch.tensor([[1.0], [2.0], [4.0]], dtype=torch.float64)
    out = gcn(x, torch.tensor([[0, 1], [1, 2]]), _eye(1))
    want = [1.0, 1 / math.sqrt(2) + 2 / 2, 2 / 2 + 4 / 2]
    assert torch.allclose(out.flatten(), torch.tensor(want, dtype=torch.float64))
    adj = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=torch.float64)
    assert torch.allclose(dense_gcn(x, adj, _eye(1))[0], out)


def test_restatement_no_edges():
    x = torch.randn(4, 3, dtype=torch.float64)
    W, b = torch.randn(2, 3, dtype=torch.float64), torch.randn(2, dtype=torch.float64)
    out = gcn(x, torch.zeros(2, 0, dtype=torch.long), W, b)
    assert torch.allclose(out, x @ W.t() + b)


def test_restatement_existing_weighted_loop():
    # node 1 has loops of weight 3 then 5 (the last wins) and an in-edge 0 -> 1 of weight 2
    x = torch.tensor([[1.0], [10.0]], dtype=torch.float64)
    ei = torch.tensor([[1, 0, 1], [1, 1, 1]])
    w = torch.tensor([3.0, 2.0, 5.0], dtype=torch.float64, requires_grad=True)
    out = gcn(x, ei, _eye(1), edge_weight=w)
    # deg = [1, 2 + 5]; out1 = 2 / sqrt(7) * 1 + 5 / 7 * 10
    assert torch.allclose(out.flatten(), torch.tensor([1.0, 2 / math.sqrt(7) + 50 / 7], dtype=torch.float64))
    out[1].sum().backward()
    assert w.grad[0] == 0 and w.grad[2] != 0


def test_restatement_isolated_without_loops():
    x = torch.tensor([[1.0], [2.0], [3.0]], dtype=torch.float64)
    out = gcn(x, torch.tensor([[0], [1]]), _eye(1), add_self_loops=False)
    # deg = [0, 1, 0]: dinv[0] = 0 (inf -> 0), so even the message 0 -> 1 vanishes
    assert torch.equal(out.flatten(), torch.zeros(3, dtype=torch.float64))
    out = gcn(x, torch.tensor([[0], [1]]), _eye(1), normalize=False)
    assert torch.equal(out.flatten(), torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))


def test_restatement_dense_overwrites_diagonal():
    x = torch.tensor([[1.0], [3.0]], dtype=torch.float64)
    adj = torch.tensor([[7.0, 0.0], [1.0, 5.0]], dtype=torch.float64)
    out = dense_gcn(x, adj, _eye(1))[0].flatten()
    # A = [[1, 0], [1, 1]]: deg = [1, 2];  improved: A = [[2, 0], [1, 2]], deg = [2, 3]
    assert torch.allclose(out, torch.tensor([1.0, 1 / math.sqrt(2) + 3 / 2], dtype=torch.float64))
    out2 = dense_gcn(x, adj, _eye(1), improved=True)[0].flatten()
    assert torch.allclose(out2, torch.tensor([1.0, 1 / math.sqrt(6) + 2.0], dtype=torch.float64))
