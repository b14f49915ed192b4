"""DenseGATConv / GATConv host side: parameters, argument checks, the C ABI's validation and the
restatement the GPU tests compare against, pinned by hand-computed answers.  No kernel runs."""
import math

import pytest
import torch

from _gat_restate import dense_gat, gat


@pytest.mark.parametrize("concat", [True, False])
def test_parameters(concat):
    from gcm import nn as G
    F, C, H = 6, 5, 3
    d = G.DenseGATConv(F, C, heads=H, concat=concat)
    s = G.GATConv(F, C, heads=H, concat=concat)
    nb = H * C if concat else C
    for m, att in ((d, (1, 1, H, C)), (s, (1, H, C))):
        sd = m.state_dict()
        assert set(sd) == {"lin.weight", "att_src", "att_dst", "bias"}
        assert sd["lin.weight"].shape == (H * C, F)
        assert sd["att_src"].shape == att and sd["att_dst"].shape == att
        assert sd["bias"].shape == (nb,) and torch.count_nonzero(sd["bias"]) == 0
        assert float(sd["lin.weight"].abs().max()) <= math.sqrt(6.0 / (H * C + F))
        for k in ("att_src", "att_dst"):
            assert 0 < float(sd[k].abs().max()) <= math.sqrt(6.0 / (H + C))
    assert set(G.DenseGATConv(F, C, bias=False).state_dict()) == {"lin.weight", "att_src", "att_dst"}
    assert not isinstance(d, (G.DenseGraphConv, G.GraphConv)) and not isinstance(s, (G.DenseGraphConv, G.GraphConv))


def test_argument_errors():
    from gcm import nn as G, _hip
    x, ei = torch.zeros(3, 2), torch.tensor([[0, 1], [1, 2]])
    for conv, args in ((G.GATConv(2, 2, dropout=0.5), (x, ei)),
                       (G.DenseGATConv(2, 2, dropout=0.5), (x, torch.ones(3, 3)))):
        with pytest.raises(NotImplementedError, match="dropout"):
            conv(*args)
        conv.eval()                                   # dropout is a no-op in eval mode: the call reaches the kernels
        with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
            conv(*args)
    with pytest.raises(NotImplementedError, match="edge_dim"):
        G.GATConv(2, 2, edge_dim=3)
    with pytest.raises(NotImplementedError, match="return_attention_weights"):
        G.GATConv(2, 2)(x, ei, return_attention_weights=True)
    with pytest.raises(NotImplementedError, match="GATv2"):
        G.GATv2Conv(2, 2)
    with pytest.raises(TypeError):
        G.DenseGATConv(2, 2)(torch.zeros(1, 3, 2), torch.zeros(1, 3, 3, dtype=torch.float64))


def test_c_abi_rejects_null_pointers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_dense_gatconv_fwd(*([None] * 14), 1, 1, 1, 1, 1, 1, 1, 0.2, None) == -1
    assert lib.gcm_dense_gatconv_bwd(*([None] * 17), 0, 1, 1, 1, 1, 1, 1, 0.2, None) == -1
    assert lib.gcm_csr_gatconv_fwd(*([None] * 14), 1, 0, 1, 1, 1, 1, 1, 0.2, None) == -1
    assert lib.gcm_csr_gatconv_bwd(*([None] * 21), 0, 1, 0, 1, 1, 1, 1, 1, 0.2, None) == -1
    assert lib.gcm_dense_gatconv_bwd_workspace_bytes(256, 128, 32, 4, 8, 1) > 0
    assert lib.gcm_csr_gatconv_bwd_workspace_bytes(1000, 900, 32, 2, 16, 0) > 0
    assert lib.gcm_dense_gatconv_bwd_workspace_bytes(0, 128, 32, 1, 32, 1) == 0


# ---- the restatement against hand-computed answers (identity weight) -------------------------
def _d(v):
    return torch.tensor(v, dtype=torch.float64)


def _softmax_sum(es, vs):
    w = [math.exp(e) for e in es]
    return sum(a * v for a, v in zip(w, vs)) / sum(w)


def _lrelu(v, s=0.2):
    return v if v > 0 else s * v


def test_restatement_two_heads():
    # heads 2, C = 1, W = I: y = x.  att_src = [1, 2], att_dst = [0.5, -1].  Edges 0 -> 2, 1 -> 2, plus loops.
    x = _d([[1.0, 0.0], [0.0, 1.0], [-1.0, 1.0]])
    W, a_s, a_d = torch.eye(2, dtype=torch.float64), _d([1.0, 2.0]), _d([0.5, -1.0])
    ei = torch.tensor([[0, 1], [2, 2]])
    out = gat(x, ei, W, a_s, a_d, heads=2)
    s_src = [[1.0, 0.0], [0.0, 2.0], [-1.0, 2.0]]       # [node][head]
    s_dst = [[0.5, 0.0], [0.0, -1.0], [-0.5, -1.0]]
    want = []
    for i, nbrs in ((0, [0]), (1, [1]), (2, [0, 1, 2])):
        want.append([_softmax_sum([_lrelu(s_dst[i][h] + s_src[j][h]) for j in nbrs], [x[j, h].item() for j in nbrs])
                     for h in range(2)])
    assert torch.allclose(out, _d(want))
    mean = gat(x, ei, W, a_s, a_d, heads=2, concat=False)
    assert torch.allclose(mean.flatten(), _d(want).mean(1))
    adj = _d([[0, 0, 0], [0, 0, 0], [1, 1, 0]])
    assert torch.allclose(dense_gat(x, adj, W, a_s, a_d, heads=2)[0], out)


def test_restatement_replaced_loop_and_duplicates():
    # node 1: a loop twice and 0 -> 1.  add_self_loops: the loops are replaced by one; without: three terms
    x = _d([[2.0], [-1.0]])
    W, a_s, a_d = torch.eye(1, dtype=torch.float64), _d([1.0]), _d([1.0])
    ei = torch.tensor([[1, 1, 0], [1, 1, 1]])
    e10, e11 = _lrelu(-1.0 + 2.0), _lrelu(-1.0 - 1.0)
    out = gat(x, ei, W, a_s, a_d)
    assert torch.allclose(out[1], _d([_softmax_sum([e10, e11], [2.0, -1.0])]))
    out = gat(x, ei, W, a_s, a_d, add_self_loops=False)
    assert torch.allclose(out[1], _d([_softmax_sum([e11, e11, e10], [-1.0, -1.0, 2.0])]))


def test_restatement_isolated_node_gives_bias():
    x = _d([[1.0], [2.0], [3.0]])
    W, a_s, a_d, b = torch.eye(1, dtype=torch.float64), _d([1.0]), _d([1.0]), _d([0.25])
    out = gat(x, torch.tensor([[0], [1]]), W, a_s, a_d, b, add_self_loops=False)
    assert torch.equal(out.flatten(), _d([0.25, 1.25, 0.25]))
    adj = _d([[0, 0, 0], [1, 0, 0], [0, 0, 0]])
    dense = dense_gat(x, adj, W, a_s, a_d, b, add_loop=False)[0]
    assert torch.equal(dense, out)
    assert not torch.isnan(dense).any()


def test_restatement_add_loop_overwrites_weighted_diagonal():
    x = _d([[1.0, -2.0], [3.0, 0.5], [0.0, 1.0]])
    W, a_s, a_d = _d([[1.0, 0.5], [-0.5, 1.0]]), _d([0.3, -0.7]), _d([1.1, 0.2])
    weighted = _d([[5.0, 0.0, 2.5], [0.1, 7.0, 0.0], [0.0, 3.0, 0.0]])
    pattern = _d([[1.0, 0.0, 1.0], [1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])
    got = dense_gat(x, weighted, W, a_s, a_d, heads=1)
    assert torch.allclose(got, dense_gat(x, pattern, W, a_s, a_d))
    # node 2 has a zero diagonal: with add_loop it attends to itself, without it only to node 1
    y = x @ W.t()
    s_src, s_dst = y @ a_s, y @ a_d
    e21, e22 = _lrelu(float(s_dst[2] + s_src[1])), _lrelu(float(s_dst[2] + s_src[2]))
    want = [_softmax_sum([e21, e22], [float(y[1, c]), float(y[2, c])]) for c in range(2)]
    assert torch.allclose(got[0, 2], _d(want))
    no_loop = dense_gat(x, weighted, W, a_s, a_d, add_loop=False)
    assert torch.allclose(no_loop[0, 2], y[1])
