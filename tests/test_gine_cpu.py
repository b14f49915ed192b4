"""GINEConv / DenseGINEConv / RelativeEdgeAttr host side: parameters, argument checks, the calling contract on
edge_attr, the C ABI's validation, the restatement the GPU tests compare against and the quantised inputs that keep
them off the ReLU's kink.  No kernel runs."""
import os
import re

import pytest
import torch

from _gin_restate import gin
from _gine_restate import (DENSE_CASES, SPARSE_CASES, DenseGINERef, GINERef, dense_case, dense_gine,
                           dense_rel_edge_attr, gine, min_abs_pre, quant_lin, rel_edge_attr, sparse_case)


def _mlp(cin=3, hid=5, cout=4):
    return torch.nn.Sequential(torch.nn.Linear(cin, hid), torch.nn.Tanh(), torch.nn.Linear(hid, cout))


def test_imports():
    from gcm import gine as GE, nn as G
    assert all(hasattr(GE, n) for n in ("GINEConv", "DenseGINEConv", "RelativeEdgeAttr"))
    assert hasattr(G, "GATv2Conv") and not hasattr(G, "GINEConv")             # the placeholder and gcm.nn's pin stay


# ---- parameters -----------------------------------------------------------------------------------
@pytest.mark.parametrize("train_eps", [False, True])
@pytest.mark.parametrize("edge_dim", [None, 2])
def test_parameters(train_eps, edge_dim):
    from gcm import gine as GE
    want = {"eps": (1,), "nn.0.weight": (5, 3), "nn.0.bias": (5,), "nn.2.weight": (4, 5), "nn.2.bias": (4,)}
    if edge_dim is not None:
        want.update({"lin.weight": (3, edge_dim), "lin.bias": (3,)})
    d = GE.DenseGINEConv(_mlp(), eps=0.25, train_eps=train_eps, edge_dim=edge_dim)
    s = GE.GINEConv(_mlp(), eps=0.25, train_eps=train_eps, edge_dim=edge_dim)
    for m in (d, s, DenseGINERef(_mlp(), 0.25, train_eps, edge_dim), GINERef(_mlp(), 0.25, train_eps, edge_dim)):
        assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
        assert m.initial_eps == 0.25 and float(m.eps.detach()) == 0.25 and m.eps.dtype == torch.float32
        assert isinstance(m.eps, torch.nn.Parameter) == train_eps
        assert ("eps" in dict(m.named_buffers())) == (not train_eps)
    s2 = GE.GINEConv(_mlp(), edge_dim=edge_dim)
    s2.load_state_dict(d.state_dict())
    for k, v in d.state_dict().items():
        assert torch.equal(s2.state_dict()[k], v)
    GINERef(_mlp(), edge_dim=edge_dim).load_state_dict(d.state_dict())
    assert repr(s) == f"GINEConv(nn={s.nn})" and repr(d) == f"DenseGINEConv(nn={d.nn})"


@pytest.mark.parametrize("cls", ["GINEConv", "DenseGINEConv"])
def test_in_channels_inference(cls):
    from gcm import gine as GE, nn as G
    C = getattr(GE, cls)
    assert C(torch.nn.Linear(7, 2), edge_dim=3).lin.weight.shape == (7, 3)
    assert C(_mlp(6), edge_dim=3).lin.weight.shape == (6, 3)
    assert C(G.GraphConv(9, 2), edge_dim=3).lin.weight.shape == (9, 3)        # in_channels, without in_features
    with pytest.raises(ValueError, match="Could not infer input channels from `nn`."):
        C(torch.nn.Tanh(), edge_dim=3)
    with pytest.raises(ValueError, match="Could not infer input channels"):
        C(torch.nn.Sequential(torch.nn.Tanh(), torch.nn.Linear(3, 3)), edge_dim=3)
    assert C(torch.nn.Tanh()).lin is None                                     # nothing to infer without edge_dim


@pytest.mark.parametrize("cls", ["GINEConv", "DenseGINEConv"])
@pytest.mark.parametrize("train_eps", [False, True])
def test_reset_parameters(cls, train_eps):
    from gcm import gine as GE
    conv = getattr(GE, cls)(_mlp(), eps=0.3, train_eps=train_eps, edge_dim=2)
    with torch.no_grad():
        conv.eps.fill_(7.0)
        for p in list(conv.nn.parameters()) + list(conv.lin.parameters()):
            p.fill_(9.0)
    conv.reset_parameters()
    assert float(conv.eps.detach()) == pytest.approx(0.3)
    for p in list(conv.nn.parameters()) + list(conv.lin.parameters()):
        assert float(p.detach().abs().max()) < 1.0            # torch.nn.Linear's init: within 1 / sqrt(fan_in)
    getattr(GE, cls)(_mlp()).reset_parameters()                # without lin


def test_relative_edge_attr_arguments():
    from gcm import gine as GE
    assert GE.RelativeEdgeAttr().out_channels == 1
    assert GE.RelativeEdgeAttr(pose_slice=slice(1, 4)).out_channels == 4
    assert GE.RelativeEdgeAttr(time=False, pose_slice=slice(1, 4)).out_channels == 3
    assert GE.RelativeEdgeAttr(time=False, pose_slice=slice(-2, None)).out_channels == 2
    assert GE.RelativeEdgeAttr(pose_slice=slice(None, 2), time_scale=0.25).out_channels == 3
    with pytest.raises(ValueError):
        GE.RelativeEdgeAttr(time=False)
    with pytest.raises(NotImplementedError, match="pose slices must be contiguous"):
        GE.RelativeEdgeAttr(pose_slice=slice(0, 4, 2))
    assert GE.RelativeEdgeAttr(time=False, pose_slice=slice(-3, -1))._range(8) == (5, 2)      # resolved against F
    assert GE.RelativeEdgeAttr(time=False, pose_slice=slice(-2, None))._range(8) == (6, 2)
    with pytest.raises(ValueError):
        GE.RelativeEdgeAttr(pose_slice=slice(1, 4))._range(3)                                 # x is too narrow


# ---- argument errors and the calling contract on edge_attr ------------------------------------------
def test_argument_errors():
    from gcm import gine as GE, nn as G, _hip
    x, ei = torch.zeros(3, 3), torch.tensor([[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="edge_attr"):
        GE.GINEConv(_mlp())(x, ei)
    with pytest.raises(ValueError, match="edge_attr"):
        GE.DenseGINEConv(_mlp())(x, torch.ones(3, 3))
    with pytest.raises(ValueError, match="Node and edge feature dimensionalities do not match. Consider setting the "
                                         "'edge_dim' attribute of 'GINEConv'"):
        GE.GINEConv(_mlp())(x, ei, torch.zeros(2, 2))
    with pytest.raises(ValueError, match="dimensionalities do not match"):
        GE.DenseGINEConv(_mlp())(x, torch.ones(3, 3), torch.zeros(3, 3, 2))
    # beyond the kernels' widths: refused before anything else
    with pytest.raises(ValueError, match="128"):
        GE.GINEConv(torch.nn.Identity())(torch.zeros(3, 129), ei, torch.zeros(2, 129))
    with pytest.raises(ValueError, match="32"):
        GE.GINEConv(_mlp(), edge_dim=33)(x, ei, torch.zeros(2, 33))
    with pytest.raises(ValueError, match="32"):
        GE.DenseGINEConv(_mlp(), edge_dim=33)(x, torch.ones(3, 3), torch.zeros(3, 3, 33))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        GE.GINEConv(_mlp(), edge_dim=2)(x, ei, torch.zeros(2, 2))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        GE.DenseGINEConv(_mlp(), edge_dim=2)(x, torch.ones(3, 3), torch.zeros(3, 3, 2))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        GE.RelativeEdgeAttr()(x, ei)
    with pytest.raises(NotImplementedError):                  # the pinned raises stay
        G.GATConv(3, 4, edge_dim=2)


def test_sparse_contract_on_edge_attr():
    from gcm import gine as GE, nn as G
    conv = GE.GINEConv(_mlp(), edge_dim=2)
    x, ei = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]])
    call = lambda ea, **kw: G._sparse_contract(conv, x, ei, 3, edge_attr=ea, edge_attr_width=2, device=False, **kw)
    with pytest.raises(TypeError, match="edge_attr must be float32"):
        call(torch.zeros(3, 2, dtype=torch.float64))
    for bad in (torch.zeros(3), torch.zeros(4, 2), torch.zeros(3, 5), torch.zeros(3, 2, 1)):
        with pytest.raises(ValueError, match="edge_attr"):
            call(bad)
    with pytest.raises(ValueError, match="my words"):
        call(torch.zeros(3, 5), edge_attr_error="my words")
    wide = torch.arange(24, dtype=torch.float32).view(3, 8)
    strided = wide[:, 1:3]                                    # strided, and starts at an odd element
    out = call(strided)
    assert len(out) == 5
    assert out[4].is_contiguous() and out[4].data_ptr() % 16 == 0 and torch.equal(out[4], strided)
    ready = torch.zeros(3, 2)
    assert call(ready)[4] is ready                            # what is ready already comes back itself
    # every existing layer ignores edge_attr exactly as before: no shape rule, four values
    gat = G.GATConv(3, 4)
    out = G._sparse_contract(gat, x, ei, 3, edge_attr=torch.zeros(7, 7, 7)[:, ::2], device=False)
    assert len(out) == 4
    with pytest.raises(TypeError):                            # (its dtype was checked before, and still is)
        G._sparse_contract(gat, x, ei, 3, edge_attr=torch.zeros(3, 2, dtype=torch.float64), device=False)


def test_dense_contract_on_edge_attr():
    from gcm import gine as GE, nn as G
    conv = GE.DenseGINEConv(_mlp(), edge_dim=2)
    x, adj = torch.zeros(2, 4, 3), torch.zeros(2, 4, 4)
    call = lambda ea, a=adj, xx=x: G._dense_contract(conv, xx, a, None, 3, edge_attr=ea, edge_attr_width=2,
                                                     device=False)
    with pytest.raises(TypeError, match="edge_attr must be float32"):
        call(torch.zeros(2, 4, 4, 2, dtype=torch.float64))
    for bad in (torch.zeros(2, 4, 4), torch.zeros(3, 4, 4, 2), torch.zeros(2, 4, 4, 3), torch.zeros(2, 4, 5, 2)):
        with pytest.raises(ValueError, match="edge_attr"):
            call(bad)
    for ea in (torch.zeros(4, 4, 2), torch.zeros(1, 4, 4, 2), torch.zeros(2, 4, 4, 2),
               torch.zeros(2, 4, 4, 4)[..., 1:3]):
        out = call(ea)
        assert len(out) == 3 and out[2].shape == (2, 4, 4, 2)
        assert out[2].is_contiguous() and out[2].data_ptr() % 16 == 0
    out = call(torch.zeros(4, 4, 2), torch.zeros(4, 4), torch.zeros(4, 3))     # 2-D operands: B = 1
    assert out[0].shape == (1, 4, 3) and out[2].shape == (1, 4, 4, 2)
    assert len(G._dense_contract(G.DenseGINConv(_mlp()), x, adj, device=False)) == 2


# ---- the restatement --------------------------------------------------------------------------------
_ID = torch.nn.Identity()


def _d(v):
    return torch.tensor(v, dtype=torch.float64)


def test_restatement_by_hand():
    # 0 -> 1 with e = [1, -5], 1 -> 1 with e = [0, 0]; eps = 0.5
    x = _d([[1.0, 2.0], [3.0, -1.0]])
    ei = torch.tensor([[0, 1], [1, 1]])
    ea = _d([[1.0, -5.0], [0.0, 0.0]])
    want = _d([[1.5, 3.0], [4.5 + 2.0 + 3.0, -1.5 + 0.0 + 0.0]])
    assert torch.equal(gine(x, ei, ea, 0.5, _ID), want)
    adj = _d([[0, 0], [1, 1]])
    dense_ea = torch.full((2, 2, 2), float("nan"), dtype=torch.float64)        # unset entries may hold anything
    dense_ea[1, 0], dense_ea[1, 1] = ea[0], ea[1]
    assert torch.equal(dense_gine(x, adj, dense_ea, 0.5, _ID)[0], want)
    assert torch.equal(dense_gine(x, 2 * adj, dense_ea, 0.5, _ID, add_loop=False)[0], _d([[0, 0], [10.0, 0.0]]))


def test_restatement_dense_equals_sparse():
    torch.manual_seed(1)
    B, N, F, D = 2, 9, 3, 2
    ref = DenseGINERef(_mlp(), eps=0.3, train_eps=True, edge_dim=D).double()
    sref = GINERef(_mlp(), train_eps=True, edge_dim=D).double()
    sref.load_state_dict(ref.state_dict())
    adj = (torch.rand(B, N, N) < 0.4).double()
    adj[:, 2] = 0
    x = torch.randn(B, N, F, dtype=torch.float64)
    ea = torch.randn(B, N, N, D, dtype=torch.float64)
    bb, ii, jj = adj.nonzero(as_tuple=True)
    ei = torch.stack([bb * N + jj, bb * N + ii])              # adj[b, i, j]: edge j -> i
    d = ref(x, adj, ea)
    s = sref(x.view(B * N, F), ei, ea[bb, ii, jj]).view(B, N, -1)
    assert float((d - s).detach().abs().max()) <= 1e-12


def test_restatement_identity_lin_and_gin():
    torch.manual_seed(2)
    M, E, F = 9, 30, 4
    x = torch.randn(M, F, dtype=torch.float64)
    ei = torch.randint(0, M, (2, E))
    ea = torch.randn(E, F, dtype=torch.float64)
    nn = _mlp(F).double()
    lin = torch.nn.Linear(F, F).double()
    with torch.no_grad():
        lin.weight.copy_(torch.eye(F))
        lin.bias.zero_()
    assert torch.equal(gine(x, ei, ea, 0.25, nn), gine(x, ei, ea, 0.25, nn, lin))
    xp = x.abs() + 0.1                                        # relu(x_j + 0) = x_j: GINConv
    assert torch.equal(gine(xp, ei, torch.zeros_like(ea), 0.25, nn), gin(xp, ei, 0.25, nn))


def test_restatement_relative_edge_attr():
    x = _d([[0.0, 1.0, 2.0], [0.5, 3.0, 5.0], [1.0, 7.0, 11.0]])
    ei = torch.tensor([[0, 2], [2, 1]])
    got = rel_edge_attr(x, ei, True, slice(1, 3), 0.25)
    assert torch.equal(got, _d([[0.5, -6.0, -9.0], [-0.25, 4.0, 6.0]]))
    dense = dense_rel_edge_attr(x.unsqueeze(0), True, slice(1, 3), 0.25)
    assert torch.equal(dense[0, 2, 0], got[0]) and torch.equal(dense[0, 1, 2], got[1])      # (b, sink, source)
    assert rel_edge_attr(x, ei, True, None).shape == (2, 1)
    assert torch.equal(rel_edge_attr(x, ei, False, slice(-2, None)), got[:, 1:])


# ---- the quantised inputs of the GPU tests: off the kink by construction ----------------------------
@pytest.mark.parametrize("case", SPARSE_CASES)
def test_quantised_sparse_cases_stay_off_the_kink(case):
    M, E, F, D = case
    x, ei, ea = sparse_case(*case)
    assert x.shape == (M, F) and ei.shape == (2, E)
    if D is None:
        e64, margin = ea, 1 / 16
        e32 = ea.float()
    else:
        lin = torch.nn.Linear(D, F).double()
        quant_lin(lin, torch.Generator().manual_seed(5))
        e64, margin = lin(ea).detach(), 1 / 32
        e32 = copy_to_float(lin)(ea.float()).detach()
    assert min_abs_pre(x, ei[0], e64) >= margin
    assert torch.equal((x.float()[ei[0]] + e32).double(), x[ei[0]] + e64)      # exact in fp32


def copy_to_float(lin):
    out = torch.nn.Linear(lin.in_features, lin.out_features)
    out.load_state_dict({k: v.float() for k, v in lin.state_dict().items()})
    return out


@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: "-".join(map(str, c[:4])))
def test_quantised_dense_cases_stay_off_the_kink(case):
    B, N, F, D, opts = case
    x, adj, ea, _ = dense_case(*case)
    x = x.unsqueeze(0) if x.dim() == 2 else x
    ea = ea.unsqueeze(0) if ea.dim() == 3 else ea
    lin = torch.nn.Linear(D, F).double()
    quant_lin(lin, torch.Generator().manual_seed(5))
    pre64 = x.unsqueeze(1) + lin(ea).detach()                 # every entry: what g_adj reads
    assert float(pre64.abs().min()) >= 1 / 32
    pre32 = x.float().unsqueeze(1) + copy_to_float(lin)(ea.float()).detach()
    assert torch.equal(pre32.double(), pre64)


# ---- the C ABI --------------------------------------------------------------------------------------
_FUNCTIONS = {"gcm_csr_gine_fwd", "gcm_csr_gine_bwd", "gcm_csr_gine_bwd_workspace_bytes",
              "gcm_dense_gine_fwd", "gcm_dense_gine_fwd_workspace_bytes", "gcm_dense_gine_bwd",
              "gcm_dense_gine_bwd_workspace_bytes", "gcm_rel_edge_attr_fwd", "gcm_rel_edge_attr_bwd",
              "gcm_dense_rel_edge_attr_fwd", "gcm_dense_rel_edge_attr_bwd"}


def test_library_exports_every_symbol_of_the_gine_header():
    from gcm import _abi, _hip
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    assert '#include "gcm_hip_gine.h"' in open(os.path.join(inc, "gcm_hip.h")).read()
    declared = set(re.findall(r"\b(gcm_[a-z0-9_]+)\s*\(", _abi.header("gcm_hip_gine.h")))
    assert declared == set(_hip.GINE_PROTOTYPES) == _FUNCTIONS
    others = [v for k, v in vars(_hip).items() if k.endswith("PROTOTYPES") and k != "GINE_PROTOTYPES"]
    assert len(others) >= 20 and not any(declared & set(o) for o in others)
    lib = _hip.lib()
    for name in declared:
        assert getattr(lib, name).argtypes == _hip.GINE_PROTOTYPES[name][1]
    assert lib.gcm_abi_version() == 8                         # the section is additive
    assert _hip.GINE_MAX_EDGE_DIM == 32


def test_c_abi_rejects_null_pointers_and_wide_layers():
    from gcm import _hip
    lib = _hip.lib()
    assert lib.gcm_csr_gine_fwd(*([None] * 9), 1, 0, 1, 1, None) == -1
    assert lib.gcm_csr_gine_bwd(*([None] * 18), 0, 1, 0, 1, 1, None) == -1
    assert lib.gcm_dense_gine_fwd(*([None] * 8), 0, 1, 1, 1, 1, 1, None) == -1
    assert lib.gcm_dense_gine_bwd(*([None] * 15), 0, 1, 1, 1, 1, 1, None) == -1
    assert lib.gcm_rel_edge_attr_fwd(None, None, None, 1, 1, 1, 0, 1, 1, 1.0, None) == -1
    assert lib.gcm_rel_edge_attr_bwd(*([None] * 6), 1, 1, 1, 0, 1, 1, None) == -1
    assert lib.gcm_dense_rel_edge_attr_fwd(None, None, 1, 1, 1, 0, 1, 1, 1.0, None) == -1
    assert lib.gcm_dense_rel_edge_attr_bwd(None, None, 1, 1, 1, 0, 1, 1, None) == -1
    # beyond the limits: GCM_EUNSUPPORTED before any launch (the pointers are never read: any non-null value)
    buf = torch.zeros(64)
    p = buf.data_ptr()
    assert lib.gcm_csr_gine_fwd(p, p, p, p, p, p, p, None, p, 1, 0, 129, 3, None) == _hip.GCM_EUNSUPPORTED
    assert lib.gcm_csr_gine_fwd(p, p, p, p, p, p, p, None, p, 1, 0, 8, 33, None) == _hip.GCM_EUNSUPPORTED
    assert lib.gcm_csr_gine_bwd(*([p] * 17), p, 1 << 20, 1, 0, 129, 3, None) == _hip.GCM_EUNSUPPORTED
    assert lib.gcm_csr_gine_bwd(*([p] * 17), p, 1 << 20, 1, 0, 8, 33, None) == _hip.GCM_EUNSUPPORTED
    assert lib.gcm_dense_gine_fwd(*([p] * 8), 1 << 20, 1, 1, 129, 3, 1, None) == _hip.GCM_EUNSUPPORTED
    assert lib.gcm_dense_gine_fwd(*([p] * 8), 1 << 20, 1, 1, 8, 33, 1, None) == _hip.GCM_EUNSUPPORTED
    assert lib.gcm_dense_gine_bwd(*([p] * 15), 1 << 20, 1, 1, 129, 3, 1, None) == _hip.GCM_EUNSUPPORTED
    assert lib.gcm_dense_gine_bwd(*([p] * 15), 1 << 20, 1, 1, 8, 33, 1, None) == _hip.GCM_EUNSUPPORTED


def test_workspace_does_not_grow_with_the_edges():
    from gcm import _hip
    lib = _hip.lib()
    M, F, D = 512 * 512, 32, 3
    few, many = (lib.gcm_csr_gine_bwd_workspace_bytes(M, E, F, D) for E in (M, 64 * M))
    assert 0 < few == many < M * F * 4                        # nothing of [E,F], less than one [M,F]
    assert lib.gcm_csr_gine_bwd_workspace_bytes(0, 0, F, D) == 0
    assert 0 < lib.gcm_dense_gine_bwd_workspace_bytes(256, 128, F, D) < 256 * 128 * F * 4
    assert lib.gcm_dense_gine_fwd_workspace_bytes(256, 128, F, D) == 256 * 128 * 4 * 4       # the bit image
