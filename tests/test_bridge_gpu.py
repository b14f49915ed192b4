"""gcm.gcm.DenseToSparse / SparseToDense on the GPU (csrc/dense_sparse.hip): the edge list and its attached index
against the restatement (tests/_bridge_restate.py) and against the sorted index, bit for bit; SparseToDense and every
gradient against the restatement; sparse layers behind the bridge against their dense twins and a DenseGCM on the
bridge against the same memory on DenseGraphConv, bounded by the float64 evaluation (tests/_golden.py's rule: at most
3x the fp32 restatement's own distance, its floors); and the reference's TestSparseGCM (tests/test_gcm.py:442-550).
No test starts a stream capture: the error of that branch is checked by reading it (tests/test_bridge_cpu.py)."""
import copy

import pytest
import torch

import _bridge_restate as R
import _mp_restate as MP
from _gcn_restate import assert_bounded
from oracle import dense as od

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _mods():
    from gcm import _ops, nn as G
    from gcm.gcm import DenseGCM, DenseToSparse, SparseToDense
    return G, _ops, DenseGCM, DenseToSparse, SparseToDense


def _x(B, N, F=3):
    return torch.arange(B * N * F, dtype=torch.float32).view(B, N, F) / 7


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), what


def _check_index(_ops, ei, graph, M, transpose, what):
    """The attached index equals the one a stable sort gives (GraphIndex.from_edge_index and its csc())."""
    want = _ops.GraphIndex.from_edge_index(ei, M)
    E = ei.shape[1]
    assert graph.M == M and graph.E == E and graph.mask is None and graph.edge_index is ei
    _same(graph.row_ptr, want.row_ptr, what + " row_ptr")
    if transpose:       # the list is in sink order already: no permutation, and the sort's is the identity
        assert graph.csr_perm is None
        _same(want.csr_perm, torch.arange(E, device=DEV), what + " sorted perm")
    else:
        _same(graph.csr_perm, want.csr_perm, what + " csr_perm")
    _same(graph.col, want.col, what + " col")
    _same(graph.dst_csr(), want.dst_csr(), what + " dst_csr")
    assert graph._csc is not None, "the CSC view must come prebuilt"
    for got, ref, name in zip(graph.csc(), want.csc(), ("col_ptr", "rows", "perm")):
        _same(got, ref, f"{what} csc {name}")
    node_off, B, N = graph.batches
    assert B * N == M and torch.equal(node_off.cpu(), torch.arange(0, M + 1, N))


# ---- structure ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("B,N", R.SHAPES)
def test_edge_list_and_index(B, N, transpose):
    _, _ops, _, DenseToSparse, _ = _mods()
    bridge = DenseToSparse(transpose=transpose, edge_values=True)
    x = _x(B, N)
    xd = x.to(DEV)
    for kind in R.PATTERNS:
        adj = R.pattern(kind, B, N)
        want = R.dense_to_sparse(x, adj, transpose, edge_values=True)
        got = bridge(xd, adj.to(DEV))
        again = bridge(xd, adj.to(DEV))
        for g, a, w, name in zip(got, again, want, ("x_sp", "edge_index", "batch_idx", "edge_weight")):
            _same(g.cpu(), w.to(g.dtype), f"{kind} {name}")
            _same(g, a, f"{kind} {name}, second call")
        assert got[0].data_ptr() == xd.data_ptr() and got[3].dtype == torch.float32
        _check_index(_ops, got[1], got[1].gcm_graph, B * N, transpose, kind)
        three = DenseToSparse(transpose=transpose)(xd, adj.to(DEV))
        assert len(three) == 3
        _same(three[1], got[1], f"{kind} without values")


@pytest.mark.parametrize("transpose", [False, True])
def test_above_the_kernel_bound_takes_the_torch_path(transpose):
    _, _ops, _, DenseToSparse, _ = _mods()
    B, N = 1, _ops.BRIDGE_MAX_N + 1
    x, adj = _x(B, N, 1), R.pattern("random", B, N)
    want = R.dense_to_sparse(x, adj, transpose, edge_values=True)
    bridge = DenseToSparse(transpose=transpose, edge_values=True)
    got, again = bridge(x.to(DEV), adj.to(DEV)), bridge(x.to(DEV), adj.to(DEV))
    for g, a, w in zip(got, again, want):
        _same(g.cpu(), w.to(g.dtype), "fallback")
        _same(g, a, "fallback, second call")
    graph = got[1].gcm_graph
    assert graph.M == N and graph.E == want[1].shape[1]
    _same(graph.row_ptr.cpu(), torch.searchsorted(want[1][1].sort().values, torch.arange(N + 1)), "fallback row_ptr")


def test_other_dtypes_are_converted_first():
    _, _ops, _, DenseToSparse, _ = _mods()
    adj = R.pattern("values", 3, 9)
    for dtype in (torch.float64, torch.float16, torch.int32, torch.bool):
        a = (adj > 0) if dtype is torch.bool else adj.to(dtype)
        want = R.dense_to_sparse(_x(3, 9), a.float(), edge_values=True)
        got = DenseToSparse(edge_values=True)(_x(3, 9).to(DEV), a.to(DEV))
        _same(got[1].cpu(), want[1], str(dtype))
        _same(got[3].cpu(), want[3], str(dtype))


# ---- SparseToDense -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", R.SHAPES)
def test_round_trip(B, N):
    _, _, _, DenseToSparse, SparseToDense = _mods()
    x = _x(B, N).to(DEV)
    for kind in R.PATTERNS:
        adj = R.pattern(kind, B, N).to(DEV)
        want = (adj > 0).float()
        for transpose in (False, True):
            x_sp, ei, batch = DenseToSparse(transpose=transpose)(x, adj)
            x_d, adj_d = SparseToDense()(x_sp, ei, batch, B, N)
            _same(x_d, x, f"{kind} x")
            _same(adj_d, want.transpose(1, 2).contiguous() if transpose else want, f"{kind} adj")
            ei_plain = ei.clone()                   # no index attached: SparseToDense builds one
            assert not hasattr(ei_plain, "gcm_graph")
            _same(SparseToDense()(x_sp, ei_plain, batch, B, N)[1], adj_d, f"{kind} adj from a plain list")


def _ragged(seed=0):
    """Graphs of 4, 0, 7 and 2 nodes (B = 4): random edges inside each, the edge 0 -> 1 three times, a loop, and an edge
    from graph 2 to graph 3; shuffled."""
    gen = torch.Generator().manual_seed(seed)
    sizes, first = [4, 0, 7, 2], [0, 4, 4, 11]
    batch = torch.cat([torch.full((n,), b) for b, n in enumerate(sizes)])
    ei = [torch.randint(0, n, (2, 3 * n), generator=gen) + first[b] for b, n in enumerate(sizes) if n]
    ei = torch.cat(ei + [torch.tensor([[0, 0, 0, 5, 5], [1, 1, 1, 5, 12]])], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=gen)]
    return batch, ei, torch.randn(13, 5, generator=gen)


@pytest.mark.parametrize("N", [3, 7, 9])        # nodes and edges beyond N dropped / exact / padded
@pytest.mark.parametrize("weighted", [False, True])
def test_sparse_to_dense_against_the_restatement(N, weighted):
    """Duplicates add, what lies beyond N is dropped, a graph without nodes is zero; the gradients of x_sp and of the
    weights are gathers, so they equal the fp32 restatement's exactly.  The weights are multiples of 1/4: the sum of
    duplicates is then exact in any order, and the forward is compared bit for bit as well."""
    _, _, _, _, SparseToDense = _mods()
    B = 4
    batch, ei, x = _ragged(1)
    gen = torch.Generator().manual_seed(3)
    w = torch.randint(-4, 5, (ei.shape[1],), generator=gen).float() / 4 if weighted else None
    g_x, g_adj = torch.randn(B, N, 5, generator=gen), torch.randn(B, N, N, generator=gen)

    xr = x.clone().requires_grad_(True)
    wr = None if w is None else w.clone().requires_grad_(True)
    want_x, want_adj = R.sparse_to_dense(xr, ei, batch, B, N, wr)
    ((want_x * g_x).sum() + (want_adj * g_adj).sum()).backward()

    xd = x.to(DEV).requires_grad_(True)
    wd = None if w is None else w.to(DEV).requires_grad_(True)
    got_x, got_adj = SparseToDense()(xd, ei.to(DEV), batch.to(DEV), B, N, wd)
    ((got_x * g_x.to(DEV)).sum() + (got_adj * g_adj.to(DEV)).sum()).backward()
    _same(got_x.detach().cpu(), want_x.detach(), "x")
    _same(got_adj.detach().cpu(), want_adj.detach(), "adj")
    assert float(want_adj.detach()[0].abs().max()) >= (0.0 if weighted else 3.0)      # 0 -> 1 three times
    _same(xd.grad.cpu(), xr.grad, "x_sp.grad")
    if weighted:
        _same(wd.grad.cpu(), wr.grad, "edge_weight.grad")
    again = SparseToDense()(xd, ei.to(DEV), batch.to(DEV), B, N, wd)
    _same(again[1], got_adj, "second call")


def test_duplicate_weights_add_in_list_order():
    """Weights that do not add exactly: every sink sums its entries in list order, as the restatement's index_put on
    the CPU does, and two calls agree bit for bit."""
    _, _, _, _, SparseToDense = _mods()
    gen = torch.Generator().manual_seed(5)
    ei = torch.tensor([[0, 0, 0, 0, 2, 2, 2], [1, 1, 1, 1, 1, 1, 1]])
    ei = ei[:, torch.randperm(7, generator=gen)]
    w = torch.randn(7, generator=gen) * torch.tensor([1e4, 1.0, 1e-4, 1e2, 1.0, 1e3, 1e-3])
    batch = torch.zeros(3, dtype=torch.long)
    want = torch.zeros(3, 3, dtype=torch.float32)
    for e in range(7):
        want[ei[0, e], ei[1, e]] += w[e]
    got = SparseToDense()(torch.zeros(3, 1, device=DEV), ei.to(DEV), batch.to(DEV), 1, 3, w.to(DEV))[1]
    _same(got[0].cpu(), want, "sum in list order")


def test_edge_values_gradient():
    _, _, _, DenseToSparse, _ = _mods()
    for B, N in [(3, 64), (2, 130)]:
        for transpose in (False, True):
            adj = R.pattern("values", B, N)
            a_r = adj.clone().requires_grad_(True)
            w_r = R.dense_to_sparse(_x(B, N), a_r, transpose, edge_values=True)[3]
            g = torch.randn(w_r.numel(), generator=torch.Generator().manual_seed(B))
            (w_r * g).sum().backward()
            a_d = adj.to(DEV).requires_grad_(True)
            w_d = DenseToSparse(transpose=transpose, edge_values=True)(_x(B, N).to(DEV), a_d)[3]
            assert w_d.requires_grad
            (w_d * g.to(DEV)).sum().backward()
            _same(a_d.grad.cpu(), a_r.grad, "adj.grad")


# ---- layers behind the bridge --------------------------------------------------------------------------------------
def _dense_graphconv(x, adj, conv):
    """out[b,i] = lin_rel(sum_j adj[b,i,j] x[b,j]) + lin_root(x[b,i]): DenseGraphConv restated, dtype generic."""
    return conv.lin_rel(adj @ x) + conv.lin_root(x)


def _grads(out, g, tensors):
    return torch.autograd.grad((out * g).sum(), tensors, allow_unused=True)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("transpose", [True, False])
@pytest.mark.parametrize("B,N", [(3, 10), (2, 65)])
def test_graphconv_behind_the_bridge_equals_its_dense_twin(B, N, transpose, weighted):
    """transpose=True: GraphConv on the bridge's list == DenseGraphConv on the same adj.  transpose=False (the
    reference's orientation): == DenseGraphConv on adj transposed.  Weighted: the edge values as edge_weight."""
    G, _, _, DenseToSparse, _ = _mods()
    F, H = 6, 5
    gen = torch.Generator().manual_seed(10 * B + N)
    adj = R.pattern("random", B, N)
    if weighted:
        adj = adj * torch.tensor([0.5, 2.0])[torch.randint(0, 2, adj.shape, generator=gen)]
    x, g = torch.randn(B, N, F, generator=gen), torch.randn(B, N, H, generator=gen)
    torch.manual_seed(3)
    dense = G.DenseGraphConv(F, H)
    sparse = G.GraphConv(F, H)
    sparse.load_state_dict(dense.state_dict())
    seen = adj if transpose else adj.transpose(1, 2).contiguous()      # what the dense twin must be given

    def restated(dtype):
        m = copy.deepcopy(dense).to(dtype)
        xs, a = x.clone().to(dtype).requires_grad_(True), seen.clone().to(dtype).requires_grad_(True)
        out = _dense_graphconv(xs, a, m)
        return out, _grads(out, g.to(dtype), [xs, a] + list(m.parameters()))

    o64, g64 = restated(torch.float64)
    o32, g32 = restated(torch.float32)

    dense, sparse = dense.to(DEV), sparse.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    ad = adj.to(DEV).requires_grad_(weighted)
    res = DenseToSparse(transpose=transpose, edge_values=weighted)(xd, ad)
    out = sparse(res[0], res[1], res[3] if weighted else None).view(B, N, H)
    got = _grads(out, g.to(DEV), [xd] + ([ad] if weighted else []) + list(sparse.parameters()))
    assert_bounded(out, o64, o32, "bridge + GraphConv")
    names = ["x", "adj", "lin_rel.weight", "lin_rel.bias", "lin_root.weight"]
    if not weighted:
        names.remove("adj")
    for name, grad in zip(names, got):
        i = ["x", "adj", "lin_rel.weight", "lin_rel.bias", "lin_root.weight"].index(name)
        w64, w32 = g64[i], g32[i]
        if name == "adj":           # the bridge differentiates the entries that are edges; back in adj's own layout
            mask = (seen > 0)
            w64, w32 = w64 * mask, w32 * mask
            grad = grad if transpose else grad.transpose(1, 2)
        assert_bounded(grad, w64, w32, "bridge + GraphConv: d " + name, floor=5e-7, relative=True)
    # and the dense twin on the device, under the same bound
    x2 = x.to(DEV).requires_grad_(True)
    out2 = dense(x2, seen.to(DEV))
    assert_bounded(out2, o64, o32, "DenseGraphConv")
    assert_bounded(_grads(out2, g.to(DEV), [x2])[0], g64[0], g32[0], "DenseGraphConv: d x", floor=5e-7, relative=True)


def test_message_passing_subclass_behind_the_bridge():
    """GATv2 written on gcm.nn.MessagePassing (tests/_mp_restate.py) behind DenseToSparse(transpose=True), against the
    same body on the restated base class fed by the restated bridge."""
    G, _, _, DenseToSparse, _ = _mods()
    B, N, F, C = 3, 10, 6, 4
    gen = torch.Generator().manual_seed(8)
    adj, x = R.pattern("random", B, N), torch.randn(B, N, F, generator=gen)
    g = torch.randn(B * N, 2 * C, generator=gen)
    torch.manual_seed(9)
    ref = MP.layers(MP.RefMessagePassing).GATv2(F, C, heads=2)
    dev = MP.layers(G.MessagePassing, G).GATv2(F, C, heads=2)
    dev.load_state_dict(ref.state_dict())
    assert isinstance(dev, G.MessagePassing)

    def restated(dtype):
        m = copy.deepcopy(ref).to(dtype)
        xs = x.clone().to(dtype).requires_grad_(True)
        x_sp, ei, _ = R.dense_to_sparse(xs, adj, transpose=True)
        out = m(x_sp, ei)
        return out, _grads(out, g.to(dtype), [xs] + list(m.parameters()))

    o64, g64 = restated(torch.float64)
    o32, g32 = restated(torch.float32)
    dev = dev.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    x_sp, ei, _ = DenseToSparse(transpose=True)(xd, adj.to(DEV))
    out = dev(x_sp, ei)
    got = _grads(out, g.to(DEV), [xd] + list(dev.parameters()))
    assert_bounded(out, o64, o32, "bridge + GATv2")
    for (name, _), grad, w64, w32 in zip([("x", None)] + list(dev.named_parameters()), got, g64, g32):
        assert_bounded(grad, w64, w32, "bridge + GATv2: d " + name, floor=5e-7, relative=True)


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_densegcm_on_the_bridge_equals_densegcm_on_dense_layers():
    """B = 3, N = 8, F = 6, T = 11 (the overflow is crossed at t = 8), TemporalBackedge([1, 2]): the memory whose GNN is
    bridge + two GraphConv + Tanh, and the same memory on DenseGraphConv, both against the oracle in float64 -
    beliefs, parameter and observation gradients; rollout() equals T calls."""
    from _golden import fp64_rollout_bounds
    from gcm.edge_selectors.temporal import TemporalBackedge
    G, _, DenseGCM, DenseToSparse, SparseToDense = _mods()
    B, N, F, T = 3, 8, 6, 11
    torch.manual_seed(21)
    ref = od.canonical_gnn(F, F)
    obs = torch.rand(T, B, F)
    w = torch.linspace(0.5, 1.5, T * B * F).view(T, B, F)
    out32, hid32, bounds, (out64, out_atol) = fp64_rollout_bounds(
        ref, obs.clone().requires_grad_(True), None, w, lambda: od.TemporalBackedge([1, 2]), N)

    dense_gnn = G.Sequential("x, adj, weights, B, N", [
        (G.DenseGraphConv(F, F), "x, adj -> x"), torch.nn.Tanh(),
        (G.DenseGraphConv(F, F), "x, adj -> x"), torch.nn.Tanh()])
    dense_gnn.load_state_dict(ref.state_dict())
    sparse_gnn = G.Sequential("x, adj, weights, B, N", [
        (DenseToSparse(transpose=True), "x, adj -> x_sp, edge_index, batch_idx"),
        (G.GraphConv(F, F), "x_sp, edge_index -> x_sp"), torch.nn.Tanh(),
        (G.GraphConv(F, F), "x_sp, edge_index -> x_sp"), torch.nn.Tanh(),
        (SparseToDense(), "x_sp, edge_index, batch_idx, B, N -> x, adj"),
        (lambda x: x, "x -> x")])
    names = [k for k, _ in ref.named_parameters()]
    assert len(names) == len(list(sparse_gnn.parameters())) == 6
    with torch.no_grad():
        for p, q in zip(sparse_gnn.parameters(), ref.parameters()):
            p.copy_(q)

    for what, gnn in (("bridge", sparse_gnn), ("dense", dense_gnn)):
        gnn = gnn.to(DEV)
        mem = DenseGCM(gnn, edge_selectors=TemporalBackedge([1, 2]), graph_size=N)
        o = obs.to(DEV).requires_grad_(True)
        hidden, outs = None, []
        for t in range(T):
            mx, hidden = mem(o[t], hidden)
            outs.append(mx)
        out = torch.stack(outs)
        (out * w.to(DEV)).sum().backward()
        mem.check_flags()
        err = float((out.detach().cpu().double() - out64).abs().max())
        assert err <= out_atol, f"{what}: beliefs {err:.3e} > {out_atol:.3e}"
        for i in (0, 1, 3):
            assert torch.equal(hidden[i].detach().cpu(), hid32[i]), (what, i)
        for k, grad in [("obs", o.grad)] + list(zip(names, [p.grad for p in gnn.parameters()])):
            g64, atol = bounds[k]
            err = float((grad.cpu().double() - g64).abs().max())
            assert err <= atol, f"{what}: d {k} {err:.3e} > {atol:.3e}"
        if what == "bridge":
            with torch.no_grad():
                rolled, hid_r = mem.rollout(obs.to(DEV))
            assert torch.equal(rolled, out.detach()), "rollout() != T calls"
            for i in (0, 1, 3):
                assert torch.equal(hid_r[i], hidden[i].detach()), i


# ---- the reference's TestSparseGCM (tests/test_gcm.py:442-550) -----------------------------------------------------
class _Reference:
    """setUp of the reference's TestSparseGCM: its GNN verbatim (the lambda stage and the trailing comma included),
    with gcm.nn.GCNConv and gcm.nn.Sequential for torch_geometric's.  The stored adjacency is float32 where the
    reference passes int64: this DenseGCM asserts a float32 adjacency, as it always has (the int64 form goes through
    the bridge directly in test_reference_round_trip)."""

    def __init__(self):
        G, _, DenseGCM, DenseToSparse, SparseToDense = _mods()
        feats = 11
        batches = 5
        N = 10
        conv_type = G.GCNConv
        torch.manual_seed(0)
        self.g = G.Sequential(
            "x, adj, weights, B, N",
            [
                (DenseToSparse(), "x, adj, -> x_sp, edge_index, batch_idx"),
                (conv_type(feats, feats), "x_sp, edge_index -> x_sp"),
                (torch.nn.ReLU()),
                (conv_type(feats, feats), "x_sp, edge_index -> x_sp"),
                (torch.nn.ReLU()),
                (SparseToDense(), "x_sp, edge_index, batch_idx, B, N -> x, adj"),
                # Return only x not adj
                (lambda x: x, "x -> x"),
            ],
        ).to(DEV)
        self.s = DenseGCM(self.g)
        self.optimizer = torch.optim.Adam(self.s.parameters(), lr=0.005)
        self.nodes = torch.arange(batches * N * feats, dtype=torch.float, device=DEV).reshape(batches, N, feats)
        self.obs = torch.ones(batches, feats, device=DEV)
        self.adj = torch.zeros(batches, N, N, device=DEV)
        self.adj[:, 0:2, 3:4] = 1
        self.weights = torch.ones(batches, N, N, device=DEV)
        self.num_nodes = torch.zeros(batches, dtype=torch.long, device=DEV)


def test_reference_zeroth_and_first_entry():
    r = _Reference()
    _, (nodes, adj, weights, num_nodes) = r.s(r.obs, (r.nodes, r.adj, r.weights, r.num_nodes))
    assert not torch.any(nodes[:, 0] != r.obs)
    _, (nodes, adj, weights, num_nodes) = r.s(r.obs, (nodes, adj, weights, num_nodes))
    assert not torch.any(nodes[:, 1] != r.obs)


def test_reference_round_trip():
    G, _, _, DenseToSparse, SparseToDense = _mods()
    r = _Reference()
    B, N = r.nodes.shape[0], r.nodes.shape[1]
    adj = r.adj.long()                          # the reference's int64 adjacency
    seq = G.Sequential(
        "x, adj, weights, B, N",
        [
            (DenseToSparse(), "x, adj -> x_sp, edge_index, batch_idx"),
            (SparseToDense(), "x_sp, edge_index, batch_idx, B, N -> x_d, adj_d"),
        ],
    )
    x_d, adj_d = seq(r.nodes.clone(), adj.clone(), r.weights.clone(), B, N)
    assert not torch.any(x_d != r.nodes)
    assert adj_d.shape == (B, N, N) and not torch.any(adj_d != adj)


def test_reference_propagation():
    r = _Reference()
    out, _ = r.s(r.obs, (r.nodes, r.adj, r.weights, r.num_nodes))
    assert not torch.all(out == r.obs)


def test_reference_sparse_learn():
    r = _Reference()
    feats, batches, T, N = 11, 5, 4, 10
    losses = []
    for i in range(20):
        nodes = torch.arange(batches * N * feats, dtype=torch.float, device=DEV).reshape(batches, N, feats)
        obs = torch.ones(batches, feats, device=DEV)
        adj = torch.zeros(batches, N, N, device=DEV)
        weights = torch.ones(batches, N, N, device=DEV)
        num_nodes = torch.zeros(batches, dtype=torch.long, device=DEV)
        r.s.zero_grad()
        hidden = (nodes, adj, weights, num_nodes)
        for t in range(T):
            obs, hidden = r.s(obs, hidden)
        loss = torch.norm(obs)
        loss.backward()
        losses.append(float(loss))
        r.optimizer.step()
    assert losses[-1] < losses[0], losses
