"""LearnedEdge(deterministic=True): the sparsemax selection kernels (csrc/learned_sparsemax.hip) and the DenseGCM step
on top of them against the eager restatement (tests/_learned_det_restate.py), evaluated in float64 for the bound and in
float32 for the restatement's own error (the rule of tests/_golden.py:56-68: max(2e-6, 3 x that error)).  Supports are
compared exactly, so every case asserts that its float64 margin min |z_j - tau| is >= 1e-3 first - three orders above
what fp32 moves a logit by.  Needs an MI355X."""
import copy
import functools

import pytest
import torch

from _learned_det_restate import LearnedEdgeDet, assert_bounded, sparsemax_select
from oracle import dense as od

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-3


# ---- kernel level -----------------------------------------------------------------------------------
def kernel_case(N, ties):
    """-> (logits [B,N], cur [B], adj [B,N,N] with 0 / 1 / 0.5 entries, g_adj), all on the CPU in fp32.
    ties=False: B = 5 (a part-full block of four waves), logits 3 randn, cur = 0, 1, N-1, an interior value and one
    above N-1 (clamped).  ties=True: B = 3 at cur = N-1: all logits equal (full support); the two largest logits
    exactly equal, in different lanes and - from N = 70 - different columns (both in); the same row shifted by +1e4
    (same support: the logits are multiples of 1/64, so the shift is exact in fp32)."""
    g = torch.Generator().manual_seed(1000 + N + (500 if ties else 0))
    if ties:
        B = 3
        cur = torch.full((B,), N - 1)
        z = (3 * torch.randn(N, generator=g) * 64).round() / 64
        z[3] = z[N - 2] = z.max() + 0.25
        logits = torch.stack((torch.full((N,), 0.703125), z, z + 1e4))
        assert torch.equal(logits[2] - 1e4, z)
    else:
        B = 5
        cur = torch.tensor([0, 1, N - 1, N // 2 + 1, N + 3])
        logits = 3 * torch.randn(B, N, generator=g)
    adj = torch.randint(0, 3, (B, N, N), generator=g).float() * 0.5        # 0, 0.5, 1
    g_adj = torch.randn(B, N, N, generator=g)
    return logits, cur, adj, g_adj


def kernel_reference(N, ties, dtype):
    """The restatement on kernel_case(N, ties) in `dtype`: (new_adj, soft, g_logits, g_adj_in, margin)."""
    logits, cur, adj, g_adj = kernel_case(N, ties)
    logits = logits.to(dtype).requires_grad_(True)
    adj = adj.to(dtype).requires_grad_(True)
    new_adj, soft, margin = sparsemax_select(logits, adj, cur)
    new_adj.backward(g_adj.to(dtype))
    return new_adj.detach(), soft.detach(), logits.grad, adj.grad, margin


@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("N", [8, 70, 130])
def test_sparsemax_kernels_match_the_restatement(N, ties):
    from gcm import _hip, _ops
    logits, cur, adj, g_adj = kernel_case(N, ties)
    B = logits.shape[0]
    adj64, soft64, gz64, ga64, margin = kernel_reference(N, ties, torch.float64)
    adj32, soft32, gz32, _, _ = kernel_reference(N, ties, torch.float32)
    print(f"N={N} ties={ties}: float64 margin {margin:.3e}, support sizes {(soft64 > 0).sum(-1).tolist()}")
    assert margin >= MARGIN             # (the tie rows too: their ties are exact, every other entry is this far off)
    assert torch.equal(adj32.double(), adj64)
    assert torch.equal(ga64, g_adj.double())

    lib, st = _hip.lib(), _hip.stream()
    d_logits, d_cur, d_gadj = logits.to(DEV), cur.to(DEV), g_adj.to(DEV)
    d_adj = adj.to(DEV)
    d_soft = torch.full((B, N), float("nan"), device=DEV)
    _hip.check(lib.gcm_learned_sparsemax_fwd(_hip.ptr(d_logits), _hip.ptr(d_cur), _hip.ptr(d_adj), _hip.ptr(d_soft),
                                             B, N, st), "fwd")
    d_gz = torch.full((B, N), float("nan"), device=DEV)
    _hip.check(lib.gcm_learned_sparsemax_bwd(_hip.ptr(d_gadj), _hip.ptr(d_soft), _hip.ptr(d_cur), _hip.ptr(d_gz),
                                             B, N, st), "bwd")
    got_adj, got_soft, got_gz = d_adj.cpu(), d_soft.cpu(), d_gz.cpu()

    assert torch.equal(got_adj.double(), adj64), "adjacency differs from the restatement"
    curc = cur.clamp(0, N - 1)
    for b in range(B):                  # untouched outside row cur and for j >= n (0.5 entries stay 0.5)
        n = int(curc[b])
        keep = torch.ones(N, N, dtype=torch.bool)
        keep[n, :n] = False
        assert torch.equal(got_adj[b][keep], adj[b][keep])
        assert set(got_adj[b, n, :n].unique().tolist()) <= {0.0, 1.0}
        assert bool((got_adj[b, n, :n][adj[b, n, :n] > 0] == 1).all())     # 0.5 and 1 become 1
        assert float(got_soft[b, n:].abs().sum()) == 0 and float(got_gz[b, n:].abs().sum()) == 0
    assert torch.equal(got_soft > 0, soft64 > 0), "support differs from the restatement"
    assert_bounded(got_soft, soft64, soft32, "soft")
    assert_bounded(got_gz, gz64, gz32, "g_logits")
    if ties:
        n = N - 1
        assert bool((got_soft[0, :n] > 0).all())                           # equal logits: the full support
        assert float(got_soft[0, :n].min()) == float(got_soft[0, :n].max())
        assert float(got_soft[1, 3]) > 0 and float(got_soft[1, 3]) == float(got_soft[1, N - 2])
        assert torch.equal(got_soft[2] > 0, got_soft[1] > 0)               # shifted by 1e4: the same support
        assert_bounded(got_soft[2], soft64[1], soft32[1], "soft of the shifted row")

    # the autograd node: same kernels, in place on the caller-owned adjacency; incoming adjacency gets g_adj itself
    a_leaf = adj.to(DEV).requires_grad_(True)
    z_leaf = logits.to(DEV).requires_grad_(True)
    a_in = a_leaf.clone()
    out = _ops.learned_sparsemax_select_(a_in, z_leaf, d_cur)
    assert out.data_ptr() == a_in.data_ptr()
    out.backward(d_gadj)
    assert torch.equal(out.detach(), d_adj) and torch.equal(z_leaf.grad, d_gz)
    assert torch.equal(a_leaf.grad, d_gadj)


def test_sparsemax_kernels_reject_wide_graphs():
    from gcm import _ops
    B, N = 1, 1025
    with pytest.raises(RuntimeError):
        _ops.learned_sparsemax_select_(torch.zeros(B, N, N, device=DEV), torch.zeros(B, N, device=DEV),
                                       torch.zeros(B, dtype=torch.long, device=DEV))


# ---- end to end -------------------------------------------------------------------------------------
B, N, F, H, T = 3, 8, 4, 8, 11          # overflow from step 8
# The last linear of the edge network is scaled by LOGIT_SCALE: at their initial values the networks give nearly equal
# logits and sparsemax keeps every candidate, which would not test the support.  With these seeds the supports vary
# (60 and 61 of the 84 possible edges survive) and the float64 margins of the trajectories are 1.6e-2 and 6.0e-3
# (asserted in reference(); e.g. seed 1 gives 4.1e-4 for "default" and must not be used).
LOGIT_SCALE = 4.0
SEEDS = {"default": 3, "custom": 4}


def make_nets(kind):
    """-> (oracle GNN, oracle edge network, observations [T,B,F]), fp32 on the CPU."""
    torch.manual_seed(SEEDS[kind])
    gnn = od.canonical_gnn(F, H)
    if kind == "default":
        net = od.build_edge_network(F)
    else:
        net = torch.nn.Sequential(torch.nn.Linear(2 * F, 6), torch.nn.Tanh(), torch.nn.Linear(6, 1))
    with torch.no_grad():
        net[-1].weight.mul_(LOGIT_SCALE)
    return gnn, net, torch.rand(T, B, F)


def oracle_run(kind, dtype):
    gnn, net, obs = make_nets(kind)
    gnn, net = copy.deepcopy(gnn).to(dtype), copy.deepcopy(net).to(dtype)
    obs = obs.to(dtype).requires_grad_(True)
    sel = LearnedEdgeDet(net)
    out, hid = od.dense_rollout(obs, None, gnn, graph_size=N, edge_selectors=sel)
    out.mean().backward()
    grads = {"gnn." + k: p.grad for k, p in gnn.named_parameters()}
    grads.update({"edge." + k: p.grad for k, p in net.named_parameters()})
    grads["obs"] = obs.grad
    return out.detach(), tuple(h.detach() for h in hid), grads, sel.margin


@functools.lru_cache(maxsize=None)
def reference(kind):
    """The restatement's rollout in float64 and float32, computed once per kind and shared (never modified)."""
    r64, r32 = oracle_run(kind, torch.float64), oracle_run(kind, torch.float32)
    print(f"{kind}: float64 margin of the trajectory {r64[3]:.3e}")
    assert r64[3] >= MARGIN
    assert torch.equal(r32[1][1].double(), r64[1][1])
    return r64, r32


def device_memory(kind):
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.learned import LearnedEdge
    from gcm import nn as G
    gnn, net, obs = make_nets(kind)
    dev_gnn = G.Sequential("x, adj, weights, B, N", [
        (G.DenseGraphConv(F, H), "x, adj -> x"), torch.nn.Tanh(),
        (G.DenseGraphConv(H, H), "x, adj -> x"), torch.nn.Tanh()])
    dev_gnn.load_state_dict(gnn.state_dict())
    if kind == "default":
        sel = LearnedEdge(F, deterministic=True)
        sel.edge_network.load_state_dict(net.state_dict())
    else:
        sel = LearnedEdge(model=copy.deepcopy(net), deterministic=True)
    mem = DenseGCM(dev_gnn.to(DEV), edge_selectors=sel.to(DEV), graph_size=N)
    return mem, dev_gnn, sel, obs.to(DEV)


def steps(mem, obs, hidden=None):
    outs = []
    for t in range(obs.shape[0]):
        mx, hidden = mem(obs[t], hidden)
        outs.append(mx)
    return torch.stack(outs), hidden


def check_state(hid, hid64, hid32):
    assert torch.equal(hid[1].detach().cpu().double(), hid64[1]), "adjacency must be exact"
    assert torch.equal(hid[0].detach().cpu(), hid32[0]) and torch.equal(hid[3].cpu(), hid64[3])


@pytest.mark.parametrize("kind", ["default", "custom"])
def test_deterministic_learned_edge_matches_the_restatement(kind):
    """default: the one-node path (pairs -> MLP -> select); custom: a user `model=`, op by op."""
    (out64, hid64, g64, _), (out32, hid32, g32, _) = reference(kind)
    mem, dev_gnn, sel, obs = device_memory(kind)
    assert mem._structure() is None                                     # not the fused LearnedEdge step
    obs.requires_grad_(True)
    out, hid = steps(mem, obs)
    out.mean().backward()
    mem.check_flags()
    assert hid[1].requires_grad                                         # the adjacency carries a gradient
    check_state(hid, hid64, hid32)
    assert_bounded(out, out64, out32, "beliefs")
    got = {"gnn." + k: p.grad for k, p in dev_gnn.named_parameters()}
    got.update({"edge." + k: p.grad for k, p in sel.edge_network.named_parameters()})
    got["obs"] = obs.grad
    assert set(got) == set(g64)
    for k in g64:
        assert got[k] is not None, k
        assert_bounded(got[k], g64[k], g32[k], "grad " + k)


def test_deterministic_steps_repeat_bit_for_bit_and_draw_nothing():
    mem, _, _, obs = device_memory("default")
    with torch.no_grad():
        _, hid = steps(mem, obs[:5])
        state = tuple(t.clone() for t in hid)
        torch.cuda.synchronize()
        rng = torch.cuda.get_rng_state()
        mx1, h1 = mem(obs[5], tuple(t.clone() for t in state))
        torch.cuda.synchronize()
        assert torch.equal(torch.cuda.get_rng_state(), rng), "a deterministic step moved the device RNG"
        mx2, h2 = mem(obs[5], tuple(t.clone() for t in state))
    assert torch.equal(mx1, mx2) and torch.equal(h1[1], h2[1]) and torch.equal(h1[0], h2[0])
    assert float(h1[1][:, 5].sum()) >= B                                 # every graph chose at least one edge
    # ... and from empty graphs, whole trajectories (the parent commit sampled: they differed)
    with torch.no_grad():
        o1, ha = steps(mem, obs)
        o2, hb = steps(mem, obs)
    assert torch.equal(o1, o2) and torch.equal(ha[1], hb[1])


@pytest.mark.parametrize("kind", ["default", "custom"])
def test_rollout_equals_single_steps(kind):
    (out64, hid64, _, _), (out32, hid32, _, _) = reference(kind)
    mem, _, _, obs = device_memory(kind)
    with torch.no_grad():
        want, hid_s = steps(mem, obs)
    out, hid = mem.rollout(obs)
    mem.check_flags()
    for a, b in zip(hid, hid_s):
        assert torch.equal(a.detach(), b.detach())
    check_state(hid, hid64, hid32)
    assert_bounded(out, out64, out32, "rollout beliefs")
    assert_bounded(want, out64, out32, "step beliefs")


def test_deterministic_step_is_capturable():
    """4 steps forward + backward on the layered path, captured in a HIP graph and replayed: no host synchronisation
    between the state advance and the selection kernels."""
    mem, dev_gnn, sel, obs = device_memory("default")
    with torch.no_grad():
        _, h0 = steps(mem, obs[:3])
    h0 = tuple(t.detach().clone() for t in h0)
    params = list(dev_gnn.parameters()) + list(sel.parameters())
    x = obs[3:7].clone().requires_grad_(True)

    def run():
        out, hid = steps(mem, x, tuple(t.clone() for t in h0))
        out.mean().backward()
        return out, hid

    def clear():
        for p in params + [x]:
            p.grad = None

    def eager():
        out, hid = run()
        return [out.detach().clone(), hid[1].detach().clone()] + [p.grad.clone() for p in params + [x]]

    # (no autograd graph of an eager run may outlive this line: it would keep the parameters' AccumulateGrad nodes
    #  alive, bound to the stream they were made on, and the captured backward would then synchronise with that
    #  stream: a segmentation fault when the capture ends - DESIGN 3.11)
    want = eager()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            clear()
            run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, hid = run()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    got = [out.detach(), hid[1].detach()] + [p.grad for p in params + [x]]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    mem.check_flags()
