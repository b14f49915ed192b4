"""Eager, dtype-generic restatement of LearnedEdge(deterministic=True) (edge_selectors/learned.py:78-111 of the
reference with the `deterministic` branch taken): the edges are util.Spardmax of the candidate logits - the published
sparsemax (Martins & Astudillo 2016; oracle.dense.sparsemax) made binary with a straight-through estimator, cutoff 0.
The reference's own import of the `sparsemax` package is commented out, so this is pinned to the published algorithm.
TEST INFRASTRUCTURE ONLY: what the HIP kernels of csrc/learned_sparsemax.hip are compared against, evaluated in float64
for the bound and in float32 for the restatement's own error."""
import math

import torch

from oracle import dense as od


def sparsemax_select(logits, adj, cur):
    """logits [B, N] (entries j >= n_b are not read), adj [B, N, N], cur [B] (clamped to [0, N-1]; n_b = cur_b) ->
    (new_adj, soft [B, N], margin): row cur_b of adj rewritten for j < n_b as STE(Spardmax(z[:n_b]) + adj), soft =
    sparsemax(z[:n_b]) padded with zeros, margin = min over the live rows and j < n_b of |z_j - tau| (inf without a
    live row).  Running sparsemax over [:n_b] equals the reference's [B, max n] matrix filled with -1e10: for
    n_b >= 1 a fill entry never enters the support, for n_b = 0 no entry is read back (tests/test_learned_det_cpu.py
    checks it).  Functional: the inputs are not modified; gradients flow to logits and adj."""
    B, N = logits.shape
    cur = cur.clamp(0, N - 1)
    new_adj = adj.clone()
    soft, margin = [], math.inf
    for b in range(B):
        n = int(cur[b])
        if n == 0:
            soft.append(logits.new_zeros(N))
            continue
        z = logits[b, :n]
        p = od.sparsemax(z)
        with torch.no_grad():
            tau = (z - p)[int(p.argmax())]                        # p_j = z_j - tau on the support
            margin = min(margin, float((z - tau).abs().min()))
        edges = (p > 0).to(p.dtype) - p.detach() + p              # util.Spardmax, util.py:38-42 (cutoff 0)
        j = torch.arange(n)
        row = torch.full((n,), n)
        new_adj = new_adj.index_put((torch.full((n,), b), row, j), od._STE.apply(edges + adj[b, n, :n]))
        soft.append(torch.cat((p, p.new_zeros(N - n))))
    return new_adj, torch.stack(soft), margin


class LearnedEdgeDet:
    """f(nodes, adj, weights, num_nodes, B) -> (adj, weights) for oracle.dense.dense_step / dense_rollout, with the
    index logic of oracle.dense.LearnedEdge (learned.py:64-76) in front of sparsemax_select.  `margin`: the smallest
    |z_j - tau| over every live row of every call so far - how far the trajectory stays from a support flip."""

    def __init__(self, edge_network):
        self.net = edge_network
        self.margin = math.inf

    def __call__(self, nodes, adj, weights, num_nodes, B):
        if int(num_nodes.max()) < 1:
            return adj, weights
        N = adj.shape[-1]
        past = torch.nonzero(torch.arange(N)[None, :] < num_nodes[:, None])
        b_idx, j_idx = past[:, 0], past[:, 1]
        i_idx = num_nodes[b_idx]
        pair = torch.cat((nodes[b_idx, i_idx], nodes[b_idx, j_idx]), dim=-1)
        logits = self.net(pair).squeeze(-1)
        shaped = logits.new_zeros(B, N).index_put((b_idx, j_idx), logits)
        new_adj, _, margin = sparsemax_select(shaped, adj, num_nodes)
        self.margin = min(self.margin, margin)
        return new_adj, weights


def closed_form_grad(soft, g_adj, cur):
    """The sparsemax Jacobian applied to row cur of g_adj: g_j - mean_{k in S} g_k for j in S = {soft > 0}, else 0."""
    B, N = soft.shape
    cur = cur.clamp(0, N - 1)
    out = torch.zeros_like(soft)
    for b in range(B):
        n = int(cur[b])
        S = soft[b] > 0
        S[n:] = False
        if n == 0 or not bool(S.any()):
            continue
        g = g_adj[b, n]
        out[b, S] = g[S] - g[S].mean()
    return out


def bound(f64, f32_ref, floor=2e-6):
    """atol = max(floor, 3 x the restatement's own fp32 distance from its float64 evaluation): tests/_golden.py:56-68."""
    own = float((f32_ref.detach().double() - f64.detach().double()).abs().max()) if f64.numel() else 0.0
    return max(floor, 3.0 * own)


def assert_bounded(got, f64, f32_ref, what):
    atol = bound(f64, f32_ref)
    err = float((got.detach().cpu().double() - f64.detach().double()).abs().max()) if f64.numel() else 0.0
    print(f"{what}: max error {err:.3e}, bound {atol:.3e}")
    assert err <= atol, f"{what}: max error {err:.3e} > bound {atol:.3e}"
