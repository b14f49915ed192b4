"""Restatement of the GEMM-form backward of csrc/rows_bptt_hops.hip in torch (any float dtype; float64 for bounds).

A DenseGCM chain from empty graphs with forward temporal hops, tanh / tanh: step t writes row t, aggregates the rows
t - h >= 0 for the distinct hops h > 0 (a hop of 0: the row itself).  Layer-1 rows are final once written, so with
s a step of the call and j = cur[s] the row it wrote:

    D2[s]    = g_mx[s] * (1 - mx[s]^2)
    U[s]     = D2[s] . [W_rel2 | W_root2]  = [dAgg2 | dH1c]
    dW_rel2  = D2^T . AGG2     dW_root2 = D2^T . H1CUR     db2 = colsum D2
    G1pre[j] = sum_{s : j = cur[s] - h, h a hop > 0} dAgg2[s]  +  (j = cur[s'] ?  dH1c[s'] + self * dAgg2[s']  :  0)
    G1[j]    = G1pre[j] * (1 - cH[j]^2)
    dW_rel1  = G1^T . cA       dW_root1 = G1^T . cX        db1 = colsum G1

`forward_empty` builds the chain's caches and records in closed form, `backward` is the formulas above; both batched
over the graphs, summed over them at the end."""
import torch

PARAM_KEYS = ("module_0.lin_rel.weight", "module_0.lin_root.weight", "module_0.lin_rel.bias",
              "module_2.lin_rel.weight", "module_2.lin_root.weight", "module_2.lin_rel.bias")   # the order of the packed vector / a slab


def split_hops(hops):
    """-> (distinct hops 0 < h < 128 ascending, self loop present)"""
    return sorted({int(h) for h in hops if 0 < int(h) < 128}), any(int(h) == 0 for h in hops)


def forward_empty(obs, params, hops):
    """obs [T, B, F] fed into empty graphs of >= T nodes; params: {PARAM_KEYS name: tensor}.
    -> cX [B,T,F], cA [B,T,F], cH [B,T,H1], v = agg2 | h1cur [T,B,2 H1], mx [T,B,H2]"""
    hs, self_loop = split_hops(hops)
    T, B, F = obs.shape
    w_rel1, w_root1, b1, w_rel2, w_root2, b2 = (params[k] for k in PARAM_KEYS)
    cX = obs.transpose(0, 1).contiguous()
    cA = torch.zeros_like(cX)
    for h in hs:
        if h < T:
            cA[:, h:] += cX[:, :T - h]
    if self_loop:
        cA = cA + cX
    cH = torch.tanh(cA @ w_rel1.T + b1 + cX @ w_root1.T)
    agg2 = torch.zeros_like(cH)
    for h in hs:
        if h < T:
            agg2[:, h:] += cH[:, :T - h]
    if self_loop:
        agg2 = agg2 + cH
    mx = torch.tanh(agg2 @ w_rel2.T + b2 + cH @ w_root2.T)
    v = torch.cat([agg2, cH], dim=2).transpose(0, 1).contiguous()
    return cX, cA, cH, v, mx.transpose(0, 1).contiguous()


def backward(mx, v, g_mx, cur, cH, cA, cX, w_rel2, w_root2, hops):
    """mx [S,B,H2], v [S,B,2 H1], g_mx [S,B,H2] of the S steps of the call, cur[s] the row step s wrote; the caches
    [B,R,.] restricted to the R rows the chain has written.  -> {PARAM_KEYS name: gradient}"""
    hs, self_loop = split_hops(hops)
    H1 = cH.shape[2]
    D2 = g_mx * (1 - mx * mx)
    U = D2 @ torch.cat([w_rel2, w_root2], dim=1)            # [S,B,2 H1]
    dagg2, dh1c = U[..., :H1], U[..., H1:]
    G1pre = torch.zeros_like(cH)
    for s, j in enumerate(cur):
        for h in hs:
            if j - h >= 0:
                G1pre[:, j - h] += dagg2[s]
        G1pre[:, j] += dh1c[s] + (dagg2[s] if self_loop else 0)
    G1 = G1pre * (1 - cH * cH)
    return {
        PARAM_KEYS[0]: torch.einsum("bjh,bjf->hf", G1, cA),
        PARAM_KEYS[1]: torch.einsum("bjh,bjf->hf", G1, cX),
        PARAM_KEYS[2]: G1.sum((0, 1)),
        PARAM_KEYS[3]: torch.einsum("sbo,sbk->ok", D2, v[..., :H1]),
        PARAM_KEYS[4]: torch.einsum("sbo,sbk->ok", D2, v[..., H1:]),
        PARAM_KEYS[5]: D2.sum((0, 1)),
    }


def pack(grads):
    return torch.cat([grads[k].reshape(-1) for k in PARAM_KEYS])


def bound(g32, g64, factor=3.0, floor=5e-7):
    """tests/_golden.py's rule (fp64_grad_bound / fp64_rollout_bounds; factor and floor are those functions' defaults, not
    a new tolerance): atol = max(factor x |the same computation in fp32 - fp64|, floor x the gradient's scale).  _golden's
    functions run the oracle's rollout, which has no entry for records a kernel wrote; here the fp32 leg is the
    restatement's own fp32 run on those records - a backward alone, so an error no larger than the reference's fp32
    forward + backward: the bound is the tighter of the two."""
    return max(factor * float((g32.double() - g64).abs().max()), floor * float(g64.abs().max()))


# (hops, N, T): the lean step's cases (tests/test_cached_lean_gpu.py), the K loops at full length, and a chain shorter
# than its largest hop
CASES = [([1, 2, 4], 128, 128), ([1, 2, 4], 40, 25), ([1], 32, 32), ([3, 5], 24, 17), ([0, 1, 2, 4], 128, 60),
         ([0, 3, 5], 16, 16), ([2, 4, 1, 2], 20, 20), ([3, 5], 8, 5)]
