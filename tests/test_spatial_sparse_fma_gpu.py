"""The spatial selectors' squared distance is the reference's unfused fp32 sum: (x_i - x_j)^2 per column, each
product rounded, added in column order.  A contracted kernel (s = fma(d, d, s), what hipcc makes of `s + d * d`
under its default -ffp-contract=fast-honor-pragmas) differs in the last bit for many pairs; these tests place such
pairs on opposite sides of the radius, and such near-equal candidates in a kNN ranking, so that only the unfused
form passes.  The cases are searched on the CPU with an exact emulation of both forms."""
from fractions import Fraction
import math

import numpy as np
import pytest
import torch

from test_spatial_sparse_cpu import restate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _round32(x):
    """a rational rounded to the nearest float32 (ties to even), exactly"""
    if x == 0:
        return np.float32(0.0)
    e = math.frexp(float(x))[1] - 24          # |x| / 2^e in [2^23, 2^24) (adjusted below)
    m = x / Fraction(2) ** e
    while abs(m) >= 2 ** 24:
        e += 1
        m = x / Fraction(2) ** e
    while abs(m) < 2 ** 23:
        e -= 1
        m = x / Fraction(2) ** e
    q = math.floor(m)
    rem = m - q
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and q % 2):
        q += 1
    return np.float32(float(Fraction(q) * Fraction(2) ** e))


def _diffs(a, b):
    return [np.float32(np.float32(x) - np.float32(y)) for x, y in zip(a, b)]


def ref_d2(a, b):
    """the reference: ((a - b) ** 2).sum(-1) in fp32, in column order"""
    s = np.float32(0.0)
    for d in _diffs(a, b):
        s = np.float32(s + np.float32(d * d))
    return s


def fused_d2(a, b):
    """the contracted form: s = d0 * d0, then s = fma(d, d, s) per further column"""
    ds = _diffs(a, b)
    s = np.float32(ds[0] * ds[0])
    for d in ds[1:]:
        s = _round32(Fraction(float(d)) ** 2 + Fraction(float(s)))
    return s


def find_radius_pairs(P, count, seed=0):
    """(a, b, radius) with sqrt(ref) and sqrt(fused) rounding to different floats; the radius is the larger of the
    two, so exactly one form puts the pair inside it (strict <)"""
    rng = np.random.default_rng(seed + P)
    out = []
    while len(out) < count:
        a = rng.random(P, dtype=np.float32)
        b = rng.random(P, dtype=np.float32)
        r, f = np.sqrt(ref_d2(a, b)), np.sqrt(fused_d2(a, b))
        if r != f:
            out.append((a, b, max(r, f)))
    return out


def find_knn_swap(P, seed=0):
    """(sink x, candidate a, candidate b) whose reference squared distances tie (the same differences in swapped
    columns: the lower index wins) while the fused form ranks b strictly first"""
    rng = np.random.default_rng(100 + seed + P)
    while True:
        x = rng.random(P, dtype=np.float32) * np.float32(0.5) + np.float32(0.25)
        a = rng.random(P, dtype=np.float32) * np.float32(0.5) + np.float32(0.25)
        d = _diffs(x, a)
        perm = list(range(P))[::-1]
        b = np.array([np.float32(x[p] - d[perm[p]]) for p in range(P)], dtype=np.float32)
        if [abs(v) for v in _diffs(x, b)] != [abs(d[perm[p]]) for p in range(P)]:
            continue
        if ref_d2(x, a) == ref_d2(x, b) and fused_d2(x, b) < fused_d2(x, a):
            return x, a, b


def _run(sel, nodes, T, taus):
    out = sel(nodes.to(DEV), T.to(DEV), taus.to(DEV), nodes.shape[0])
    return out.coalesce().indices().cpu()


@pytest.mark.parametrize("P", [2, 3, 5])
def test_radius_uses_the_unfused_sum(P):
    from gcm.sparse_edge_selectors.spatial import SpatialRadiusEdge
    for a, b, radius in find_radius_pairs(P, 6):
        ref_in = bool(np.sqrt(ref_d2(a, b)) < radius)
        assert ref_in != bool(np.sqrt(fused_d2(a, b)) < radius)      # the case separates the two forms
        nodes = torch.from_numpy(np.stack([a, b]))[None]
        T, taus = torch.tensor([0]), torch.tensor([2])
        got = _run(SpatialRadiusEdge(slice(0, P), float(radius)), nodes, T, taus)
        want = restate(nodes, T, taus, list(range(P)), "radius", radius=float(radius))
        assert torch.equal(got, want) and (want.shape[1] == 1) == ref_in
        got = _run(SpatialRadiusEdge(slice(0, P), float(radius), causal=False), nodes, T, taus)
        assert torch.equal(got, restate(nodes, T, taus, list(range(P)), "radius", radius=float(radius),
                                        causal=False))


@pytest.mark.parametrize("P", [2, 3, 5])
def test_knn_ranks_on_the_unfused_sum(P):
    from gcm.sparse_edge_selectors.spatial import SpatialKNNEdge
    x, a, b = find_knn_swap(P)
    nodes = torch.from_numpy(np.stack([a, b, x]))[None]          # candidates 0 and 1, sink 2
    T, taus = torch.tensor([0]), torch.tensor([3])
    got = _run(SpatialKNNEdge(slice(0, P), 2), nodes, T, taus)    # the sink itself + its nearest other node
    want = restate(nodes, T, taus, list(range(P)), "knn", k=2)
    assert [0, 2, 0] in want.T.tolist()                            # tie -> the lower index (a fused kernel: 1)
    assert torch.equal(got, want)
