"""The folded GEMM-form backward (csrc/rows_bptt_hops.hip: k_bptt_hops_graph_fold behind gcm_dense_rows_bptt_cached_hops;
the kernel before it behind gcm_dense_rows_bptt_cached_hops_unfolded) on the cases the fold can newly get wrong: a
layer-1 wave owns a tile of 32 cache rows and forms the operand of its product from the D2 rows of the row's hop
sources, which other waves wrote - so tiles with one live row, sources in the next tile, sources that do not exist
(a partial loss, a hop beyond the chain, rows at or beyond rows_written that hold NaN), every shape of hop set, the
q < H2 lanes, every activation pair (act1' multiplies the tile in the accumulator's layout) and a step order that is
not the identity.  Each case against the float64 restatement (tests/_bptt_hops_restate.py) under the bound of
tests/test_bptt_hops_gpu.py's _Chain.check, and bit for bit from call to call."""
import ctypes

import pytest
import torch

from test_dense_gpu import DEV
from test_bptt_hops_gpu import _Chain, _desc, F, H1
import _bptt_hops_restate as R

pytestmark = pytest.mark.gpu

NONE, TANH, RELU = 0, 1, 2   # GCM_ACT_*


def _run(ch, steps, grads, sb, sh, act1=TANH, act2=TANH, rows_written=None, caches=None, fold=True):
    """one of the two entries over the records `steps` (step i of the call = record steps[i], which wrote row steps[i])
    -> g_params on the device"""
    hip, lib, B = ch.hip, ch.lib, ch.B
    n = len(steps)
    sv = (ctypes.c_void_p * n)(*[ch.saved[t].data_ptr() for t in steps])
    gm = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
    cb = (ctypes.c_uint8 * n)(*steps)
    ws_bytes = 4 * ch.P * B
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((ch.P,), float("nan"), device=DEV)
    desc = _desc(hip, ch.hops)
    cH, cA, cX = (ch.cH, ch.cA, ch.cX) if caches is None else caches
    p = hip.ptr
    entry = lib.gcm_dense_rows_bptt_cached_hops if fold else lib.gcm_dense_rows_bptt_cached_hops_unfolded
    rc = entry(sv, gm, n, sb, sh, p(ch.params), 3, act1, act2, p(cX), p(cH), p(cA), cb, ctypes.addressof(desc), 1,
               ch.T if rows_written is None else rows_written, None, p(out), p(ws), ws_bytes, B, ch.N, F, H1, ch.H2,
               hip.stream())
    assert rc == 0, rc
    return out


def _both(ch, steps, grads, sb, sh, **kw):
    """two calls on the same inputs: identical bits"""
    new = _run(ch, steps, grads, sb, sh, **kw)
    again = _run(ch, steps, grads, sb, sh, **kw)
    torch.cuda.synchronize()
    assert torch.equal(new.view(torch.int32), again.view(torch.int32))
    return new.cpu()


def _act_grad(y, act):
    """d act / d pre through the activation's OUTPUT (csrc/gcm_common.h gcm_act_grad)"""
    if act == TANH:
        return 1 - y * y
    if act == RELU:
        return (y > 0).to(y.dtype)
    return torch.ones_like(y)


def _restated(ch, steps, g, dtype, act1, act2, rows):
    """_bptt_hops_restate.backward with the two derivatives left open (it is tanh / tanh) and the caches restricted to
    `rows` written rows, on the records the GPU wrote; g [S, B, H2] on the CPU -> packed gradient"""
    B, H2 = ch.B, ch.H2
    mx = torch.stack([ch.saved[t][:B * H2].view(B, H2) for t in steps]).cpu().to(dtype)
    v = torch.stack([ch.saved[t][ch.o_v:ch.o_v + B * 64].view(B, 64) for t in steps]).cpu().to(dtype)
    cH, cA, cX = (c[:, :rows].cpu().to(dtype) for c in (ch.cH, ch.cA, ch.cX))
    par = ch.params.cpu().to(dtype)
    w_rel2 = par[2 * H1 * F + H1:2 * H1 * F + H1 + H2 * H1].view(H2, H1)
    w_root2 = par[2 * H1 * F + H1 + H2 * H1:2 * H1 * F + H1 + 2 * H2 * H1].view(H2, H1)
    hs, self_loop = R.split_hops(ch.hops)
    D2 = g.to(dtype) * _act_grad(mx, act2)
    U = D2 @ torch.cat([w_rel2, w_root2], dim=1)
    dagg2, dh1c = U[..., :H1], U[..., H1:]
    G1pre = torch.zeros_like(cH)
    for s, j in enumerate(steps):
        for h in hs:
            if j - h >= 0:
                G1pre[:, j - h] += dagg2[s]
        G1pre[:, j] += dh1c[s] + (dagg2[s] if self_loop else 0)
    G1 = G1pre * _act_grad(cH, act1)
    return R.pack({
        R.PARAM_KEYS[0]: torch.einsum("bjh,bjf->hf", G1, cA), R.PARAM_KEYS[1]: torch.einsum("bjh,bjf->hf", G1, cX),
        R.PARAM_KEYS[2]: G1.sum((0, 1)),
        R.PARAM_KEYS[3]: torch.einsum("sbo,sbk->ok", D2, v[..., :H1]),
        R.PARAM_KEYS[4]: torch.einsum("sbo,sbk->ok", D2, v[..., H1:]), R.PARAM_KEYS[5]: D2.sum((0, 1))})


def _check(ch, got, steps, g, act1=TANH, act2=TANH, rows=None):
    """_Chain.check; for another activation pair or fewer written rows the same rule (R.bound, section by section of the
    packed vector, no NaN) on the restatement above"""
    if act1 == TANH and act2 == TANH and rows is None:
        return ch.check(got, steps, g)
    rows = ch.T if rows is None else rows
    g64 = _restated(ch, steps, g, torch.float64, act1, act2, rows)
    g32 = _restated(ch, steps, g, torch.float32, act1, act2, rows)
    assert not bool(torch.isnan(got).any())
    H2, o = ch.H2, 0
    for n in (H1 * F, H1 * F, H1, H2 * H1, H2 * H1, H2):
        atol = R.bound(g32[o:o + n], g64[o:o + n])
        err = float((got[o:o + n].double() - g64[o:o + n]).abs().max())
        print("section at %d: err %.3g, bound %.3g" % (o, err, atol))
        assert err <= atol, (o, err, atol)
        o += n


@pytest.fixture(scope="module")
def chains():
    """one chain per (hops, B, N, T, H2), built once and left unchanged"""
    cache = {}

    def get(hops, B, N, T, H2):
        key = (tuple(hops), B, N, T, H2)
        if key not in cache:
            cache[key] = _Chain(hops, B, N, H2, T, seed=N + T + H2 + B)
        return cache[key]

    return get


def _grads(T, B, H2, seed):
    g = torch.rand(T, B, H2, generator=torch.Generator().manual_seed(seed))
    return g, g.to(DEV)


def test_restatement_with_open_derivatives_is_the_restatement(chains):
    """_restated at tanh / tanh is tests/_bptt_hops_restate.py's backward: the reference of the other pairs is the
    project's, not a second one."""
    ch = chains([0, 3, 5, 3], 2, 40, 33, 24)
    g, _ = _grads(33, 2, 24, 4)
    steps = list(range(33))
    mine, theirs = _restated(ch, steps, g, torch.float64, TANH, TANH, 33), ch.restated(steps, g, torch.float64)
    assert float((mine - theirs).abs().max()) <= 1e-12 * float(theirs.abs().max())   # (float64 rounding at the most)


# a tile is 32 rows: T = 33 and 65 leave a tile with one live row, and the sources j + h of rows 28 .. 31 (60 .. 63)
# lie in the next tile, which another wave owns
@pytest.mark.parametrize("N,T", [(128, 128), (80, 33), (80, 64), (80, 65)])
def test_fold_tile_ownership(chains, N, T):
    hops, B, H2 = [1, 2, 4], 2, 32
    ch = chains(hops, B, N, T, H2)
    g, gd = _grads(T, B, H2, 5)
    steps = list(range(T))
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1)
    _check(ch, got, steps, g)


@pytest.mark.parametrize("part", ["third", "tail"])
def test_fold_partial_loss(chains, part):
    """step(j) exists while step(j + h) does not, and the other way round."""
    hops, B, N, T, H2 = [1, 2, 4], 2, 80, 33, 32
    ch = chains(hops, B, N, T, H2)
    steps = list(range(0, T, 3)) if part == "third" else list(range(20, T))
    g, gd = _grads(T, B, H2, 7)
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1)
    _check(ch, got, steps, g[steps])


def test_fold_hop_beyond_the_chain(chains):
    hops, B, N, T, H2 = [1, 2, 9], 2, 16, 5, 32
    ch = chains(hops, B, N, T, H2)
    g, gd = _grads(T, B, H2, 8)
    steps = list(range(T))
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1)
    _check(ch, got, steps, g)


def test_fold_nan_rows_behind_rows_written(chains):
    """The first 20 steps with rows_written = 20: the rows 20 .. N - 1 of the caches, filled with NaN here, lie in the
    tile of rows 0 .. 31 beside live rows and in tiles of their own; steps 16 .. 19 have sources at rows >= 20."""
    hops, B, N, T, H2 = [1, 2, 4], 2, 80, 33, 32
    ch = chains(hops, B, N, T, H2)
    R_ = 20
    caches = tuple(c.clone() for c in (ch.cH, ch.cA, ch.cX))
    for c in caches:
        c[:, R_:] = float("nan")
    steps = list(range(R_))
    g, gd = _grads(T, B, H2, 9)
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1, rows_written=R_, caches=caches)
    assert bool(torch.isfinite(got).all())
    _check(ch, got, steps, g[steps], rows=R_)


# four distinct hops; the self loop alone (D2s is D2: both halves read the same row); self and a duplicate; one hop
@pytest.mark.parametrize("hops", [[1, 2, 4, 7], [0], [0, 3, 5, 3], [1]])
def test_fold_hop_sets(chains, hops):
    B, N, T, H2 = 2, 40, 33, 32
    ch = chains(hops, B, N, T, H2)
    g, gd = _grads(T, B, H2, 10)
    steps = list(range(T))
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1)
    _check(ch, got, steps, g)


@pytest.mark.parametrize("H2,B", [(24, 2), (1, 2), (32, 1)])
def test_fold_narrow_beliefs_and_one_graph(chains, H2, B):
    """the q < H2 lanes of D2 and of both weight tiles; one graph"""
    hops, N, T = [0, 1, 2, 4], 40, 33
    ch = chains(hops, B, N, T, H2)
    g, gd = _grads(T, B, H2, 11)
    steps = list(range(T))
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1)
    _check(ch, got, steps, g)


@pytest.mark.parametrize("act2", [NONE, TANH, RELU])
@pytest.mark.parametrize("act1", [NONE, TANH, RELU])
def test_fold_activation_pairs(chains, act1, act2):
    """Every pair the entry accepts, on the records of a tanh / tanh chain (the backward reads the activations' outputs,
    which lie in (-1, 1) with both signs): act1' multiplies the sum of two half-products."""
    hops, B, N, T, H2 = [0, 1, 2, 4], 2, 40, 33, 24
    ch = chains(hops, B, N, T, H2)
    g, gd = _grads(T, B, H2, 12)
    steps = list(range(T))
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1, act1=act1, act2=act2)
    _check(ch, got, steps, g, act1, act2)


@pytest.mark.parametrize("hops,N,T,H2", [([1, 2, 4], 80, 65, 32), ([0, 3, 5, 3], 40, 33, 24)])
def test_fold_reversed_steps(chains, hops, N, T, H2):
    """Step i wrote row T - 1 - i: the map is not the identity, the wave that owns a row's tile does not own its step."""
    B = 2
    ch = chains(hops, B, N, T, H2)
    g, gd = _grads(T, B, H2, 6)
    steps = list(range(T))[::-1]
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1)
    _check(ch, got, steps, g[steps])


def test_fold_switch():
    """The kernel before the fold behind its own entry: equal to itself bit for bit, and both forms inside the bound."""
    hops, B, N, T, H2 = [1, 2, 4], 9, 128, 128, 32
    ch = _Chain(hops, B, N, H2, T, seed=N + T + H2)
    g, gd = _grads(T, B, H2, 5)
    steps = list(range(T))
    off = _both(ch, steps, [gd[t] for t in steps], H2, 1, fold=False)
    on = _both(ch, steps, [gd[t] for t in steps], H2, 1, fold=True)
    _check(ch, off, steps, g)
    _check(ch, on, steps, g)


def test_fold_switch_through_the_module(monkeypatch):
    """DenseGCM.rows_hops_fold (env GCM_BPTT_HOPS_FOLD, read when the module is made): the kernel that ran, by name, and
    the gradients of both against the oracle's float64 bounds."""
    from test_bptt_hops_gpu import _module_run, _check_vs_oracle, NEW
    hops, N, T, H2 = [1, 2, 4], 64, 40, 32
    runs = []
    for env in ("1", "0"):
        monkeypatch.setenv("GCM_BPTT_HOPS_FOLD", env)
        r = _module_run(hops, N, T, H2, 6, True)
        assert r["mem"].rows_hops_fold == (env == "1")
        ran = [k for k in r["names"] if NEW in k]
        assert ran and all(("k_bptt_hops_graph_fold" in k) == (env == "1") for k in ran), ran
        runs.append(r)
    _check_vs_oracle(runs, N)
