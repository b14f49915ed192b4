"""What the outlier cases of tests/test_ring_conditioning_gpu.py can tell apart, from references alone: the
column-write cached step restated with its aggregates kept in fp32 (tests/_ring_restate.py, wide = False) must MISS
the per-regime float64 bounds clearly, the form the kernel uses (wide = True: float64 aggregates) must hold them, and
with the outliers taken out both must - so a GPU failure in those cases is the kernel's conditioning, not the bound or
the restatement.  No GPU needed."""
import functools

import pytest
import torch

from _golden import fp64_regime_bounds
from _ring_restate import CASES, OUTLIER, _sel, make_inputs, make_modules, ring_rollout

RING_CASES = [k for k in CASES if not k.startswith("forward")]      # (the forward control runs rows_cached.hip's ring)


@functools.lru_cache(maxsize=None)
def _ratios(name, outlier):
    """-> {form: (belief error on the quiet steps / its bound, {param: gradient error / its bound})}, the bounds,
    the quiet mask and the float64 beliefs."""
    spec, B, N, F, H1, H2, T, steps = CASES[name]
    obs, quiet, w = make_inputs(name, outlier)
    ref = make_modules(name)
    out32, _, bounds, (out64, out_atol) = fp64_regime_bounds(ref, obs, None, w, lambda: _sel(spec), N, quiet)
    res = {}
    for form, wide in (("fp32 ring", False), ("wide ring", True)):
        ref.zero_grad(set_to_none=True)
        out = ring_rollout(ref, obs, N, spec, wide)
        (out * w).sum().backward()
        err = float((out.detach().double() - out64)[quiet].abs().max())
        gr = {}
        for k, p in ref.named_parameters():
            g64, atol = bounds[k]
            ge = float((p.grad.double() - g64).abs().max())
            # (a parameter the beliefs do not depend on - lin_rel2's weight without forward hops: zero, bound zero)
            gr[k] = ge / atol if atol > 0 else (0.0 if ge == 0 else float("inf"))
        res[form] = (err / out_atol, gr, err)
    return res, out_atol, quiet, out64


@pytest.mark.parametrize("name", list(CASES))
def test_case_conditions(name):
    """The cases can show the residue: quiet steps are at least half of T; behind every outlier's window come quiet
    steps during which rows that held it are still stored; the float64 beliefs there are not saturated."""
    spec, B, N, F, H1, H2, T, steps = CASES[name]
    obs, quiet, w = make_inputs(name)
    assert int(quiet.sum()) * 2 >= T
    assert float(obs[list(steps)].abs().max()) == OUTLIER and float(obs[quiet].abs().max()) <= 0.5
    for s in steps:
        # rows made at steps s .. s + N - 1 held the outlier; the last of them is stored up to step s + 2 N - 2.
        # N quiet steps behind the window - all of them while such a row is stored, but for the last - or, where the
        # rollout ends sooner, every step that is left: the N = 68 case ends at T = 3 N + 8 with its outlier at N + 12,
        # 64 steps behind the window instead of 68.
        n_after = min(N, T - (s + N))
        assert n_after == (N if N != 68 else N - 4), (s, n_after)
        assert bool(quiet[s + N:s + N + n_after].all())
    assert bool((w[~quiet] == 0).all()) and bool((w[quiet] > 0).any())
    if name in RING_CASES:
        _, _, _, out64 = _ratios(name, OUTLIER)
        a = out64[quiet].abs()
        if N == 8:
            assert float(a.median()) < 0.99
        else:
            # DenseEdge with default-initialised layers: layer 2 adds N near-equal rows (every stored row has the same
            # aggregate), so from N = 36 on most beliefs of a full graph sit at +-1 (median 1 - 1e-6) whatever the
            # seed (test_unsaturated_share_does_not_hang_on_the_seed).  The bounds are maxima: what they need is
            # beliefs left that can move - here 18 % .. 27 % of the quiet-step beliefs are below 0.99; one in ten is
            # asked for.  That these carry the residue is what test_fp32_ring_fails_and_wide_ring_holds shows for
            # the same cases.
            assert float((a < 0.99).float().mean()) >= 0.1


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", [k for k in CASES if k.startswith("dense") and CASES[k][2] >= 36])
def test_unsaturated_share_does_not_hang_on_the_seed(name, seed):
    """Other initial weights and other observations for the DenseEdge cases with N >= 36: the float64 oracle's
    quiet-step beliefs are mostly saturated there as well (median above 0.99 - the condition of the N = 8 cases cannot
    hold at these sizes with default-initialised layers), and again at least one in ten is not."""
    import copy
    from oracle import dense as od
    spec, B, N, F, H1, H2, T, steps = CASES[name]
    obs, quiet, _ = make_inputs(name, seed=seed)
    ref64 = copy.deepcopy(make_modules(name, seed=seed)).double()
    with torch.no_grad():
        out64, _ = od.dense_rollout(obs.double(), None, ref64, graph_size=N, edge_selectors=_sel(spec))
    a = out64[quiet].abs()
    share = float((a < 0.99).float().mean())
    print(f"{name} seed {seed}: median |belief| {float(a.median()):.6f}, {100 * share:.0f} % below 0.99")
    assert float(a.median()) >= 0.99 and share >= 0.1


@pytest.mark.parametrize("name", RING_CASES)
def test_fp32_ring_fails_and_wide_ring_holds(name):
    spec, B, N, F, H1, H2, T, steps = CASES[name]
    res, out_atol, quiet, _ = _ratios(name, OUTLIER)
    for form in res:
        r, gr, err = res[form]
        print(f"{name:22s} {form}: quiet-step belief error {err:.2e} = {r:7.2f} x bound {out_atol:.2e}; "
              f"gradients {min(gr.values()):7.2f} .. {max(gr.values()):7.2f} x their bounds")
    r, gr, _ = res["wide ring"]
    assert r <= 1.0 and max(gr.values()) <= 1.0, (r, gr)
    r, gr, _ = res["fp32 ring"]
    if spec[0] == "dense":
        assert r >= 10.0 and min(gr.values()) >= 10.0, (r, gr)
    elif spec[2] == "both":
        assert r >= 10.0, r
    # ("backward": no row ever loses a source - nothing is subtracted, the control of the GPU test)


@pytest.mark.parametrize("name", RING_CASES)
def test_without_outliers_both_forms_hold(name):
    """The same draws with the outlier steps left as they were: the restatement itself sits inside the bounds."""
    res, out_atol, _, _ = _ratios(name, 0.0)
    for form, (r, gr, err) in res.items():
        print(f"{name:22s} {form}, no outlier: {r:5.2f} x bound {out_atol:.2e}; "
              f"gradients up to {max(gr.values()):5.2f} x")
        assert r <= 1.0 and max(gr.values()) <= 1.0, (form, r, gr)
