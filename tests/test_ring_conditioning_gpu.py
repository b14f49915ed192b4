"""The column-write cached step (csrc/rows_colcache.hip: DenseEdge, TemporalBackedge "backward" / "both") under
outlier observations.  The step keeps one layer-1 aggregate per stored node and corrects it in place - `+ x[cur]`,
and past graph_size steps `- x[dropped]` (the ring form) - where the reference sums afresh.  One observation of
+-2^12 among U(-0.5, 0.5) ones is what tells the two apart: an aggregate that held it in fp32 has rounded away
~eps x 2^12 of its small terms, and the subtraction leaves that behind for up to N steps.  So the bounds here are per
regime: the beliefs of the QUIET steps (no outlier in the window) against 3 x the fp32 oracle's own distance from
float64 over those steps, the loss weighted on those steps only - tests/test_ring_conditioning_cpu.py shows from
references alone that an fp32 ring misses these bounds by two orders of magnitude and that the kernel's form (float64
aggregates) holds them.  Needs an MI355X."""
import functools

import pytest
import torch

from _golden import fp64_regime_bounds
from _ring_restate import CASES, _sel, make_inputs, make_modules
from test_dense_gpu import DEV
from test_rows_gpu import _mk

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The oracle in fp32 and float64 on the case's inputs, once per case -> the inputs, the final fp32 state, the
    gradient bounds, the float64 beliefs, the quiet-step bound and the global one (fp64_rollout_bounds' rule)."""
    spec, B, N, F, H1, H2, T, steps = CASES[name]
    obs, quiet, w = make_inputs(name)
    ref = make_modules(name)
    out32, hid32, bounds, (out64, atol_quiet) = fp64_regime_bounds(ref, obs, None, w, lambda: _sel(spec), N, quiet)
    atol_all = max(2e-6, 3.0 * float((out32.double() - out64).abs().max()))
    return obs, quiet, w, hid32, bounds, out64, atol_quiet, atol_all, ref


def _run(name, donate, col_steps, col_cache=True, rollout=False):
    spec, B, N, F, H1, H2, T, steps = CASES[name]
    obs, quiet, w, hid32, bounds, out64, atol_quiet, atol_all, ref = _reference(name)
    # the module as tests/test_rows_gpu.py::_mk builds it, with the oracle's weights
    _, g, mem, _ = _mk(B, N, F, H1, H2, ("dense", None, None) if spec[0] == "dense" else spec, donate)
    g.load_state_dict(ref.state_dict())
    mem.rows_col_cache = col_cache
    obs_d = obs.to(DEV)
    if rollout:
        out, hid = mem.rollout(obs_d)
    else:
        hid, outs = None, []
        for t in range(T):
            mx, hid = mem(obs_d[t], hid)
            outs.append(mx)
        out = torch.stack(outs)
        assert mem.rows_steps() == T
        assert mem.rows_col_steps_taken() == col_steps
    (out * w.to(DEV)).sum().backward()
    mem.check_flags()
    assert torch.equal(hid[0].cpu(), hid32[0]) and torch.equal(hid[1].cpu(), hid32[1])      # the state: bit exact
    assert torch.equal(hid[3].cpu(), hid32[3])
    err = (out.detach().cpu().double() - out64).abs()
    e_quiet, e_rest = float(err[quiet].max()), float(err[~quiet].max())
    print(f"{name} donate={donate}: quiet steps {e_quiet:.3g} = {e_quiet / atol_quiet:.2f} x bound {atol_quiet:.3g}, "
          f"the others {e_rest:.3g} = {e_rest / atol_all:.2f} x bound {atol_all:.3g}")
    assert e_quiet <= atol_quiet, (e_quiet, atol_quiet, e_quiet / atol_quiet)
    assert e_rest <= atol_all, (e_rest, atol_all)
    for k, p in g.named_parameters():
        g64, atol = bounds[k]
        ge = float((p.grad.cpu().double() - g64).abs().max())
        assert ge <= atol, (k, ge, atol, ge / atol if atol else None)
    return mem


# k_step_colcache8 with one and with two layer-2 tiles, k_step_colcache<64, 32> and <32, 64>; N = 8: one tile, 36: past
# the 16-slot and 32-slot tile edges, 68 (the first widths, donated): past the 64-bit word of the row masks
SWEEP = [(n, d) for n in CASES if n.startswith("dense-N8-") or n.startswith("dense-N36-") for d in (True, False)]
SWEEP.append(("dense-N68-32-32-16", True))


@pytest.mark.parametrize("name,donate", SWEEP)
def test_dense_edge_ring_under_outliers(name, donate):
    """DenseEdge: every stored row gains the new node and loses the dropped one at every step of the ring form."""
    _run(name, donate, col_steps=CASES[name][6])


def test_temporal_both_ring_under_outliers():
    """Hops [2, 7] in both directions at N = 8: rows d + 2 and d + 7 lose the dropped node d, and both are read again
    as sources of later rows (row d + 7 at the very next step, by hop 2) before they go themselves; the fp32 ring
    misses the quiet-step bound 36-fold here (tests/test_ring_conditioning_cpu.py)."""
    _run("both-2-7-N8", True, col_steps=CASES["both-2-7-N8"][6])


def test_temporal_backward_control():
    """Backward hops only: rows gain sources and never lose one - nothing is subtracted."""
    _run("backward-1-3-N8", True, col_steps=CASES["backward-1-3-N8"][6])


def test_temporal_forward_control():
    """Forward hops: the cached step of rows_cached.hip and its own ring - rows are final once written."""
    mem = _run("forward-1-2-4-N12", True, col_steps=0)
    assert mem.rows_cached_steps_taken() == CASES["forward-1-2-4-N12"][6]


def test_general_kernel_control():
    """The same DenseEdge inputs with the form switched off: the general live-row kernel re-aggregates every row."""
    _run("dense-N8-32-32-16", True, col_steps=0, col_cache=False)


def test_rollout_control():
    """... and through mem.rollout(obs), which sums afresh."""
    _run("dense-N8-32-32-16", False, col_steps=0, rollout=True)
