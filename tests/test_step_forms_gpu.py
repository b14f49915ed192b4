"""The fused DenseGCM step kernels in every activation / bias form: act1 / act2 in {none, tanh, relu} and has_bias bits 1
and 2 are run-time arguments of the kernels, and which kernel runs depends on them (the lean cached step takes tanh / tanh
only, the column-write step has an epilogue per activation, a missing bias leaves the one-node pack_params path, the
folded preprocessor writes W_root1 b_p into the layer-1 bias slot whether or not the layer has a bias).  11 forms on the
smallest shapes that reach each kernel family (tests/_forms.py), every driver of a (case, form) against ONE cached
oracle trajectory: state bit equal to the float32 oracle, beliefs and every gradient inside the float64 bounds of
tests/_golden.fp64_rollout_bounds, the path counters of the kernels that must have run.  The seeds are chosen so that
no ReLU pre-activation sits within 10 x the oracle's float32 error of zero and every wrong form would be seen
(tests/test_step_forms_cpu.py asserts the same without a GPU).  Needs an MI355X.

Worst error / atol measured on an MI355X: see DESIGN.md section 4, "Forms"."""
import pytest
import torch

import _forms as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

DRIVERS = ["steps", "steps_donated", "rollout", "layered"]
PARAMS = [(case, form, d) for case, form in F.pairs() for d in DRIVERS]
# the cached step that is NOT the lean one (k_step_rows_cached_img4b) on the forms the lean one takes
PARAMS += [("temporal", form, "not_lean") for form in F.FORMS if form[:2] == ("tanh", "tanh")]
# the donated loop + backward captured once and replayed twice: the no-bias host path (torch.cat over zero slots)
# and the one-node pack_params path under capture
PARAMS += [("temporal", form, "captured") for form in (("tanh", "tanh", 0), ("relu", "relu", 3))]
DONATED = ("steps_donated", "not_lean", "captured")


def _build(t, driver):
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.temporal import TemporalBackedge
    from gcm.edge_selectors.dense import DenseEdge
    from gcm.edge_selectors.distance import EuclideanEdge
    from gcm.edge_selectors.learned import LearnedEdge
    DenseGCM.did_warn = True        # (the one-time overflow notice)
    c = F.CASES[t.case]
    B, N, Fin, H1, H2, T = t.shape
    g = F.build_gnn(c.get("pre", Fin), H1, H2, t.form, G.DenseGraphConv, G.Sequential)
    g.load_state_dict(t.inp.gnn)
    g = g.to(DEV)
    named = dict(g.named_parameters())
    for conv, bit in zip(F.convs_of(g), (1, 2)):       # a missing bias: no tensor, so no gradient - as on the oracle
        assert (conv.lin_rel.bias is None) == (not t.form[2] & bit)
    pre = None
    if t.inp.pre is not None:
        pre = torch.nn.Linear(Fin, c["pre"], bias=True)
        pre.load_state_dict(t.inp.pre)
        pre = pre.to(DEV)
        named.update({"pre." + k: p for k, p in pre.named_parameters()})
    kind = c["sel"]
    if kind[0] == "temporal":
        sel = TemporalBackedge(kind[1], direction=kind[2])
    elif kind[0] == "dense":
        sel = DenseEdge()
    elif kind[0] == "euclid":
        sel = EuclideanEdge(kind[1])
    else:
        sel = LearnedEdge(Fin, num_edge_samples=kind[1])
        sel.edge_network.load_state_dict(t.inp.net)
        sel = sel.to(DEV)
        named.update({"net." + k: p for k, p in sel.edge_network.named_parameters()})
    mem = DenseGCM(g, preprocessor=pre, edge_selectors=sel, graph_size=N, donate_state=driver in DONATED,
                   fused=driver != "layered")
    if driver == "not_lean":
        mem.rows_lean_step = False
    assert set(named) == set(t.bounds) - {"obs"}
    return mem, named


def _loop(mem, x, hidden=None):
    outs = []
    for i in range(x.shape[0]):
        mx, hidden = mem(x[i], hidden)
        outs.append(mx)
    return torch.stack(outs), hidden


def _assert_path(mem, t, driver):
    """Which kernels ran - the expectations of test_training_gpu._assert_path, test_rows_path_matches_reference,
    test_folded_step_matches_reference and test_learned_chain_steady_state_one_launch_vs_oracle for a chain from empty
    graphs."""
    B, N, Fin, H1, H2, T = t.shape
    case = t.case
    if driver == "layered":
        assert mem.rows_steps() == 0 and mem._cfg_last is None, "fused=False took a fused kernel"
        return
    cfg = mem._cfg_last[3] if mem._cfg_last else None
    assert cfg is not None, "the fused kernels were not taken"
    if driver == "rollout":      # (one C call or the module's own donated loop: the per-chain counters are gone by now)
        assert (cfg.learned_sel is not None) == (case == "learned") and (cfg.fold is not None) == (case == "fold")
        return
    donate = driver in DONATED
    if case == "learned":
        assert cfg.learned_sel is not None
        assert mem.learned_steady_steps_taken() == (T - N if donate else 0)
        return
    if case == "ragged":          # N, F no multiples of 4: the round-1 fused step, not the live-row kernels
        assert mem.rows_steps() == 0
        return
    runs = 3 if driver == "captured" else 1       # (two warm-up iterations ahead of the capture)
    assert mem.rows_steps() == runs * T, "the live-row path was not taken"
    cached, rolled, col = mem.rows_cached_steps_taken(), mem.rows_rolled_steps_taken(), mem.rows_col_steps_taken()
    if case in ("dense8", "both4"):          # (the column-write form takes a functional state too)
        assert (cached, rolled, col) == (0, 0, T)
    elif case == "fold":
        assert cfg.fold is not None and cfg.rows_ok and (cached, rolled, col) == (0, 0, 0)
    elif not donate:                         # (the cached forms of forward hops / EuclideanEdge: donated state only)
        assert (cached, rolled, col) == (0, 0, 0)
    elif case == "euclid":
        assert (cached, rolled, col) == (T, T - N, 0)
    elif case == "obs_grad":                 # (observation gradients: the rolling regime goes to the general kernel)
        assert (cached, rolled, col) == (N, 0, 0)
    else:                                    # steady-state form: F, H1 in (32, 64) and N > 2 max(hops)
        steady = case in ("temporal", "wide")
        assert (cached, rolled, col) == ((T, T - N, 0) if steady else (N, 0, 0))


def _check(t, tag, out, hidden, named, x):
    want = t.hidden
    assert torch.equal(hidden[1].detach().cpu(), want[1]), "adjacency must be bit exact"
    assert torch.equal(hidden[3].cpu(), want[3])
    assert torch.equal(hidden[0].detach().cpu(), want[0])
    worst = {"belief": float((out.detach().cpu().double() - t.out64).abs().max()) / t.out_atol}
    bad = [] if worst["belief"] <= 1.0 else [("belief", worst["belief"])]
    worst["grad"], where = 0.0, None
    for k, (g64, atol) in t.bounds.items():
        got = x.grad if k == "obs" else named[k].grad
        assert got is not None, (tag, k, "no gradient")
        ratio = float((got.detach().cpu().double() - g64).abs().max()) / atol
        if ratio > worst["grad"]:
            worst["grad"], where = ratio, k
        if not ratio <= 1.0:
            bad.append((k, ratio))
    print("\nFORMS %s: worst error/atol belief %.3f grad %.3f (%s)" % (tag, worst["belief"], worst["grad"], where))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("case,form,driver", PARAMS, ids=["%s-%s-%s" % (c, F.form_id(f), d) for c, f, d in PARAMS])
def test_step_forms_vs_oracle(case, form, driver):
    """Drivers: the per-step loop on a functional (`steps`) and on a donated state, rollout(), DenseGCM(fused=False)
    (`layered`: graphconv.hip / fused_layer.hip with the activation in their epilogue), the donated loop with
    rows_lean_step = False, and the donated loop + backward captured once and replayed twice."""
    t = F.trajectory(case, form)
    F.assert_preconditions(t.pre)            # before the device is touched
    B, N, Fin, H1, H2, T = t.shape
    mem, named = _build(t, driver)
    tag = "%s %s %s" % (case, F.form_id(form), driver)
    x = t.inp.obs.to(DEV).requires_grad_(bool(F.CASES[case].get("obs_grad")))
    w = t.inp.w.to(DEV)
    if case == "learned":        # the recorded gumbel draws, one [B, N] tensor per step in step order
        noise, calls = t.inp.noise.to(DEV), [0]

        def draws(like):
            calls[0] += 1
            return noise[calls[0] - 1]
        mem.edge_selectors.noise_fn = draws
    if driver == "captured":
        def iteration():
            out, hidden = _loop(mem, x)
            (out * w).sum().backward()
            return out, hidden
        for _ in range(2):       # (the recipe of test_training_gpu._captured: warm-up on a side stream)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for p in named.values():
                    p.grad = None
                iteration()
            torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        for p in named.values():
            p.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, hidden = iteration()
        _assert_path(mem, t, driver)
        for replay in range(2):
            for p in named.values():
                p.grad.zero_()
            graph.replay()
            torch.cuda.synchronize()
            mem.check_flags()
            _check(t, "%s replay %d" % (tag, replay), out, hidden, named, x)
        return
    out, hidden = mem.rollout(x) if driver == "rollout" else _loop(mem, x)
    _assert_path(mem, t, driver)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    mem.check_flags()
    if case == "learned":
        assert calls[0] == T
    _check(t, tag, out, hidden, named, x)
