"""DenseGCM and SparseGCM under frozen parameters and partial gradient requests.  The memories add host logic keyed
on `packed.requires_grad()` - pack_params, the parameter gate, RowsFast::arm, the need_bwd switches of
csrc/torch_ext/step_ext.cpp, _packed_params / _gate in gcm/gcm.py - and forward() chooses its path from the
observations' flag: a frozen layer, bias-only fine-tuning and a frozen memory behind a trainable encoder all go through
code that a run with everything trainable never reaches.

The cases, seeds, oracle trajectories and bounds are those of tests/_forms.py / tests/_sparse_forms.py (freezing a
tensor does not change the others' gradients, so `trajectory(...).bounds` holds the float64 gradient and atol of every
tensor), the drivers those of tests/test_step_forms_gpu.py / test_sparse_forms_gpu.py.  Patterns
(tests/_freeze.memory_patterns): flags set BEFORE the forward - layer1_frozen, layer2_frozen, biases_only,
weights_only, all_frozen, gnn_frozen_obs_grad (every parameter frozen, the observations take a gradient: the beliefs
must still have a grad_fn), the edge network / preprocessor frozen with the GNN trained and the reverse - and, with
everything trainable, torch.autograd.grad for {obs}, layer 2's tensors and one bias (the C++ nodes'
task_should_compute_output).  Asserted: the state bit equal to the float32 oracle, the beliefs and every trainable
gradient inside the float64 bounds, .grad None on everything frozen, check_flags(), and - while a GNN parameter stays
trainable and no observation gradient is added - the kernels of the unfrozen run (a freeze must not knock the chain off
them).  tests/test_freeze_cpu.py asserts that each of these gradients is >= 100x its atol.  Needs an MI355X."""
import pytest
import torch

import _forms as F
import _freeze as Z
import _sparse_forms as S
import test_sparse_forms_gpu as TSS
import test_step_forms_gpu as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _set_flags(named, trainable):
    for k, p in named.items():
        p.requires_grad_(k in trainable)
        p.grad = None


def _grads(tag, named, xs, trainable, obs_grad, asked, loss, no_gradient=()):
    """Runs the backward the pattern asks for -> {name: gradient} over what must have one, after asserting that nothing
    else got one.  xs: {bound name: observation tensor}; no_gradient: trainable tensors that nothing differentiable
    reads (.grad stays None)."""
    tensors = dict(named)
    tensors.update(xs)
    if asked is None:
        loss.backward()
        want = [k for k in named if k in trainable and k not in no_gradient] + (list(xs) if obs_grad else [])
        got = {k: tensors[k].grad for k in want}
    else:
        keys = [k for k in asked if k != "obs"] + (list(xs) if "obs" in asked else [])
        got = dict(zip(keys, torch.autograd.grad(loss, [tensors[k] for k in keys])))
    torch.cuda.synchronize()
    for k, v in tensors.items():
        if k not in got or asked is not None:
            assert v.grad is None, (tag, k, "has no request and got a gradient")
    for k, g in got.items():
        assert g is not None, (tag, k, "no gradient")
    return got


def _held(tag, t, got):
    bad, worst = [], (0.0, None)
    for k, g in got.items():
        g64, atol = t.bounds[k]
        ratio = float((g.detach().cpu().double() - g64).abs().max()) / atol
        if ratio > worst[0]:
            worst = (ratio, k)
        if not ratio <= 1.0:
            bad.append((k, ratio))
    print("\nFREEZE %s: %d gradients, worst error/atol %.3f (%s)" % (tag, len(got), worst[0], worst[1]))
    assert not bad, (tag, bad)


# ---------------------------------------------------------------------------
# DenseGCM
# ---------------------------------------------------------------------------
def _dense_params():
    out = []
    for case, form in Z.DENSE_MEMORY:
        # (the pattern list depends on the names' prefixes alone)
        probe = ["module_0.w", "module_2.w"] + {"fold": ["pre.w"], "learned": ["net.w"]}.get(case, [])
        for pattern in Z.memory_patterns(probe, bool(F.CASES[case].get("obs_grad"))):
            for driver in TS.DRIVERS:
                out.append((case, form, pattern, driver))
    return out


DENSE = _dense_params()


def _dense_state_and_beliefs(t, out, hidden):
    want = t.hidden
    assert torch.equal(hidden[1].detach().cpu(), want[1]), "adjacency must be bit exact"
    assert torch.equal(hidden[3].cpu(), want[3])
    assert torch.equal(hidden[0].detach().cpu(), want[0])
    ratio = float((out.detach().cpu().double() - t.out64).abs().max()) / t.out_atol
    assert ratio <= 1.0, ("belief", ratio)


def _run_dense(t, case, pattern, driver, build, no_gradient=()):
    has_og = bool(F.CASES.get(case, {}).get("obs_grad"))
    B, N, Fin, H1, H2, T = t.shape
    mem, named = build()
    names = list(named)
    trainable, obs_grad, asked = Z.memory_patterns(names, has_og)[pattern]
    tag = "%s %s %s %s" % (case, F.form_id(t.form), pattern, driver)
    _set_flags(named, set(trainable))
    x = t.inp.obs.to(DEV).requires_grad_(obs_grad)
    w = t.inp.w.to(DEV)
    calls = [0]
    if t.inp.noise is not None:          # the recorded gumbel draws, one [B, N] tensor per step in step order
        noise = t.inp.noise.to(DEV)

        def draws(like):
            calls[0] += 1
            return noise[calls[0] - 1]
        mem.edge_selectors.noise_fn = draws
    out, hidden = mem.rollout(x) if driver == "rollout" else TS._loop(mem, x)
    if case in F.CASES and Z.keeps_the_path(pattern, (trainable, obs_grad, asked), names, has_og):
        TS._assert_path(mem, t, driver)
    if not (set(trainable) - set(no_gradient)) and not obs_grad:
        assert not out.requires_grad and out.grad_fn is None, (tag, "beliefs of a frozen memory carry a graph")
        got = {}
    else:
        assert out.grad_fn is not None, (tag, "the beliefs have no grad_fn: nothing behind the memory would learn")
        got = _grads(tag, named, {"obs": x}, set(trainable), obs_grad, asked, (out * w).sum(), no_gradient)
    torch.cuda.synchronize()
    mem.check_flags()
    for k in no_gradient:
        assert named[k].grad is None, (tag, k)
    if t.inp.noise is not None:
        assert calls[0] == T
    _dense_state_and_beliefs(t, out, hidden)
    _held(tag, t, got)


@pytest.mark.parametrize("case,form,pattern,driver", DENSE,
                         ids=["%s-%s-%s-%s" % (c, F.form_id(f), p, d) for c, f, p, d in DENSE])
def test_dense_memory_under_partial_gradients(case, form, pattern, driver):
    og = pattern in ("gnn_frozen_obs_grad", "grad_obs") or None
    t = F.trajectory(case, form, obs_grad=og)
    F.assert_preconditions(t.pre)            # before the device is touched
    _run_dense(t, case, pattern, driver, lambda: TS._build(t, driver))


EUCLID = [(p, d) for p in ("sel_frozen", "gnn_frozen_sel_trained", "gnn_frozen_obs_grad") for d in TS.DRIVERS]


@pytest.mark.parametrize("pattern,driver", EUCLID, ids=["%s-%s" % pd for pd in EUCLID])
def test_euclidean_edge_learned_dist_param(pattern, driver):
    """EuclideanEdge(learned=True): dist_param divides the node matrix ahead of a threshold, a comparison - it has no
    gradient, on the oracle (asserted) or here.  Frozen with the GNN trained it changes nothing; trained with the GNN
    frozen nothing differentiable is trainable and the beliefs carry no graph; with everything frozen behind a
    trainable encoder the observations still get their gradient."""
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    from gcm.edge_selectors.distance import EuclideanEdge
    t = Z.euclid_learned_trajectory(obs_grad=pattern == "gnn_frozen_obs_grad")
    assert t.margin >= F.DECISION_MARGIN and all(g is None for g in t.dist_param_grads)
    B, N, Fin, H1, H2, T = t.shape

    def build():
        DenseGCM.did_warn = True        # (the one-time overflow notice)
        g = F.build_gnn(Fin, H1, H2, t.form, G.DenseGraphConv, G.Sequential)
        g.load_state_dict(t.inp.gnn)
        g = g.to(DEV)
        sel = EuclideanEdge(t.dist_param, learned=True).to(DEV)
        named = dict(g.named_parameters())
        named["sel.dist_param"] = sel.dist_param
        return DenseGCM(g, edge_selectors=sel, graph_size=N, donate_state=driver in TS.DONATED,
                        fused=driver != "layered"), named
    _run_dense(t, Z.EUCLID_LEARNED, pattern, driver, build, no_gradient=("sel.dist_param",))


# ---------------------------------------------------------------------------
# SparseGCM
# ---------------------------------------------------------------------------
def _sparse_drivers(case):
    return ["fast"] + (["layered"] if case in TSS.LAYERED else []) + (["general"] if case in TSS.GENERAL else [])


def _sparse_params():
    out = []
    for case, form in Z.SPARSE_MEMORY:
        x_grad = bool(S.CASES[case].get("x_grad"))
        probe = ["module_0.w", "module_2.w"] + (["net.w"] if "learned" in S.CASES[case] else [])
        for pattern in Z.memory_patterns(probe, x_grad, x_grad_possible=x_grad):
            for driver in _sparse_drivers(case):
                out.append((case, form, pattern, driver))
    return out


SPARSE = _sparse_params()


@pytest.mark.parametrize("case,form,pattern,driver", SPARSE,
                         ids=["%s-%s-%s-%s" % (c, S.form_id(f), p, d) for c, f, p, d in SPARSE])
def test_sparse_memory_under_partial_gradients(case, form, pattern, driver):
    t = S.trajectory(case, form)
    S.assert_preconditions(t.pre)            # before the device is touched
    c = S.CASES[case]
    x_grad = bool(c.get("x_grad"))
    mem, named = TSS._build(t, driver)
    names = list(named)
    trainable, obs_grad, asked = Z.memory_patterns(names, x_grad, x_grad_possible=x_grad)[pattern]
    tag = "sparse %s %s %s %s" % (case, S.form_id(form), pattern, driver)
    _set_flags(named, set(trainable))
    # (LearnedEdge's softmax temperature, tau_param, is a parameter too: it has no entry in `bounds` - the oracle's is a
    #  constant - and goes with the edge network, so that an all-frozen memory has nothing left to train)
    rest = [p for p in mem.parameters() if not any(p is q for q in named.values())]
    assert len(rest) == (1 if "learned" in c else 0)
    for p in rest:
        p.requires_grad_(any(k.startswith("net.") for k in trainable))
    xs = [x.to(DEV).requires_grad_(obs_grad) for x, _ in t.inp.calls]
    ws = [w.to(DEV) for w in t.inp.w]
    n_call = [0]
    if "learned" in c:        # the recorded gumbel draws, one per candidate pair in candidate order
        noise = [z.to(DEV) for z in t.inp.noise]

        def draws(logits):
            n_call[0] += 1
            assert logits.numel() == noise[n_call[0] - 1].numel()
            return noise[n_call[0] - 1]
        mem.edge_selectors.noise_fn = draws
    hidden, outs = None, []
    for x, (_, taus) in zip(xs, t.inp.calls):
        out, hidden = mem(x, taus.to(DEV), hidden)
        outs.append(out)
    if Z.keeps_the_path(pattern, (trainable, obs_grad, asked), names, x_grad):
        TSS._assert_path(mem, t, driver)
    if not trainable and not obs_grad:
        assert not any(o.requires_grad for o in outs), (tag, "beliefs of a frozen memory carry a graph")
        got = {}
    else:
        assert all(o.grad_fn is not None for o in outs if o.numel()), (tag, "beliefs without a grad_fn")
        loss = sum((o * w).sum() for o, w in zip(outs, ws))
        got = _grads(tag, named, {"x%d" % i: x for i, x in enumerate(xs)} if x_grad else {}, set(trainable),
                     obs_grad, asked, loss)
    torch.cuda.synchronize()
    mem._check_flags(mem._flag_word(xs[0].device))
    if "learned" in c:
        assert n_call[0] == len(t.inp.calls)
    TSS._check(t, tag, outs, hidden, named, xs, grads=False)      # (state bit exact, the beliefs of every call)
    _held(tag, t, got)
