"""What makes tests/test_freeze_conv_gpu.py and tests/test_freeze_memory_gpu.py sensitive, from the references alone
(tests/_freeze.py).  No GPU.

  * Every gradient those tests hold a kernel to is >= SENSITIVITY (tests/_forms.py: 100) x its own atol in size: a
    kernel that left the buffer at zero - an early return one line too high, a shared intermediate computed only under
    another request - cannot pass.  The only exceptions are gradients that are zero analytically
    (_freeze.ANALYTIC_ZERO), asserted to BE zero in float64.
  * Every subset gradient of the float64 restatement equals the full run's entry bit for bit and every tensor outside
    the subset has none: the helper's flag handling does what the GPU test relies on.
  * The input families' own conditions on the new shapes: no near tie in the weighted sparse max, no PNA family
    violation, the EuclideanEdge(learned=True) decisions away from the threshold."""
import pytest
import torch

import _forms as F
import _freeze as Z
import _sparse_forms as S

CASE_IDS = [Z.layer_id(*c) for c in Z.CASES]


def _zero_analytically(owner, name):
    return name in Z.ANALYTIC_ZERO.get(owner, ())


def _assert_sensitive(tag, owner, pairs):
    """pairs {name: (float64 gradient, atol)}."""
    scale = max(float(g.abs().max()) for g, _ in pairs.values())
    assert scale > 0, tag
    report = []
    for name, (g64, atol) in pairs.items():
        size = float(g64.abs().max())
        if _zero_analytically(owner, name):
            assert size <= 1e-9 * scale, (tag, name, "listed as analytically zero", size, scale)
            continue
        report.append((size / atol, name))
        assert size >= F.SENSITIVITY * atol, (tag, name, "gradient too small to tell a zeroed buffer", size, atol)
    print("\nFREEZE-PRE %s: smallest |gradient| / atol %.0f (%s)" % ((tag,) + min(report)))


# ---------------------------------------------------------------------------
# the helper
# ---------------------------------------------------------------------------
def test_subsets_are_exhaustive_up_to_six_tensors():
    names = ["x", "adj", "a.weight", "a.bias", "b.weight", "b.bias"]
    got = Z.subsets(names)
    assert len(got) == len(set(got)) == 64 and got[0] == tuple(names) and () in got
    assert all(list(s) == [n for n in names if n in s] for s in got)
    assert len(Z.subsets(names[:1])) == 2


def test_subsets_beyond_six_tensors():
    names = ["x", "edge_weight", "a.weight", "a.bias", "b.weight", "b.bias", "rnn.bias_ih", "eps"]
    got = set(Z.subsets(names))
    params = tuple(names[2:])
    assert Z.subsets(names)[0] == tuple(names) and () in got
    for n in names:
        assert (n,) in got and tuple(m for m in names if m != n) in got
    assert ("x",) in got and ("edge_weight",) in got and params in got
    assert ("a.bias", "b.bias", "rnn.bias_ih") in got and ("a.weight", "b.weight", "eps") in got
    assert len(got) == 2 + 2 * len(names) + 3


def test_apply_sets_the_flags_on_module_and_inputs():
    lin = torch.nn.Linear(3, 2)
    x, idx = torch.randn(4, 3), torch.arange(4)
    out = Z.apply(("weight",), lin, {"x": x, "edge_index": idx})
    assert lin.weight.requires_grad and not lin.bias.requires_grad
    assert not out["x"].requires_grad and out["x"] is not x and out["edge_index"] is idx
    out = Z.apply(("x", "bias"), lin, {"x": x})
    assert out["x"].requires_grad and out["x"].is_leaf and lin.bias.requires_grad and not lin.weight.requires_grad
    with pytest.raises(AssertionError):
        Z.apply(("adj",), lin, {"x": x})


def test_layer_table_covers_every_family_in_both_forms():
    assert len(Z.LAYERS) == 24 and len(Z.CASES) == 48
    assert {f for f, _ in Z.LAYERS} == {"GraphConv-add", "GraphConv-mean", "GraphConv-max", "SAGEConv", "GCNConv",
                                        "GINConv", "GATConv", "TransformerConv", "ResGatedGraphConv", "GatedGraphConv",
                                        "TAGConv", "PNAConv"}
    for family, dense, i in Z.CASES:
        s = Z.spec(family, dense, i)
        lead = tuple(s.inputs["x"].shape[:-1])
        assert lead == (Z.DENSE_SHAPES[i][:2] if dense else Z.SPARSE_SHAPES[i][:1])
        if not dense:       # random_edges adds two duplicate loops, a loop and a duplicate edge
            assert s.const["edge_index"].shape[1] == Z.SPARSE_SHAPES[i][1] + 5
    for family in ("GINConv",):
        assert "eps" in Z.spec(family, True, 0).names                      # train_eps
    assert "lin_beta.weight" in Z.spec("TransformerConv", False, 1).names   # beta


# ---------------------------------------------------------------------------
# the conv layers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("family,dense,i", Z.CASES, ids=CASE_IDS)
def test_conv_gradients_are_large_against_their_atol(family, dense, i):
    s = Z.spec(family, dense, i)
    full = Z.reference(family, dense, i, tuple(s.names))
    g64, g32 = full[torch.float64][1], full[torch.float32][1]
    for name in s.names:
        assert g64[name] is not None and g32[name] is not None, (name, "the restatement gives it no gradient")
    _assert_sensitive(Z.layer_id(family, dense, i), family, {n: (g64[n], Z.bound(g64[n], g32[n])) for n in s.names})
    if getattr(s, "max_margin", None) is not None:      # weighted sparse max: no two candidates within 1e-5
        assert int((s.max_margin < 1e-5).sum()) == 0
    if hasattr(s, "violations"):                        # PNA: the dyadic / generic family conditions
        assert s.violations == 0


@pytest.mark.parametrize("family,dense,i", Z.CASES, ids=CASE_IDS)
def test_conv_subset_gradients_equal_the_full_run(family, dense, i):
    s = Z.spec(family, dense, i)
    picks = Z.subsets(s.names)
    assert len(picks) == (2 ** len(s.names) if len(s.names) <= Z.EXHAUSTIVE_UP_TO else len(set(picks)))
    out_full, g_full = Z.reference(family, dense, i, picks[0])[torch.float64]
    for subset in picks[1:]:
        out, grads = Z.reference(family, dense, i, subset)[torch.float64]
        assert torch.equal(out, out_full), subset
        for name in s.names:
            if name in subset:
                assert grads[name] is not None and torch.equal(grads[name], g_full[name]), (subset, name)
            else:
                assert grads[name] is None, (subset, name)


# ---------------------------------------------------------------------------
# the memories
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case,form", Z.DENSE_MEMORY, ids=["%s-%s" % (c, F.form_id(f)) for c, f in Z.DENSE_MEMORY])
def test_dense_memory_gradients_are_large_against_their_atol(case, form):
    """On the trajectory with an observation gradient: every parameter and "obs"."""
    t = F.trajectory(case, form, obs_grad=True)
    F.assert_preconditions(t.pre)
    assert "obs" in t.bounds
    _assert_sensitive("%s %s" % (case, F.form_id(form)), case, t.bounds)
    names = [k for k in t.bounds if k != "obs"]
    plain = F.trajectory(case, form)
    assert set(plain.bounds) - {"obs"} == set(names)
    for k in names:       # (asking for the observations' gradient changes no other)
        assert torch.equal(plain.bounds[k][0], t.bounds[k][0])
    pats = Z.memory_patterns(names, bool(F.CASES[case].get("obs_grad")))
    assert {"layer1_frozen", "layer2_frozen", "biases_only", "weights_only", "all_frozen", "gnn_frozen_obs_grad",
            "grad_obs", "grad_layer2", "grad_bias"} <= set(pats)
    assert ("net_frozen" in pats) == (case == "learned") and ("pre_frozen" in pats) == (case == "fold")
    l1, l2 = Z.gnn_layers(names)
    assert len(l1) == len(l2) + (0 if form[2] == 3 else 1) == 3
    for p, (trainable, obs_grad, asked) in pats.items():
        assert set(trainable) <= set(names) and (asked is None or (asked and set(asked) <= set(names) | {"obs"})), p
    assert pats["biases_only"][0] and set(pats["biases_only"][0]) | set(pats["weights_only"][0]) == set(names)


def test_euclid_learned_trajectory_is_the_plain_one():
    """Dividing by dist_param = max_distance and thresholding at 1 selects the edges of the plain case, away from the
    threshold; the oracle gives dist_param no gradient."""
    t, plain = Z.euclid_learned_trajectory(obs_grad=True), F.trajectory("euclid", Z.RELU3, obs_grad=True)
    assert t.margin >= F.DECISION_MARGIN
    assert all(g is None for g in t.dist_param_grads)
    assert torch.equal(t.hidden[1], plain.hidden[1]) and torch.equal(t.hidden[0], plain.hidden[0])
    _assert_sensitive("euclid learned", "euclid", t.bounds)


@pytest.mark.parametrize("case,form", Z.SPARSE_MEMORY, ids=["%s-%s" % (c, S.form_id(f)) for c, f in Z.SPARSE_MEMORY])
def test_sparse_memory_gradients_are_large_against_their_atol(case, form):
    t = S.trajectory(case, form)
    S.assert_preconditions(t.pre)
    assert bool(S.CASES[case].get("x_grad")) == ("x0" in t.bounds)
    _assert_sensitive("sparse %s %s" % (case, S.form_id(form)), case, t.bounds)
