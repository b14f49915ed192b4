"""The preconditions of tests/test_step_forms_gpu.py, from the oracle alone (tests/_forms.py): under the seed chosen for
every (case, form) the float64 pre-activations of every ReLU sit >= 10 x the oracle's own float32 error away from zero
with equal signs, every neighbouring wrong form moves the float64 beliefs >= 100 x their atol, and the EuclideanEdge /
LearnedEdge decisions are >= 1e-3 from flipping.  No GPU."""
import pytest

import _forms as F


def test_forms_cover_the_matrix():
    """Every activation pair; every bias mask on a non-tanh/tanh form; tanh/tanh (the lean kernel) with a bias missing;
    a seed for every (case, form)."""
    assert len(F.FORMS) == len(set(F.FORMS)) == 11
    assert {f[:2] for f in F.FORMS} == {(a, b) for a in F.ACTS for b in F.ACTS}
    assert {f[2] for f in F.FORMS if f[:2] != ("tanh", "tanh")} == {0, 1, 2, 3}
    assert {f[2] for f in F.FORMS if f[:2] == ("tanh", "tanh")} == {0, 1, 2}
    assert set(F.LEARNED_FORMS) == {("relu", "relu", 3), ("none", "tanh", 0), ("tanh", "none", 1), ("relu", "none", 2)}
    assert set(F.SEEDS) == {(case, F.form_id(form)) for case, form in F.pairs()}
    assert all(0 <= s < 32 for s in F.SEEDS.values())
    for c in F.CASES.values():          # T > N: the chain leaves its fill phase
        assert c["shape"][5] >= c["shape"][1] + 4


def test_wrong_forms_are_the_neighbours():
    w = F.wrong_forms(("tanh", "relu", 3), fold=True)
    assert w["swapped"] == (("relu", "tanh", 3), False)
    assert {k: v[0][:2] for k, v in w.items() if k.startswith("act")} == {
        "act1=none": ("none", "relu"), "act1=relu": ("relu", "relu"), "act2=none": ("tanh", "none"), "act2=tanh": ("tanh", "tanh")}
    assert w["no bias 1"] == (("tanh", "relu", 2), False) and w["no bias 2"] == (("tanh", "relu", 1), False)
    assert w["no W_root1 b_p"] == (("tanh", "relu", 3), True)
    assert "swapped" not in F.wrong_forms(("relu", "relu", 0)) and len(F.wrong_forms(("relu", "relu", 0))) == 4


@pytest.mark.parametrize("case,form", F.pairs(), ids=["%s-%s" % (c, F.form_id(f)) for c, f in F.pairs()])
def test_form_preconditions(case, form):
    p = F.preconditions(case, form, F.SEEDS[(case, F.form_id(form))])
    n_relu = sum(a == "relu" for a in form[:2])
    assert (p.n_pre > 0) == (n_relu > 0)
    if n_relu:         # every live row of every step, per ReLU layer: sum over t of B min(t + 1, N) rows
        B, N, _, H1, H2, T = F.CASES[case]["shape"]
        rows = B * sum(min(t + 1, N) for t in range(T))
        assert p.n_pre == rows * ((H1 if form[0] == "relu" else 0) + (H2 if form[1] == "relu" else 0))
    assert len(p.sens) == len(F.wrong_forms(form, fold=case == "fold")) >= 4
    print("\nFORMS-PRE %s %s seed %d: relu ratio %.1f over %d, sensitivity >= %.0f x atol (%s), margin %.3g, gap %.3g"
          % (case, F.form_id(form), p.seed, p.relu_ratio, p.n_pre, min(p.sens.values()),
             min(p.sens, key=p.sens.get), p.margin, p.gap))
    F.assert_preconditions(p)
