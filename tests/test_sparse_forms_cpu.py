"""The preconditions of tests/test_sparse_forms_gpu.py, from the oracle alone (tests/_sparse_forms.py): under the seed
chosen for every (case, form) the float64 pre-activations of every ReLU sit >= 10 x the oracle's own float32 error away
from zero with equal signs, every neighbouring wrong form moves the float64 beliefs >= 100 x their atol, and the sparse
LearnedEdge selects the same edges in float32 and float64 with its decisions >= 1e-3 from flipping.  No GPU."""
import pytest
import torch

import _forms as F
import _sparse_forms as S


def test_sparse_forms_cover_the_matrix():
    """The forms of the dense file on 7 cases, LEARNED_FORMS on `learned`: 81 pairs, a seed in range(32) for each; the
    call layouts the kernel dispatch depends on (flat rows M per call; strictly descending hops)."""
    assert S.FORMS is F.FORMS and S.LEARNED_FORMS is F.LEARNED_FORMS
    assert len(S.pairs()) == 7 * 11 + 4 == 81
    assert set(S.SEEDS) == {(case, S.form_id(form)) for case, form in S.pairs()}
    assert all(0 <= s < 32 for s in S.SEEDS.values())
    for name, c in S.CASES.items():
        hops = c.get("hops")
        assert hops is None or all(a > b for a, b in zip(hops, hops[1:])), name
    gen = torch.Generator().manual_seed(0)
    flat = {}
    for name, c in S.CASES.items():
        T, rows = torch.zeros(c["shape"][0], dtype=torch.long), []
        for taus in S.call_taus(name, gen):
            assert int(taus.sum()) > 0
            T = T + taus
            rows.append(int(T.sum()))
        assert int(T.max()) <= c["shape"][1], name
        flat[name] = rows
    assert flat["oneshot"] == [64] and flat["oneshot64"] == [80] and flat["khop"] == [64]
    assert flat["two_calls"] == [40, 71] and flat["wide"] == [26] and flat["learned"] == [32, 64]
    assert len(flat["chain"]) == 12 and flat["chain"][0] < 32       # (the early calls of the general driver: M < 32)
    assert flat["chain64"] == [3 * (t + 1) for t in range(10)]


@pytest.mark.parametrize("case,form", S.pairs(), ids=["%s-%s" % (c, S.form_id(f)) for c, f in S.pairs()])
def test_sparse_form_preconditions(case, form):
    p = S.preconditions(case, form, S.SEEDS[(case, S.form_id(form))])
    B, N, Fin, H1, H2 = S.CASES[case]["shape"]
    n_relu = sum(a == "relu" for a in form[:2])
    assert (p.n_pre > 0) == (n_relu > 0)
    # every flat row of every call, per ReLU layer (`khop`: every node is an output node, the 2-hop subgraph is whole)
    T, rows = torch.zeros(B, dtype=torch.long), 0
    for _, taus in p.inp.calls:
        T = T + taus
        rows += int(T.sum())
    assert p.r64.rows == p.r32.rows == rows
    assert p.n_pre == rows * ((H1 if form[0] == "relu" else 0) + (H2 if form[1] == "relu" else 0))
    assert len(p.sens) == len(S.wrong_forms(form)) >= 4
    print("\nSPARSE-FORMS-PRE %s %s seed %d: relu ratio %.1f over %d, sensitivity >= %.0f x atol (%s), gap %.3g, cut %.3g"
          % (case, S.form_id(form), p.seed, p.relu_ratio, p.n_pre, min(p.sens.values()),
             min(p.sens, key=p.sens.get), p.gap, p.cut))
    S.assert_preconditions(p)
