"""The SparseGCM step kernels in every activation / bias form: act1 / act2 in {none, tanh, relu} and the presence of each
lin_rel.bias are run-time arguments of sparse_temporal_step, gcm_sparse_step_cached, gcm_csr_graphconv_fwd /
_fwd_checked / _bwd and the chain's gcm_dense_rows_bptt_cached, and every CSR kernel (k_csr_fwd3 and its checked form,
k_csr_fwd2, k_csr_graphconv_fwd; k_csr_bwd3, k_rows_bwd2, k_graphconv_bwd_rows) carries its own activation epilogue and
its own act'.  11 forms on the smallest shapes that reach each kernel family (tests/_sparse_forms.py), every driver of a
(case, form) against ONE cached oracle trajectory: state bit equal to the float32 oracle, the beliefs of every call and
every gradient inside the float64 bounds, the path (one C++ call / chain on the caches / layered) that must have run.
The seeds are chosen so that no ReLU pre-activation sits within 10 x the oracle's float32 error of zero and every wrong
form would be seen (tests/test_sparse_forms_cpu.py asserts the same without a GPU).  Needs an MI355X.

Worst error / atol measured on an MI355X: see DESIGN.md section 4, "Sparse forms"."""
import pytest
import torch

import _sparse_forms as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# driver -> cases; `fast` runs every (case, form)
LAYERED = ("oneshot", "two_calls", "wide")
GENERAL = ("chain", "chain64")
NO_GRAD = ("oneshot", "chain")
PARAMS = [(case, form, "fast") for case, form in S.pairs()]
PARAMS += [(case, form, "layered") for case in LAYERED for form in S.FORMS]
PARAMS += [(case, form, "general") for case in GENERAL for form in S.FORMS]
PARAMS += [(case, form, "no_grad") for case in NO_GRAD for form in S.FORMS]


def _build(t, driver):
    from gcm import nn as G
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.temporal import TemporalEdge
    from gcm.sparse_edge_selectors.learned import LearnedEdge
    c = S.CASES[t.case]
    B, N, Fin, H1, H2 = t.shape
    g = S.build_gnn(Fin, H1, H2, t.form, G.GraphConv, G.Sequential)
    g.load_state_dict(t.inp.gnn)
    g = g.to(DEV)
    named = dict(g.named_parameters())
    for conv, bit in zip(S.convs_of(g), (1, 2)):       # a missing bias: no tensor, so no gradient - as on the oracle
        assert (conv.lin_rel.bias is None) == (not t.form[2] & bit)
    if "learned" in c:
        sel = LearnedEdge(Fin, num_edge_samples=c["learned"]["k"], window=c["learned"]["window"], store_grads=False)
        sel.edge_network.load_state_dict(t.inp.net)
        sel = sel.to(DEV)
        named.update({"net." + k: p for k, p in sel.edge_network.named_parameters()})
    else:
        sel = TemporalEdge(c["hops"])
    mem = SparseGCM(g, edge_selectors=sel, graph_size=N, max_hops=c.get("max_hops"))
    if driver == "layered":
        mem.fast_host = False
    if driver == "general":
        mem.stepwise_cache = False
    assert set(named) == {k for k in t.bounds if not k.startswith("x")}
    return mem, named


def _assert_path(mem, t, driver):
    """Which host path ran: the one C++ call (`_canonical()`), the chain on the caches, the k-hop mask inside our own
    layers, or the layered Python path."""
    calls = len(t.inp.calls)
    if t.case == "khop":
        assert mem._canonical() is None and mem._native_gnn()
    elif t.case == "learned":
        assert mem._canonical() is None
    else:
        assert mem._canonical() is not None
    if "chain" in S.CASES[t.case] and driver in ("fast", "no_grad"):
        assert mem._chain.steps() == calls and mem._chain.live()
    else:
        assert mem._chain is None
    if driver == "layered":
        assert not mem.fast_host


def _check(t, tag, outs, hidden, named, xs, grads):
    want = t.hidden
    adj = hidden[1].detach().coalesce()
    assert torch.equal(hidden[0].detach().cpu(), want[0]), "node matrix must be bit exact"
    assert torch.equal(adj.indices().cpu(), want[1].indices()), "COO indices must be bit exact"
    assert torch.equal(adj.values().cpu(), want[1].values())
    assert torch.equal(hidden[2].cpu(), want[2])
    assert len(outs) == len(t.out64)
    worst = {"belief": 0.0, "grad": 0.0}
    bad, where = [], None
    for i, (out, out64, atol) in enumerate(zip(outs, t.out64, t.out_atol)):
        assert tuple(out.shape) == tuple(out64.shape)
        ratio = float((out.detach().cpu().double() - out64).abs().max()) / atol
        worst["belief"] = max(worst["belief"], ratio)
        if not ratio <= 1.0:
            bad.append(("belief of call %d" % i, ratio))
    if grads:
        for k, (g64, atol) in t.bounds.items():
            got = xs[int(k[1:])].grad if k.startswith("x") else named[k].grad
            assert got is not None, (tag, k, "no gradient")
            ratio = float((got.detach().cpu().double() - g64).abs().max()) / atol
            if ratio > worst["grad"]:
                worst["grad"], where = ratio, k
            if not ratio <= 1.0:
                bad.append((k, ratio))
    print("\nFORMS sparse %s: worst error/atol belief %.3f grad %.3f (%s)" % (tag, worst["belief"], worst["grad"], where))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("case,form,driver", PARAMS, ids=["%s-%s-%s" % (c, S.form_id(f), d) for c, f, d in PARAMS])
def test_sparse_forms_vs_oracle(case, form, driver):
    """Drivers: the module as built (`fast`: one C++ call per forward, the chain on the caches for x [B, 1, F]),
    fast_host = False (`layered`: gcm.nn.GraphConv with the activation in the epilogue of _ops.csr_graphconv),
    stepwise_cache = False (`general`: every call of a chain through both layers over all stored nodes), and the calls
    under torch.no_grad() (`no_grad`: beliefs and state only - no agg buffers, short records)."""
    t = S.trajectory(case, form)
    S.assert_preconditions(t.pre)            # before the device is touched
    c = S.CASES[case]
    mem, named = _build(t, driver)
    tag = "%s %s %s" % (case, S.form_id(form), driver)
    grads = driver != "no_grad"
    xs = [x.to(DEV).requires_grad_(bool(grads and c.get("x_grad"))) for x, _ in t.inp.calls]
    ws = [w.to(DEV) for w in t.inp.w]
    if "learned" in c:        # the recorded gumbel draws, one per candidate pair in candidate order
        noise, n_call = [z.to(DEV) for z in t.inp.noise], [0]

        def draws(logits):
            n_call[0] += 1
            assert logits.numel() == noise[n_call[0] - 1].numel()
            return noise[n_call[0] - 1]
        mem.edge_selectors.noise_fn = draws
    hidden, outs = None, []
    with torch.set_grad_enabled(grads):
        for x, (_, taus) in zip(xs, t.inp.calls):
            out, hidden = mem(x, taus.to(DEV), hidden)
            outs.append(out)
        _assert_path(mem, t, driver)
        if grads:
            sum((o * w).sum() for o, w in zip(outs, ws)).backward()
    torch.cuda.synchronize()
    mem._check_flags(mem._flag_word(xs[0].device))
    if "learned" in c:
        assert n_call[0] == len(t.inp.calls)
    if not grads:
        assert not any(o.requires_grad for o in outs) and all(p.grad is None for p in named.values())
    _check(t, tag, outs, hidden, named, xs, grads)
