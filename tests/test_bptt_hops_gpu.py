"""The GEMM-form backward of forward-hop cached chains (csrc/rows_bptt_hops.hip: gcm_dense_rows_bptt_cached_hops)
against the record-walking kernel it stands in for (gcm_dense_rows_bptt_cached: k_bptt_cached_graph), on the same
records, and against the float64 restatement of its formulas (tests/_bptt_hops_restate.py) under the project's bound
rule; then through the module (DenseGCM.rows_hops_bptt, env GCM_BPTT_HOPS) against the oracle."""
import ctypes

import pytest
import torch

from test_dense_gpu import DEV
from test_rows_gpu import _mk
from test_cached_lean_gpu import _chain, _kernels_run, IMG_V4
from _golden import fp64_rollout_bounds
import _bptt_hops_restate as R

pytestmark = pytest.mark.gpu

NEW, OLD = "k_bptt_hops_graph", "k_bptt_cached_graph"
F = H1 = 32


def _desc(_hip, hops, direction="forward"):
    d = _hip.SelectorDesc(kind=_hip.SEL_TEMPORAL, n_hops=len(hops), direction=_hip.DIR[direction])
    for i, h in enumerate(hops):
        d.hops[i] = h
    return (_hip.SelectorDesc * 1)(d)


class _Chain:
    """T cached steps from empty graphs through the C ABI (test_cached_lean_gpu._chain: caches NaN beyond the written
    rows), kept for both backward entries and the restatement."""

    def __init__(self, hops, B, N, H2, T, seed):
        from gcm import _hip
        self.hip, self.lib = _hip, _hip.lib()
        self.hops, self.B, self.N, self.H2, self.T = hops, B, N, H2, T
        steps, lay = _chain(self.lib, _hip, hops, B, N, H2, T, IMG_V4, seed)
        self.o_v = int(lay[1])
        self.saved = [s[0] for s in steps]
        self.cH, self.cA, self.cX = steps[-1][4:7]
        assert bool(torch.isnan(self.cH[:, T:]).all()) and bool(torch.isnan(self.cX[:, T:]).all())
        self.P = self.lib.gcm_dense_gnn2_param_count(F, H1, H2)
        # (_chain's own parameters: the first draw of its generator)
        self.params = (torch.randn(self.P, generator=torch.Generator().manual_seed(seed)) * 0.2).to(DEV)

    def run(self, which, steps, grads, sb, sh, cur=None, desc=None, rows_written=None, N=None, F_=F):
        """-> (return code, g_params) of one backward entry over the records `steps` with gradient tensors `grads`"""
        hip, lib, B = self.hip, self.lib, self.B
        n = len(steps)
        sv = (ctypes.c_void_p * n)(*[self.saved[t].data_ptr() for t in steps])
        gm = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
        ws_bytes = max(lib.gcm_dense_rows_bptt_workspace_bytes(n, B, F, H1, self.H2), 4 * self.P * B)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        out = torch.full((self.P,), float("nan"), device=DEV)
        p, st = hip.ptr, hip.stream()
        N = self.N if N is None else N
        if which == "old":
            rc = lib.gcm_dense_rows_bptt_cached(sv, gm, n, sb, sh, p(self.params), 3, 1, 1, p(self.cX), p(self.cH),
                                                p(self.cA), None, p(out), p(ws), ws_bytes, B, N, F_, H1, self.H2, st)
        else:
            cur = steps if cur is None else cur
            cb = (ctypes.c_uint8 * n)(*cur)
            desc = _desc(hip, self.hops) if desc is None else desc
            rc = lib.gcm_dense_rows_bptt_cached_hops(sv, gm, n, sb, sh, p(self.params), 3, 1, 1, p(self.cX), p(self.cH),
                                                     p(self.cA), cb, ctypes.addressof(desc), 1,
                                                     self.T if rows_written is None else rows_written, None, p(out),
                                                     p(ws), ws_bytes, B, N, F_, H1, self.H2, st)
        torch.cuda.synchronize()
        return rc, out.cpu()

    def restated(self, steps, g, dtype):
        """the restatement on the records the GPU wrote; g [S, B, H2] on the CPU -> packed gradient"""
        B, H2, T = self.B, self.H2, self.T
        mx = torch.stack([self.saved[t][:B * H2].view(B, H2) for t in steps]).cpu().to(dtype)
        v = torch.stack([self.saved[t][self.o_v:self.o_v + B * 64].view(B, 64) for t in steps]).cpu().to(dtype)
        cH, cA, cX = (c[:, :T].cpu().to(dtype) for c in (self.cH, self.cA, self.cX))
        par = self.params.cpu().to(dtype)
        w_rel2 = par[2 * H1 * F + H1:2 * H1 * F + H1 + H2 * H1].view(H2, H1)
        w_root2 = par[2 * H1 * F + H1 + H2 * H1:2 * H1 * F + H1 + 2 * H2 * H1].view(H2, H1)
        return R.pack(R.backward(mx, v, g.to(dtype), list(steps), cH, cA, cX, w_rel2, w_root2, self.hops))

    def check(self, got, steps, g):
        """inside the float64 bound of the restatement, section by section of the packed vector; no NaN"""
        g64, g32 = self.restated(steps, g, torch.float64), self.restated(steps, g, torch.float32)
        assert not bool(torch.isnan(got).any())
        H2 = self.H2
        o = 0
        for n in (H1 * F, H1 * F, H1, H2 * H1, H2 * H1, H2):
            atol = R.bound(g32[o:o + n], g64[o:o + n])
            err = float((got[o:o + n].double() - g64[o:o + n]).abs().max())
            print("section at %d: err %.3g, bound %.3g" % (o, err, atol))
            assert err <= atol, (o, err, atol)
            o += n


@pytest.mark.parametrize("H2", [16, 32])
@pytest.mark.parametrize("hops,N,T,B", [(h, n, t, 9) for h, n, t in R.CASES[:7]] + [([1, 2, 4], 128, 128, 4)])
def test_hops_bptt_c_abi_against_record_walk(hops, N, T, H2, B):
    """Both entries on the same records (caches NaN beyond the written rows): each inside the float64 bound of the
    restatement, no NaN in g_params, two runs of the new entry bit-identical."""
    ch = _Chain(hops, B, N, H2, T, seed=N + T + H2)
    g = torch.rand(T, B, H2, generator=torch.Generator().manual_seed(5))
    gd = g.to(DEV)
    steps = list(range(T))
    rc_old, old = ch.run("old", steps, [gd[t] for t in steps], H2, 1)
    rc_new, new = ch.run("new", steps, [gd[t] for t in steps], H2, 1)
    assert rc_old == 0 and rc_new == 0
    ch.check(old, steps, g)
    ch.check(new, steps, g)
    rc_again, again = ch.run("new", steps, [gd[t] for t in steps], H2, 1)
    assert rc_again == 0 and torch.equal(new, again)


@pytest.mark.parametrize("part", ["third", "last"])
@pytest.mark.parametrize("hops,N,T", [([1, 2, 4], 40, 25), ([0, 3, 5], 16, 16)])
def test_hops_bptt_gradient_subsets(hops, N, T, part):
    """Gradients for some steps only (n_steps < chain length, rows_written = chain length): a row whose step is not in
    the call still takes the dAgg2 of later steps; slices of a stacked gradient tensor."""
    B, H2 = 9, 32
    ch = _Chain(hops, B, N, H2, T, seed=N + T)
    steps = list(range(0, T, 3)) if part == "third" else [T - 1]
    g = torch.rand(T, B, H2, generator=torch.Generator().manual_seed(6))
    gd = g.to(DEV)
    for which in ("old", "new"):
        rc, got = ch.run(which, steps, [gd[t] for t in steps], H2, 1)
        assert rc == 0, which
        ch.check(got, steps, g[steps])


def test_hops_bptt_expanded_gradient():
    """out.sum(): one scalar read with stride 0 by every graph-step."""
    hops, N, T, B, H2 = [1, 2, 4], 40, 25, 9, 16
    ch = _Chain(hops, B, N, H2, T, seed=11)
    one = torch.full((1,), 0.75, device=DEV)
    steps = list(range(T))
    for which in ("old", "new"):
        rc, got = ch.run(which, steps, [one] * T, 0, 0)
        assert rc == 0, which
        ch.check(got, steps, torch.full((T, B, H2), 0.75))


def test_hops_bptt_eligibility():
    """Cases without a GEMM form return GCM_EUNSUPPORTED and launch nothing (g_params stays as it was)."""
    hops, N, T, B, H2 = [1, 2, 4], 16, 8, 3, 32
    ch = _Chain(hops, B, N, H2, T, seed=2)
    gd = torch.rand(T, B, H2, device=DEV)
    steps = list(range(T))
    gs = [gd[t] for t in steps]
    E = ch.hip.GCM_EUNSUPPORTED
    for kw in (dict(F_=64), dict(desc=_desc(ch.hip, [1, 2, 3, 5, 9])), dict(desc=_desc(ch.hip, hops, "both")),
               dict(cur=[0, 1, 2, 3, 3, 5, 6, 7]), dict(rows_written=T - 1), dict(rows_written=N + 1)):
        rc, out = ch.run("new", steps, gs, H2, 1, **kw)
        assert rc == E, kw
        assert bool(torch.isnan(out).all()), kw
    rc, out = ch.run("new", steps, gs, H2, 1)
    assert rc == 0 and not bool(torch.isnan(out).any())


def _module_run(hops, N, T, H2, B, hops_bptt, rollout=False, seed=None):
    torch.manual_seed(N + T + H2 if seed is None else seed)
    ref, g, mem, osel = _mk(B, N, F, H1, H2, ("temporal", hops, "forward"), True)
    mem.rows_hops_bptt = hops_bptt
    obs = torch.rand(T, B, F)
    w = torch.rand(T, B, H2)
    box = {}

    def run():
        if rollout:
            out, hid = mem.rollout(obs.to(DEV))
        else:
            hid, outs = None, []
            for t in range(T):
                mx, hid = mem(obs[t].to(DEV), hid)
                outs.append(mx)
            out = torch.stack(outs)
        (out * w.to(DEV)).sum().backward()
        box["out"], box["hid"] = out, hid

    names = _kernels_run(run)
    mem.check_flags()
    hid = box["hid"]
    return dict(names=names, out=box["out"].detach().cpu(), state=[t.cpu() for t in (hid[0], hid[1], hid[3])],
                grads={k: p.grad.cpu().clone() for k, p in g.named_parameters()}, ref=ref, osel=osel, obs=obs, w=w, mem=mem)


def _check_vs_oracle(runs, N):
    r0 = runs[0]
    out32, hid32, bounds, (out64, out_atol) = fp64_rollout_bounds(r0["ref"], r0["obs"], None, r0["w"], lambda: r0["osel"], N)
    for r in runs:
        s = r["state"]
        assert torch.equal(s[0], hid32[0]) and torch.equal(s[1], hid32[1]) and torch.equal(s[2], hid32[3])
        assert float((r["out"].double() - out64).abs().max()) <= out_atol
        for k, gd in r["grads"].items():
            g64, atol = bounds[k]
            assert float((gd.double() - g64).abs().max()) <= atol, k


@pytest.mark.parametrize("H2", [16, 32])
@pytest.mark.parametrize("hops,N,T", [([1, 2, 4], 128, 128), ([1, 2, 4], 64, 40), ([1], 32, 32), ([3, 5], 24, 17),
                                      ([0, 1, 2, 4], 48, 48), ([0, 3, 5], 16, 11)])
def test_hops_bptt_module_vs_oracle(hops, N, T, H2):
    """A donated per-step rollout from hidden = None, (out * w).sum().backward(), with rows_hops_bptt on and off: state
    bit exact against the oracle, beliefs and the six parameter gradients inside the float64 bound; the backward kernel
    that ran is the expected one."""
    runs = []
    for on in (True, False):
        r = _module_run(hops, N, T, H2, 6, on)
        assert any(NEW in k for k in r["names"]) == on
        assert any(OLD in k for k in r["names"]) == (not on)
        assert r["mem"].rows_cached_steps_taken() == T
        runs.append(r)
    _check_vs_oracle(runs, N)


@pytest.mark.parametrize("hops,N,T", [([1, 2, 4], 16, 40), ([1, 2, 3, 5, 9], 24, 30), ([1, 5], 8, 20)])
def test_hops_bptt_leaves_handed_over_chains_alone(hops, N, T):
    """Chains that leave the lean step's case mid-way or never enter it (test_lean_step_chain_handed_over_to_other_kernels'
    shapes): the record-walking backward as before, by name, gradients inside the bounds."""
    r = _module_run(hops, N, T, 32, 5, True, seed=N + T)
    assert any(OLD in k for k in r["names"]) and not any(NEW in k for k in r["names"])
    _check_vs_oracle([r], N)


@pytest.mark.parametrize("N,T", [(32, 32), (40, 25)])
def test_hops_bptt_rollout_from_empty_graphs(N, T):
    """DenseGCM.rollout() from empty graphs: the same entry with the trivial table (cur[t] = t), on and off."""
    runs = []
    for on in (True, False):
        r = _module_run([1, 2, 4], N, T, 32, 5, on, rollout=True)
        assert any(NEW in k for k in r["names"]) == on
        runs.append(r)
    _check_vs_oracle(runs, N)


def test_hops_bptt_graph_capture_replay():
    """cfg2's loop forward and backward captured as a HIP graph (the step table and the row -> step map baked into the
    node) and replayed: equal to the eager run, every replay (test_lean_step_graph_capture_replay's comparison; that the
    GEMM form is what such a loop runs by default: test_hops_bptt_module_vs_oracle)."""
    B, N, H2, T = 8, 32, 32, 32
    torch.manual_seed(3)
    ref, g, mem, osel = _mk(B, N, F, H1, H2, ("temporal", [1, 2, 4], "forward"), True)
    assert mem.rows_hops_bptt
    obs = torch.rand(T, B, F, device=DEV)

    def rollout():
        hid, outs = None, []
        for t in range(T):
            mx, hid = mem(obs[t], hid)
            outs.append(mx)
        out = torch.stack(outs)
        out.mean().backward()
        return out, hid

    # (no autograd graph of an eager run may outlive the next two lines - DESIGN 3.11: its AccumulateGrad nodes are bound
    #  to the stream they were made on, and the captured backward would synchronise with it)
    g.zero_grad(set_to_none=True)
    out_e, hid_e = rollout()
    out_e, hid_e = out_e.detach().clone(), tuple(t.clone() for t in hid_e)
    grads_e = {k: p.grad.clone() for k, p in g.named_parameters()}
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g.zero_grad(set_to_none=True)
            rollout()
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, hid_g = rollout()
    for _ in range(3):
        for p in g.parameters():
            p.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(hid_g[0], hid_e[0]) and torch.equal(hid_g[1], hid_e[1]) and torch.equal(hid_g[3], hid_e[3])
        assert torch.equal(out_g.detach(), out_e)
        for k, p in g.named_parameters():
            torch.testing.assert_close(p.grad, grads_e[k], rtol=1e-5, atol=1e-6 * float(grads_e[k].abs().max()) + 1e-9)
    mem.check_flags()
