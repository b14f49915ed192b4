"""The lean cached step (csrc/rows_cached_lean.hip): cfg2's case of the cached temporal-hops step - F = H1 = 32,
H2 <= 32, tanh / tanh, at most four forward hops, the row known on the host - against k_step_rows_cached_img4b behind
the A/B switch (GCM_STEP_NOT_LEAN in has_bias; the module's GCM_LEAN_STEP) and against the oracle."""
import ctypes

import pytest
import torch

from test_dense_gpu import DEV
from test_rows_gpu import _mk
from _golden import fp64_rollout_bounds

pytestmark = pytest.mark.gpu

IMG_V4, NOT_LEAN = 64, 1024


def _chain(lib, _hip, hops, B, N, H2, T, flags_bits, seed):
    """T cached steps from empty graphs through the C ABI: [(record, nodes, adj, count, cH, cA, cX) after each step]"""
    F = H1 = 32
    g = torch.Generator().manual_seed(seed)
    P = lib.gcm_dense_gnn2_param_count(F, H1, H2)
    params = (torch.randn(P, generator=g) * 0.2).to(DEV)
    obs = torch.rand(T, B, F, generator=g).to(DEV)
    img = torch.empty(lib.gcm_dense_rows_cached_weight_image_floats(), device=DEV)
    st, p = _hip.stream(), _hip.ptr
    assert lib.gcm_dense_rows_cached_weight_image(p(params), p(img), F, H1, H2, st) == 0
    lay = (ctypes.c_size_t * 5)()
    assert lib.gcm_dense_rows_cached_layout(B, N, F, H1, H2, ctypes.addressof(lay)) == 0
    d = _hip.SelectorDesc(kind=_hip.SEL_TEMPORAL, n_hops=len(hops), direction=_hip.DIR["forward"])
    for i, h in enumerate(hops):
        d.hops[i] = h
    arr = (_hip.SelectorDesc * 1)(d)
    nodes, adj = torch.zeros(B, N, F, device=DEV), torch.zeros(B, N, N, device=DEV)
    count = torch.zeros(B, dtype=torch.int64, device=DEV)
    cH, cA, cX = (torch.full((B, N, w), float("nan"), device=DEV) for w in (H1, F, F))
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = []
    for t in range(T):
        saved = torch.full((lay[0],), float("nan"), device=DEV)
        rc = lib.gcm_dense_rows_step_cached(p(obs[t]), p(nodes), p(adj), p(count), ctypes.addressof(arr), 1, p(params),
                                            p(img), 3 | flags_bits, 1, 1, p(cH), p(cA), p(cX), p(saved), 1, t, p(flags),
                                            B, N, F, H1, H2, st)
        assert rc == 0, (t, rc)
        out.append(tuple(x.clone() for x in (saved, nodes, adj, count, cH, cA, cX)))
    torch.cuda.synchronize()
    assert int(flags.item()) == 0
    return out, lay


@pytest.mark.parametrize("H2", [16, 32])
@pytest.mark.parametrize("hops,N,T", [([1, 2, 4], 128, 128), ([1, 2, 4], 40, 25), ([1], 32, 32), ([3, 5], 24, 17),
                                      ([0, 1, 2, 4], 128, 60), ([0, 3, 5], 16, 16), ([2, 4, 1, 2], 20, 20)])
def test_lean_step_c_abi_against_img4b(hops, N, T, H2):
    """Every output of the lean step against img4b's, step by step: the state, the node / agg1 caches and the record's
    header, live list and coefficients bit exact; the beliefs, h1 and agg2 (the two layers' products re-associated:
    two chains of eight per half-wave instead of one of sixteen) within a few ulps of tanh's range."""
    from gcm import _hip
    lib = _hip.lib()
    B = 9
    lean, lay = _chain(lib, _hip, hops, B, N, H2, T, IMG_V4, seed=N + T + H2)
    base, _ = _chain(lib, _hip, hops, B, N, H2, T, IMG_V4 | NOT_LEAN, seed=N + T + H2)
    o_v, o_hdr, o_coef, o_live = (int(x) for x in lay[1:5])
    for t in range(T):
        (sv, n, a, c, h, ca, cx), (sv0, n0, a0, c0, h0, ca0, cx0) = lean[t], base[t]
        assert torch.equal(n, n0) and torch.equal(a, a0) and torch.equal(c, c0), t
        assert torch.equal(ca[:, :t + 1], ca0[:, :t + 1]) and torch.equal(cx[:, :t + 1], cx0[:, :t + 1]), t
        assert float((h[:, :t + 1] - h0[:, :t + 1]).abs().max()) <= 2e-6, t
        assert float((sv[:B * H2] - sv0[:B * H2]).abs().max()) <= 2e-6, t
        assert float((sv[o_v:o_v + B * 64] - sv0[o_v:o_v + B * 64]).abs().max()) <= 1e-5, t
        hdr, hdr0 = sv[o_hdr:o_hdr + 4 * B].view(torch.int32), sv0[o_hdr:o_hdr + 4 * B].view(torch.int32)
        assert torch.equal(hdr, hdr0), t
        L = hdr.view(B, 4)[:, 0].cpu()
        live, live0 = sv[o_live:o_live + B * N].view(torch.int32).view(B, N), sv0[o_live:o_live + B * N].view(torch.int32).view(B, N)
        coef, coef0 = sv[o_coef:o_coef + B * N].view(B, N), sv0[o_coef:o_coef + B * N].view(B, N)
        for b in range(B):
            assert torch.equal(live[b, :L[b]], live0[b, :L[b]]) and torch.equal(coef[b, :L[b]], coef0[b, :L[b]]), (t, b)


def _kernels_run(fn):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events()}


@pytest.mark.parametrize("H2", [16, 32])
@pytest.mark.parametrize("hops,N,T", [([1, 2, 4], 128, 128), ([1, 2, 4], 64, 40), ([1], 32, 32), ([3, 5], 24, 17),
                                      ([0, 1, 2, 4], 48, 48), ([0, 3, 5], 16, 11)])
def test_lean_step_module_vs_oracle(hops, N, T, H2):
    """A donated DenseGCM rollout from hidden = None, forward and backward, with the lean step and with img4b
    (rows_lean_step, the module's side of GCM_LEAN_STEP): state bit exact against the oracle, beliefs and parameter
    gradients inside the float64 bound; the lean kernel is the one that ran."""
    B, F, H1 = 6, 32, 32
    res = []
    obs = None
    for lean in (True, False):
        torch.manual_seed(N + T + H2)
        ref, g, mem, osel = _mk(B, N, F, H1, H2, ("temporal", hops, "forward"), True)
        mem.rows_lean_step = lean
        obs = torch.rand(T, B, F)
        w = torch.rand(T, B, H2)
        box = {}

        def run():
            hid, outs = None, []
            for t in range(T):
                mx, hid = mem(obs[t].to(DEV), hid)
                outs.append(mx)
            out = torch.stack(outs)
            (out * w.to(DEV)).sum().backward()
            box["out"], box["hid"] = out, hid

        names = _kernels_run(run)
        assert any("k_step_rows_cached_img4_lean" in k for k in names) == lean
        assert any("k_step_rows_cached_img4b" in k for k in names) == (not lean)
        assert mem.rows_cached_steps_taken() == T
        mem.check_flags()
        hid = box["hid"]
        res.append((box["out"].detach().cpu(), [t.cpu() for t in (hid[0], hid[1], hid[3])],
                    {k: p.grad.cpu().clone() for k, p in g.named_parameters()}, ref, osel, w))
    ref, osel, w = res[0][3], res[0][4], res[0][5]
    out32, hid32, bounds, (out64, out_atol) = fp64_rollout_bounds(ref, obs, None, w, lambda: osel, N)
    for out, state, grads, *_ in res:
        assert torch.equal(state[0], hid32[0]) and torch.equal(state[1], hid32[1]) and torch.equal(state[2], hid32[3])
        assert float((out.double() - out64).abs().max()) <= out_atol
        for k, gd in grads.items():
            g64, atol = bounds[k]
            assert float((gd.double() - g64).abs().max()) <= atol, k


@pytest.mark.parametrize("hops,N,T,lean_steps", [([1, 2, 4], 16, 40, 16),            # then the steady-state step
                                                 ([1, 2, 3, 5, 9], 24, 30, 0),       # five hops: img4b throughout
                                                 ([1, 5], 8, 20, 8)])                # N <= 2 max hop: the live-row step behind
def test_lean_step_chain_handed_over_to_other_kernels(hops, N, T, lean_steps):
    """A chain that leaves the lean step's case mid-way (the graphs fill up at t = N) or never enters it (more than four
    hops): the kernels behind it carry on from its caches and records; against the oracle."""
    B, F, H1, H2 = 5, 32, 32, 32
    torch.manual_seed(N + T)
    ref, g, mem, osel = _mk(B, N, F, H1, H2, ("temporal", hops, "forward"), True)
    obs = torch.rand(T, B, F)
    w = torch.rand(T, B, H2)
    box = {}

    def run():
        hid, outs = None, []
        for t in range(T):
            mx, hid = mem(obs[t].to(DEV), hid)
            outs.append(mx)
        out = torch.stack(outs)
        (out * w.to(DEV)).sum().backward()
        box["out"], box["hid"] = out, hid

    names = _kernels_run(run)
    assert any("k_step_rows_cached_img4_lean" in k for k in names) == (lean_steps > 0)
    mem.check_flags()
    out32, hid32, bounds, (out64, out_atol) = fp64_rollout_bounds(ref, obs, None, w, lambda: osel, N)
    hid = box["hid"]
    assert torch.equal(hid[0].cpu(), hid32[0]) and torch.equal(hid[1].cpu(), hid32[1]) and torch.equal(hid[3].cpu(), hid32[3])
    assert float((box["out"].detach().cpu().double() - out64).abs().max()) <= out_atol
    for k, p in g.named_parameters():
        g64, atol = bounds[k]
        assert float((p.grad.cpu().double() - g64).abs().max()) <= atol, k


def test_lean_step_graph_capture_replay():
    """cfg2's loop (T = N, hops [1, 2, 4]) forward and backward captured as a HIP graph - the lean step's per-step
    arguments (row cur, the source rows) baked into each node - and replayed: equal to the eager run, every replay."""
    B, N, F, H1, H2, T = 8, 32, 32, 32, 32, 32
    torch.manual_seed(3)
    ref, g, mem, osel = _mk(B, N, F, H1, H2, ("temporal", [1, 2, 4], "forward"), True)
    obs = torch.rand(T, B, F, device=DEV)

    def rollout():
        hid, outs = None, []
        for t in range(T):
            mx, hid = mem(obs[t], hid)
            outs.append(mx)
        out = torch.stack(outs)
        out.mean().backward()
        return out, hid

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
