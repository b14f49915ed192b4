"""The GEMM-form backward (csrc/rows_bptt_hops.hip: k_bptt_hops_graph) through gcm_dense_rows_bptt_cached_hops on the
cases its first tests leave out: one and two graphs, the waves' ownership boundaries at rows 16 w, H2 = 24, a step
order that is not the identity, g_params_prev, a captured call - against the float64 restatement
(tests/_bptt_hops_restate.py) under the bound tests/test_bptt_hops_gpu.py uses (its _Chain.check), and bit for bit from
call to call and replay to replay.  (The re-cut these cases were written for - the records' h1cur section not read
where the same lane holds the cache row - left the benchmark where it was and is not part of the kernel: DESIGN 3.2.)"""
import ctypes

import pytest
import torch

from test_dense_gpu import DEV
from test_bptt_hops_gpu import _Chain, _desc, F, H1

pytestmark = pytest.mark.gpu


def _run(ch, steps, grads, sb, sh, prev=None, out=None):
    """gcm_dense_rows_bptt_cached_hops over the records `steps` (step i of the call = record steps[i], which wrote row
    steps[i]) -> g_params on the device"""
    hip, lib, B = ch.hip, ch.lib, ch.B
    n = len(steps)
    sv = (ctypes.c_void_p * n)(*[ch.saved[t].data_ptr() for t in steps])
    gm = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
    cb = (ctypes.c_uint8 * n)(*steps)
    ws_bytes = 4 * ch.P * B
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((ch.P,), float("nan"), device=DEV) if out is None else out
    desc = _desc(hip, ch.hops)
    p = hip.ptr
    rc = lib.gcm_dense_rows_bptt_cached_hops(sv, gm, n, sb, sh, p(ch.params), 3, 1, 1, p(ch.cX), p(ch.cH), p(ch.cA), cb,
                                             ctypes.addressof(desc), 1, ch.T, p(prev), p(out), p(ws), ws_bytes, B, ch.N,
                                             F, H1, ch.H2, hip.stream())
    assert rc == 0, rc
    return out


def _both(ch, steps, grads, sb, sh, **kw):
    """two calls on the same inputs: identical bits"""
    new = _run(ch, steps, grads, sb, sh, **kw)
    again = _run(ch, steps, grads, sb, sh, **kw)
    torch.cuda.synchronize()
    assert torch.equal(new.view(torch.int32), again.view(torch.int32))
    return new.cpu()


@pytest.fixture(scope="module")
def chains():
    """one chain per (hops, B, N, T, H2), built once and left unchanged"""
    cache = {}

    def get(hops, B, N, T, H2):
        key = (tuple(hops), B, N, T, H2)
        if key not in cache:
            cache[key] = _Chain(hops, B, N, H2, T, seed=N + T + H2 + B)
        return cache[key]

    return get


# wave ownership boundaries at rows 16 w (T = 16, 33, 128), a chain shorter than its largest hop ((16, 5) with hop 9),
# a last wave with partly missing steps (T = 33, 5); a self loop and a duplicate hop
@pytest.mark.parametrize("H2", [32, 24])
@pytest.mark.parametrize("hops,N,T", [([1, 2, 9], 16, 5), ([0, 3, 5, 3], 16, 16), ([1, 2, 4], 128, 128), ([0, 1, 2, 4], 128, 33)])
@pytest.mark.parametrize("B", [1, 2, 9])
def test_recut_identity_rows(chains, hops, N, T, H2, B):
    """cur_host the identity (every chain from empty graphs whose steps all take part): inside the float64 bound."""
    ch = chains(hops, B, N, T, H2)
    g = torch.rand(T, B, H2, generator=torch.Generator().manual_seed(5))
    gd = g.to(DEV)
    steps = list(range(T))
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1)
    ch.check(got, steps, g)


@pytest.mark.parametrize("hops,N,T,H2", [([1, 2, 4], 128, 33, 24), ([0, 3, 5, 3], 16, 16, 32)])
def test_recut_reversed_steps(chains, hops, N, T, H2):
    """The call's steps in reverse order (step i wrote row T - 1 - i): the row -> step map is not the identity, the
    wave that owns a step does not own the row it wrote."""
    B = 2
    ch = chains(hops, B, N, T, H2)
    g = torch.rand(T, B, H2, generator=torch.Generator().manual_seed(6))
    gd = g.to(DEV)
    steps = list(range(T))[::-1]
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1)
    ch.check(got, steps, g[steps])


@pytest.mark.parametrize("part", ["third", "tail", "head"])
def test_recut_gradient_on_part_of_the_beliefs(chains, part):
    """"head": the first 20 steps only - written rows behind the call's last step; "third" / "tail": steps missing in
    front, so cur_host[i] != i."""
    hops, B, N, T, H2 = [1, 2, 4], 2, 128, 33, 24
    ch = chains(hops, B, N, T, H2)
    steps = {"third": list(range(0, T, 3)), "tail": list(range(20, T)), "head": list(range(20))}[part]
    g = torch.rand(T, B, H2, generator=torch.Generator().manual_seed(7))
    gd = g.to(DEV)
    got = _both(ch, steps, [gd[t] for t in steps], H2, 1)
    ch.check(got, steps, g[steps])


def test_recut_expanded_gradient_and_prev(chains):
    """out.sum(): one scalar read with stride 0; g_params_prev added behind the sum (exact in float32 arithmetic:
    prev + gradient, one rounding)."""
    hops, B, N, T, H2 = [0, 3, 5, 3], 9, 16, 16, 24
    ch = chains(hops, B, N, T, H2)
    one = torch.full((1,), 0.75, device=DEV)
    steps = list(range(T))
    got = _both(ch, steps, [one] * T, 0, 0)
    ch.check(got, steps, torch.full((T, B, H2), 0.75))
    prev = torch.rand(ch.P, generator=torch.Generator().manual_seed(8)).to(DEV)
    with_prev = _both(ch, steps, [one] * T, 0, 0, prev=prev)
    assert torch.equal(with_prev, (prev.cpu() + got))


def test_recut_two_replays_of_a_captured_call(chains):
    """The call captured as a HIP graph and replayed twice over a poisoned output: the bits of the eager call."""
    hops, B, N, T, H2 = [1, 2, 4], 9, 128, 128, 32
    ch = chains(hops, B, N, T, H2)
    gd = torch.rand(T, B, H2, generator=torch.Generator().manual_seed(5)).to(DEV)
    steps = list(range(T))
    grads = [gd[t] for t in steps]
    eager = _run(ch, steps, grads, H2, 1).clone()
    out = torch.empty(ch.P, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(ch, steps, grads, H2, 1, out=out)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run(ch, steps, grads, H2, 1, out=out)
    for _ in range(2):
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32))
