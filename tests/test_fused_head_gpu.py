"""The head of a rollout as one launch (csrc/head_fused.hip: gcm_dense_rows_head_fused; DenseGCM.rows_fused_head, env
GCM_FUSED_HEAD): the packed parameter vector, the cached step's weight image and the zero state against the three
launches it stands in for - torch.cat, gcm_dense_rows_cached_weight_image, torch.zeros - bit for bit: through the C
ABI, through the module (beliefs, state, gradients, rebuilt after the parameters change) and under graph capture."""
import ctypes

import pytest
import torch

from test_dense_gpu import DEV
from test_rows_gpu import _mk
from test_cached_lean_gpu import _kernels_run

pytestmark = pytest.mark.gpu

FUSED, IMAGE = "k_head_fused", "k_cached_weight_image"


def _pad(n):
    return (n + 63) & ~63


def _sources(F, H1, H2, edge_net, seed):
    """the six GNN tensors (+ the ten of the edge network, widths of gcm_hip.h's layout) with distinct values"""
    shapes = [(H1, F), (H1, F), (H1,), (H2, H1), (H2, H1), (H2,)]
    if edge_net:
        shapes += [(F, 2 * F), (F,), (F,), (F,), (F, F), (F,), (F,), (F,), (1, F), (1,)]
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV) for s in shapes]


def _poison(*sizes):
    """the allocator's cached blocks of these float counts hold NaN (the project's poison: allocate, fill, free)"""
    blocks = [torch.full((n,), float("nan"), device=DEV) for n in sizes if n]
    torch.cuda.synchronize()
    del blocks


def _call(lib, hip, srcs, packed, image, F, H1, H2, zero_ptr, zero_bytes):
    n = len(srcs)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs])
    lens = (ctypes.c_size_t * n)(*[t.numel() for t in srcs])
    rc = lib.gcm_dense_rows_head_fused(ptrs, lens, n, hip.ptr(packed), hip.ptr(image), F, H1, H2, zero_ptr, zero_bytes,
                                       hip.stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("B,N", [(3, 5), (1, 1), (7, 128)])
@pytest.mark.parametrize("F,H1,H2,edge_net", [(32, 32, 32, False), (32, 32, 24, False), (64, 32, 32, False),
                                              (32, 32, 32, True)])
def test_head_fused_c_abi(F, H1, H2, edge_net, B, N):
    """packed == torch.cat, image == gcm_dense_rows_cached_weight_image(packed) over all three layouts, the state all
    zero where the allocator's blocks held NaN; then the forms without a zero region and without an image."""
    from gcm import _hip
    lib = _hip.lib()
    srcs = _sources(F, H1, H2, edge_net, seed=F + H2 + B)
    want_packed = torch.cat([t.reshape(-1) for t in srcs])
    n_img = lib.gcm_dense_rows_cached_weight_image_floats()
    want_image = torch.full((n_img,), float("nan"), device=DEV)
    assert lib.gcm_dense_rows_cached_weight_image(_hip.ptr(want_packed), _hip.ptr(want_image), F, H1, H2, _hip.stream()) == 0
    # (the state of DenseGCM._fresh_state: nodes | adj at 64-float paddings, two floats per graph of counts - a byte
    #  count that is no multiple of the 16-byte store at odd B, and far below one block's round at B = N = 1)
    n_state = _pad(B * N * F) + _pad(B * N * N) + 2 * B
    total = want_packed.numel()

    _poison(total, n_img, n_state)
    packed, image, state = (torch.empty(n, device=DEV) for n in (total, n_img, n_state))
    assert _call(lib, _hip, srcs, packed, image, F, H1, H2, state.data_ptr(), 4 * n_state) == 0
    assert torch.equal(packed.view(torch.int32), want_packed.view(torch.int32))
    assert torch.equal(image.view(torch.int32), want_image.view(torch.int32))
    assert not bool(state.view(torch.int32).any())

    # no zero region: pack + image
    _poison(total, n_img)
    packed, image = (torch.empty(n, device=DEV) for n in (total, n_img))
    assert _call(lib, _hip, srcs, packed, image, F, H1, H2, None, 0) == 0
    assert torch.equal(packed.view(torch.int32), want_packed.view(torch.int32))
    assert torch.equal(image.view(torch.int32), want_image.view(torch.int32))

    # no image: fill + pack
    _poison(total, n_state)
    packed, state = (torch.empty(n, device=DEV) for n in (total, n_state))
    assert _call(lib, _hip, srcs, packed, None, F, H1, H2, state.data_ptr(), 4 * n_state) == 0
    assert torch.equal(packed.view(torch.int32), want_packed.view(torch.int32))
    assert not bool(state.view(torch.int32).any())


@pytest.mark.parametrize("n_bytes", [1, 15, 16, 17, 4 * 256 * 16 - 3, 4 * 256 * 16 + 16 * 300 + 7, 2048 * 4 * 256 * 16 + 16 * 5 + 9])
def test_head_fused_fill_stays_in_bounds(n_bytes):
    """Any byte count: a tail shorter than a store, less than one block's round, one block and a ragged second round,
    and more than the grid covers in one round - exactly n_bytes bytes are cleared, the byte behind them is not."""
    from gcm import _hip
    lib = _hip.lib()
    srcs = _sources(32, 32, 32, False, seed=1)
    packed = torch.empty(sum(t.numel() for t in srcs), device=DEV)
    buf = torch.full((n_bytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    assert _call(lib, _hip, srcs, packed, None, 32, 32, 32, buf.data_ptr(), n_bytes) == 0
    assert not bool(buf[:n_bytes].any())
    assert bool((buf[n_bytes:] == 0xFF).all())


def test_head_fused_rejects_bad_arguments():
    from gcm import _hip
    lib = _hip.lib()
    srcs = _sources(32, 32, 24, False, seed=2)
    packed = torch.full((sum(t.numel() for t in srcs),), float("nan"), device=DEV)
    image = torch.empty(lib.gcm_dense_rows_cached_weight_image_floats(), device=DEV)
    buf = torch.zeros(64, device=DEV)
    assert _call(lib, _hip, srcs, packed, image, 32, 32, 32, None, 0) != 0             # H2 does not match the sources
    assert _call(lib, _hip, srcs[:5], packed, image, 32, 32, 24, None, 0) != 0         # an image needs the six tensors
    assert _call(lib, _hip, srcs, packed, None, 32, 32, 24, buf.data_ptr() + 4, 16) != 0   # unaligned zero region
    assert bool(torch.isnan(packed).all())


def _rollout(mem, obs, w):
    hid, outs = None, []
    for t in range(obs.shape[0]):
        mx, hid = mem(obs[t], hid)
        outs.append(mx)
    out = torch.stack(outs)
    (out * w).sum().backward()
    return out, hid


def _snapshot(out, hid, g):
    grads = [p.grad for p in g.parameters()]
    # every gradient a view of one flat tensor (PackNode): one storage, back to back in the packed vector's order
    assert len({x.untyped_storage().data_ptr() for x in grads}) == 1
    order = sorted(grads, key=lambda x: x.storage_offset())
    assert all(a.storage_offset() + a.numel() == b.storage_offset() for a, b in zip(order, order[1:]))
    return (out.detach().clone(), [t.clone() for t in (hid[0], hid[1], hid[3])], [x.clone() for x in grads])


def _same(a, b):
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        assert x.shape == y.shape and torch.equal(x, y)


def _module_stages(fused):
    """three rollouts of one module: as built, after p.data.add_ (no version counter moves), after an optimiser step"""
    B, N, T, F, H = 3, 8, 8, 32, 32
    torch.manual_seed(7)
    ref, g, mem, osel = _mk(B, N, F, H, H, ("temporal", [1, 2, 4], "forward"), True)
    mem.rows_fused_head = fused
    gen = torch.Generator().manual_seed(8)
    obs, w = torch.rand(T, B, F, generator=gen).to(DEV), torch.rand(T, B, H, generator=gen).to(DEV)
    opt = torch.optim.SGD(g.parameters(), lr=0.1)
    stages, names = [], []
    for stage in range(3):
        g.zero_grad(set_to_none=True)
        box = {}
        names.append(_kernels_run(lambda: box.update(r=_rollout(mem, obs, w))))
        assert mem.rows_cached_steps_taken() == T
        stages.append(_snapshot(*box["r"], g))
        if stage == 0:
            for p in g.parameters():
                p.data.add_(0.03125)
        elif stage == 1:
            opt.step()
    mem.check_flags()
    return stages, names


def test_fused_head_module_on_off():
    """Donated per-step rollouts from hidden = None with rows_fused_head on and off: beliefs, final state and the six
    gradients bit-identical at every stage (so the vector AND the image were rebuilt from the changed parameters); the
    head is one launch of the fused kernel with the switch on, cat + image kernel with it off."""
    on, names_on = _module_stages(True)
    off, names_off = _module_stages(False)
    for a, b in zip(on, off):
        _same(a, b)
    assert not torch.equal(on[0][0], on[1][0]) and not torch.equal(on[1][0], on[2][0])   # (the stages do differ)
    for names in names_on:
        assert any(FUSED in k for k in names) and not any(IMAGE in k for k in names)
    for names in names_off:
        assert any(IMAGE in k for k in names) and not any(FUSED in k for k in names)


def test_fused_head_from_a_callers_state():
    """A chain that starts from a state the caller made: pack + image in one launch (no zero region), results as with
    the switch off."""
    B, N, T, F, H = 3, 8, 6, 32, 32
    res = []
    for fused in (True, False):
        torch.manual_seed(9)
        ref, g, mem, osel = _mk(B, N, F, H, H, ("temporal", [1, 2], "forward"), True)
        mem.rows_fused_head = fused
        gen = torch.Generator().manual_seed(10)
        obs = torch.rand(T, B, F, generator=gen).to(DEV)
        hid = tuple(t.to(DEV) for t in mem.get_initial_hidden_state(torch.zeros(B, F)))
        box = {}

        def run():
            h, outs = hid, []
            for t in range(T):
                mx, h = mem(obs[t], h)
                outs.append(mx)
            out = torch.stack(outs)
            out.sum().backward()
            box["r"] = (out, h)

        names = _kernels_run(run)
        assert any(FUSED in k for k in names) == fused
        res.append(_snapshot(*box["r"], g))
        mem.check_flags()
    _same(res[0], res[1])


def test_fused_head_graph_capture_replay():
    """Loop + backward captured with the fused head and replayed, a parameter changed in place between two replays:
    each replay equals the eager, switched-off run of a fresh module with the same parameters, bit for bit."""
    B, N, T, F, H = 3, 8, 4, 32, 32
    torch.manual_seed(11)
    ref, g, mem, osel = _mk(B, N, F, H, H, ("temporal", [1, 2, 4], "forward"), True)
    assert mem.rows_fused_head
    gen = torch.Generator().manual_seed(12)
    obs, w = torch.rand(T, B, F, generator=gen).to(DEV), torch.rand(T, B, H, generator=gen).to(DEV)

    def eager_off():
        ref2, g2, mem2, _ = _mk(B, N, F, H, H, ("temporal", [1, 2, 4], "forward"), True)
        g2.load_state_dict(g.state_dict())
        mem2.rows_fused_head = False
        out, hid = _rollout(mem2, obs, w)
        torch.cuda.synchronize()
        return _snapshot(out, hid, g2)

    # (warm-up on a side stream, no eager autograd graph left alive: as test_hops_bptt_graph_capture_replay)
    for _ in range(2):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            g.zero_grad(set_to_none=True)
            _rollout(mem, obs, w)
        torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, hid_g = _rollout(mem, obs, w)
    for change in (False, True):
        with torch.no_grad():
            for p in g.parameters():
                if change:
                    p.add_(0.0625)
                p.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _same(_snapshot(out_g, hid_g, g), eager_off())
    mem.check_flags()
