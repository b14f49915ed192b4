"""Plain-torch restatement of SparseGCM.drop_oldest and the helpers the sliding-window tests share.
TEST INFRASTRUCTURE ONLY: runs on whatever device its tensors live on, pinned against oracle/ by
tests/test_sparse_window_cpu.py."""
import torch


def drop_oldest_ref(hidden, k):
    nodes, adj, T = hidden
    adj = adj.coalesce()
    B, N, F = nodes.shape
    k = torch.minimum(k.clamp(min=0), T)
    j = torch.arange(N, device=nodes.device)[None, :] + k[:, None]
    g = nodes.gather(1, j.clamp(max=N - 1)[:, :, None].expand(B, N, F))
    new_nodes = torch.where((j < T[:, None])[:, :, None], g, torch.zeros_like(g))
    idx, val = adj.indices(), adj.values()
    kb = k[idx[0]]
    keep = idx[2] >= kb
    nidx = torch.stack([idx[0][keep], idx[1][keep] - kb[keep], idx[2][keep] - kb[keep]])
    return new_nodes, torch.sparse_coo_tensor(nidx, val[keep], size=adj.shape), T - k


def wrap_k(T, taus, N):
    """How many nodes every graph loses ahead of a call in overflow="wrap"."""
    return (T + taus - N).clamp(min=0)


def reset_ref(hidden, mask):
    return drop_oldest_ref(hidden, torch.where(mask, hidden[2], torch.zeros_like(hidden[2])))


def random_causal_state(B, N, F, density, T=None, seed=0, device="cpu"):
    """A hidden state this module could have made: T_b nodes per graph (rows beyond are zero), a coalesced edge list
    with sink > source, both < T_b, random values."""
    gen = torch.Generator().manual_seed(seed)
    if T is None:
        T = torch.randint(0, N + 1, (B,), generator=gen)
    nodes = torch.rand(B, N, F, generator=gen)
    nodes = nodes * (torch.arange(N)[None, :] < T[:, None])[:, :, None]
    live = torch.arange(N)[None, :, None] < T[:, None, None]
    m = torch.tril(torch.rand(B, N, N, generator=gen) < density, diagonal=-1) & live
    idx = m.nonzero().T.contiguous()
    val = torch.rand(idx.shape[1], generator=gen) + 0.5
    adj = torch.sparse_coo_tensor(idx, val, size=(B, N, N)).coalesce()
    return nodes.to(device), adj.to(device), T.to(device)


def state_equal(got, want):
    """Exact equality of two hidden states (nodes, coalesced indices, values, T)."""
    ga, wa = got[1].coalesce(), want[1].coalesce()
    return (torch.equal(got[0], want[0]) and torch.equal(ga.indices(), wa.indices())
            and torch.equal(ga.values(), wa.values()) and torch.equal(got[2], want[2]))


def is_sorted_coo(idx, N):
    """Strictly ascending by (batch, sink, source): coalesced order, no duplicates."""
    key = (idx[0] * N + idx[1]) * N + idx[2]
    return bool((key[1:] > key[:-1]).all())
