"""The cases of tests/test_mp_gpu.py (and the restatement checks of tests/test_mp_cpu.py), built on the CPU from seeds.
Edge lists come from tests/_gen_cases.py's helper: duplicate loops (0, 0), a duplicate edge 1 -> 2 and three isolated
nodes in every list with edges."""
import torch

from _gen_cases import MEM, edges, memory_obs  # noqa: F401  (re-exported for the memory tests)

#  M,   E,    C            C: channels, None for a 1-D tensor, a tuple for trailing dimensions
SHAPES = [
    (5, 0, 4),              # no edges
    (40, 90, 8),
    (40, 90, None),         # C = 1, given as a 1-D tensor
    (40, 90, 3),            # the 4-byte path
    (129, 700, 128),
    (40, 90, 260),          # beyond every fused layer's cap; a lane strides over the row
    (64, 2000, 16),         # high degree
    (40, 90, (4, 8)),       # 3-D: [M, H, C]
]


def trailing(C):
    return () if C is None else (C,) if isinstance(C, int) else tuple(C)


def case(M, E, C):
    """-> dict(x [M, ...], ei [2, E'] in the caller's (shuffled) order, src / logits [E', ...], g_m [M, ...],
    g_e [E', ...])."""
    t = trailing(C)
    gen = torch.Generator().manual_seed(1000 * M + E + sum(t))
    ei = edges(M, E, seed=M + E)
    n = ei.shape[1]
    return dict(x=torch.randn((M,) + t, generator=gen), ei=ei, src=torch.randn((n,) + t, generator=gen),
                g_m=torch.randn((M,) + t, generator=gen), g_e=torch.randn((n,) + t, generator=gen))


def csr_order(ei):
    """The list stably sorted by sink (what SparseGCM hands over, with a ready index) and the permutation used."""
    _, perm = torch.sort(ei[1], stable=True)
    return ei[:, perm].contiguous(), perm


def tie_case():
    """Explicit ties.  Node 3 receives edges 0, 1, 3, 4 of the caller's list: in channel 0 the maximum 2.0 is attained
    by edges 1 and 4 (sources 5 and 6), in channel 1 the minimum -3.0 by the same two - the whole gradient belongs to
    edge 1, the earlier in the caller's order.  Node 1 receives edges 2 and 5 with equal messages in both channels:
    edge 2 takes it."""
    ei = torch.tensor([[4, 5, 0, 7, 6, 2], [3, 3, 1, 3, 3, 1]])
    x = torch.zeros(8, 2)
    x[4] = torch.tensor([1.0, 5.0])
    x[5] = torch.tensor([2.0, -3.0])
    x[6] = torch.tensor([2.0, -3.0])
    x[7] = torch.tensor([-1.0, 4.0])
    x[0] = torch.tensor([0.5, 0.5])
    x[2] = torch.tensor([0.5, 0.5])                            # node 1: edges 2 and 5 tie in both channels
    return dict(x=x, ei=ei, M=8)


def memory_stack(L, seed=31):
    """Two subclassed layers F -> H -> H for the memories: a mean GraphConv body, then a GATv2 body with two heads."""
    torch.manual_seed(seed)
    return L.GraphConv(MEM["F"], MEM["H"], aggr="mean"), L.GATv2(MEM["H"], MEM["H"] // 2, heads=2)
