"""The cases of tests/test_edgeconv_gpu.py, built on the CPU from seeds.  The CPU suite (tests/test_edgeconv_cpu.py)
checks on the same tensors the two conditions under which an fp32 run must pick the float64 winners: evaluated in
float64, no (sink, channel) has its two best messages closer than GAP, and no set entry has a pre-activation within
KINK of the activation's kink.  x is standard normal, W1 ~ N(0, 1/2F), W2 ~ N(0, 1/H), biases 0.1 N(0, 1)."""
import torch

from _edgeconv_restate import make_nn

GAP = 2e-5          # 10x the largest fp32-vs-float64 output error seen on these shapes (2e-6)
KINK = 1e-5         # tests/_gen_cases.py's value: |pre| below this may sit on the other side of the kink in fp32

HOPS = (1, 2, 4)

#  name: (B, N, F, H, C), pattern, act, bias, seed   (the seed: the first of 0, 1, 2, .. that meets both conditions)
DENSE = {
    "D1": ((2, 8, 6, 8, 5), "random40", "relu", True, 0),            # one empty row and one diagonal entry forced
    "D2": ((2, 33, 12, 16, 9), "random30", "relu", True, 0),         # one past a 32-tile
    "D3": ((1, 130, 32, 32, 32), "hops+2", "relu", True, 0),         # N past 128
    "D4": ((3, 16, 32, 64, 32), "lower", "relu", True, 0),           # the DenseEdge pattern
    "D5": ((2, 70, 7, 33, 3), "hops+5", "relu", True, 0),            # widths no multiples of 4, H one past a tile
    "D6": ((1, 9, 128, 128, 128), "hops", "relu", True, 0),          # the width limit
    "D2-leaky": ((2, 33, 12, 16, 9), "random30", "leaky", True, 0),  # LeakyReLU(0.2)
    "D2-nobias": ((2, 33, 12, 16, 9), "random30", "relu", False, 0), # bias=False on both linears
}
CSR_EXTRA = "S7"    # duplicate edges, self edges and isolated nodes
S7 = ((1, 40, 6, 16, 8), "leaky", True, 0)
CSR = list(DENSE) + [CSR_EXTRA]


def pattern(kind, B, N, gen):
    adj = torch.zeros(B, N, N)
    if kind.startswith("random"):
        adj = (torch.rand(B, N, N, generator=gen) < int(kind[6:]) / 100).float()
        if kind == "random40":
            adj[:, 3, :] = 0          # an empty row
            adj[:, 5, 5] = 1          # a diagonal entry
    elif kind == "lower":
        adj = torch.tril(torch.ones(N, N), -1).expand(B, N, N).clone()
    else:
        for i in range(N):
            for h in HOPS:
                if i - h >= 0:
                    adj[:, i, i - h] = 1
        extra = int(kind[5:]) if kind.startswith("hops+") else 0
        for b in range(B):
            for i in range(1, N):
                for _ in range(extra):
                    adj[b, i, int(torch.randint(0, i, (1,), generator=gen))] = 1
    return adj


def dense_case(name, seed=None):
    """-> dict(nn, x [B,N,F], adj [B,N,N], g [B,N,C] (the output's gradient))."""
    (B, N, F, H, C), kind, act, bias, s = DENSE[name]
    gen = torch.Generator().manual_seed(s if seed is None else seed)
    torch.manual_seed(1000 + (s if seed is None else seed))
    nn = make_nn(F, H, C, act, bias)
    x = torch.randn(B, N, F, generator=gen)
    adj = pattern(kind, B, N, gen)
    return dict(nn=nn, x=x, adj=adj, g=torch.randn(B, N, C, generator=gen))


def extra_edges(M, gen):
    """An edge list with duplicate edges, self edges and isolated nodes (the last 3), unsorted."""
    ei = torch.randint(0, M - 3, (2, 3 * M), generator=gen)
    more = torch.tensor([[0, 1, 0, 2, 1, 7, 7], [0, 2, 0, 2, 2, 9, 9]])      # loops (0,0) x2, (2,2); 1 -> 2 x2; 7 -> 9 x2
    return torch.cat([ei[:, :M], more, ei[:, M:]], 1)


def csr_case(name, seed=None):
    """-> dict(nn, x [M,F], ei [2,E] (source, sink), g [M,C]): the twin of the dense case with the same edge set
    (adj[b,i,j]: edge j -> i, in (b, i, j) order), or the extra case."""
    if name == CSR_EXTRA:
        (B, M, F, H, C), act, bias, s = S7
        gen = torch.Generator().manual_seed(s if seed is None else seed)
        torch.manual_seed(1000 + (s if seed is None else seed))
        nn = make_nn(F, H, C, act, bias)
        return dict(nn=nn, x=torch.randn(M, F, generator=gen), ei=extra_edges(M, gen),
                    g=torch.randn(M, C, generator=gen))
    c = dense_case(name, seed)
    B, N, F = c["x"].shape
    bb, ii, jj = c["adj"].nonzero(as_tuple=True)
    return dict(nn=c["nn"], x=c["x"].reshape(B * N, F), ei=torch.stack([bb * N + jj, bb * N + ii]),
                g=c["g"].reshape(B * N, -1))


# ---- the memories: B 3, N 8, F 6, T 11 (past graph_size: the overflow is crossed) ----
MEM = dict(B=3, N=8, F=6, H=8, T=11)


def memory_obs():
    """Columns 0..2 on the integer grid 0..3 (KNNEdge's distances are exact sums, ties go to the lower index in
    every precision), the others random."""
    g = torch.Generator().manual_seed(31)
    obs = torch.rand(MEM["T"], MEM["B"], MEM["F"], generator=g)
    obs[:, :, :3] = torch.randint(0, 4, (MEM["T"], MEM["B"], 3), generator=g).float()
    return obs


def memory_nns():
    """The MLPs of two layers F -> H -> H (hidden width H)."""
    torch.manual_seed(32)
    return make_nn(MEM["F"], MEM["H"], MEM["H"], "relu"), make_nn(MEM["H"], MEM["H"], MEM["H"], "leaky")
