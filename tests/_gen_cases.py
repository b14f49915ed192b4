"""The cases of tests/test_gen_gpu.py, built on the CPU from seeds: the CPU suite (tests/test_gen_cpu.py) checks on the
same tensors that no case has an entry of xs = lin_src(x) on relu's kink, the GPU suite then compares every entry."""
import torch

from _gen_restate import DenseGENRef, GENRef

KINK = 1e-5         # |xs| below this in float64: an fp32 lin_src may put it on the other side of relu's kink

#          B,  N,   C, options
DENSE = [
    (3, 7, 3, {}),                                            # sub-tile
    (5, 1, 4, {}),                                            # a single node
    (3, 33, 8, {"mask": True}),                               # one past a tile
    (2, 40, 16, {"cin": 10}),                                 # in != out: lin_src / lin_dst
    # several row blocks; the values of adj must not matter.  The aggregation alone: behind it the mlp's last weight
    # gradient is a library GEMM over 1200 rows, whose own fp32 chain is beyond 3x the CPU's (measured with the
    # float64 restatement's activations as its input: 1.65e-4 on the GPU, 3.4e-5 on the CPU, at a scale of 138) - an
    # error of that GEMM, not of the kernels under test, as tests/test_gin_gpu.py notes for its cfg2 case
    (4, 300, 64, {"weighted": True, "mlp": False}),
    (2, 20, 128, {}),                                         # the widest
    (1, 20, 6, {"two_d": True}),                              # [N,F] / [N,N] inputs
    (4, 20, 6, {"bcast": True}),                              # [1,N,N] adjacency
    (2, 9, 5, {"density": 0.0}),                              # all-zero adjacency
    (2, 9, 5, {"density": 1.1}),                              # a full one
    (3, 12, 8, {"cin": 5, "msg_norm": True}),                 # message norm, fixed scale
    # (seeded apart from the shape: with the shape's own seed the t gradient is a sum of 288 terms that cancels to
    #  0.4 and the restatement's fp32 run happens to land 6.6e-8 from float64, a bound of 2.0e-7 that the fp32
    #  gradients arriving from torch's backward alone exceed - measured 2.03e-7.  Over the seeds 1000..1011 the
    #  error is 0.00 to 0.66 of the bound; the first of them is used)
    (3, 12, 8, {"msg_norm": True, "learn_msg_scale": True, "norm": "layer", "seed": 1000}),
    (3, 12, 8, {"t": 0.0}),                                   # the mean
    (3, 12, 8, {"t": -2.0}),                                  # towards the min
]

#        M,   E,    C, options
CSR = [
    (40, 90, 8, {}),
    (5, 0, 4, {}),                                            # no edges
    (300, 1500, 32, {"cin": 20}),
    (129, 700, 128, {}),
    (64, 2000, 16, {}),                                       # high degree with duplicates
    (40, 90, 8, {"cin": 5, "msg_norm": True, "learn_msg_scale": True, "norm": "layer"}),
    (40, 90, 8, {"t": 0.0}),
    (40, 90, 8, {"t": -2.0}),
]


def _ref(cls, cin, C, opts):
    return cls(cin, C, t=opts.get("t", 1.0), learn_t=True, msg_norm=opts.get("msg_norm", False),
               learn_msg_scale=opts.get("learn_msg_scale", False), norm=opts.get("norm"), bias=True)


def dense_case(B, N, C, opts):
    """-> dict(ref, x [B,N,cin], xs [B,N,C] (operand of the aggregation alone), adj, mask, g, ga)."""
    torch.manual_seed(opts.get("seed", B * 1000 + N + C))
    cin = opts.get("cin", C)
    ref = _ref(DenseGENRef, cin, C, opts)
    x, xs = torch.randn(B, N, cin), torch.randn(B, N, C)
    nb = 1 if opts.get("bcast") else B
    adj = (torch.rand(nb, N, N) < opts.get("density", 0.3)).float()
    if opts.get("weighted"):
        adj = adj * (torch.rand(nb, N, N) * 4 - 2)            # any nonzero value, negative ones too, is "set"
    mask = (torch.rand(B, N) < 0.7) if opts.get("mask") else None
    if opts.get("two_d"):
        x, adj = x[0], adj[0]
    return dict(ref=ref, x=x, xs=xs, adj=adj, mask=mask, g=torch.randn(B, N, C), ga=torch.randn(B, N, C))


def edges(M, E, seed, loops=True):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, max(1, M - 3), (2, E), generator=gen)     # the last 3 nodes stay isolated
    if E and loops:
        extra = torch.tensor([[0, 1, 0, 2, 1], [0, 2, 0, 2, 2]])     # duplicate loops (0, 0), duplicate edge 1 -> 2
        ei = torch.cat([ei[:, : E // 2], extra, ei[:, E // 2:]], 1)
    return ei


def csr_case(M, E, C, opts):
    torch.manual_seed(opts.get("seed", M + E + C))
    cin = opts.get("cin", C)
    ref = _ref(GENRef, cin, C, opts)
    return dict(ref=ref, x=torch.randn(M, cin), xs=torch.randn(M, C), ei=edges(M, E, seed=M + E),
                g=torch.randn(M, C), ga=torch.randn(M, C))


def shift_case(C=8):
    """Node 0 holds 10.0 in every channel, the others U[0,1); t = 40: logits reach 400, and rows 3.. aggregate only
    from nodes >= 1 - a graph-wide shift by 400 underflows every term of theirs (exp(-360) = 0 in fp32)."""
    torch.manual_seed(40)
    N = 12
    x = torch.rand(N, C)
    x[0] = 10.0
    adj = (torch.rand(N, N) < 0.4).float()
    adj[:, 0] = 0
    adj[1, 0] = adj[2, 0] = adj[2, 5] = 1                     # rows 1, 2 see node 0; row 2 another one beside it
    adj[3:, 1] = 1                                            # every other row has at least one neighbour >= 1
    adj[N - 1] = 0                                            # and one row is empty
    ii, jj = adj.nonzero(as_tuple=True)
    return dict(x=x, adj=adj, ei=torch.stack([jj, ii]), t=40.0, g=torch.randn(N, C))


# ---- the memories: B 3, N 8, F 4, T 12 (past graph_size: the wrap is crossed) ----
MEM = dict(B=3, N=8, F=4, H=8, T=12)


def memory_obs():
    """Columns 0..2 on the integer grid 0..3 (KNNEdge's distances are exact sums, ties go to the lower index in
    every precision), column 3 random."""
    g = torch.Generator().manual_seed(21)
    obs = torch.rand(MEM["T"], MEM["B"], MEM["F"], generator=g)
    obs[:, :, :3] = torch.randint(0, 4, (MEM["T"], MEM["B"], 3), generator=g).float()
    return obs


def memory_layers(cls):
    """Two layers F -> H -> H, norm=None, a learnt t each; lin_src has no bias, so the zero rows of a memory give
    xs = 0 exactly in every precision."""
    torch.manual_seed(22)
    return (cls(MEM["F"], MEM["H"], t=1.5, learn_t=True, norm=None, bias=False),
            cls(MEM["H"], MEM["H"], t=0.5, learn_t=True, norm=None, bias=False))


def kink_entries(ref, x):
    """Number of entries of xs = lin_src(x), evaluated in float64, within KINK of zero (exact zeros of all-zero rows
    aside: they are zero in every precision)."""
    if ref.in_channels == ref.out_channels:
        return 0
    r = ref.lin_src
    xs = torch.nn.functional.linear(x.double(), r.weight.double(), None if r.bias is None else r.bias.double())
    live = (x != 0).any(-1, keepdim=True) | (r.bias is not None)
    return int(((xs.abs() < KINK) & live).sum())
