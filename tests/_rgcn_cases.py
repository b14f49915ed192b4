"""The case tables of tests/test_rgcn_gpu.py and their operands, built on the CPU from a seed.  tests/test_rgcn_cpu.py
asserts what each case claims to contain (features()) and that its output is large against its bound."""
import torch

from _rgcn_restate import bits

# (B, N, Fin, Fout, R, opts): the smallest shapes where a tile, a bit or a count can go wrong
DENSE = [
    (3, 7, 3, 5, 1, {}),
    (3, 7, 3, 5, 3, {}),
    (5, 1, 4, 3, 2, {}),
    (2, 33, 8, 8, 2, {"mask": True}),
    (2, 70, 16, 12, 5, {}),                    # N > 64
    (1, 130, 6, 9, 3, {}),                     # N > 128: two row blocks
    (2, 40, 128, 128, 2, {}),                  # the width limit
    (2, 24, 16, 24, 16, {"bit15": True}),      # R at its limit, bit 15 in use
    # options, each on a small case
    (2, 9, 4, 5, 3, {"aggr": "add"}),
    (2, 9, 4, 5, 3, {"num_bases": 2}),
    (2, 9, 4, 5, 3, {"root_weight": False}),
    (2, 9, 4, 5, 3, {"bias": False}),
    (2, 9, 4, 5, 3, {"root_weight": False, "bias": False, "aggr": "sum"}),
    (1, 9, 4, 5, 3, {"two_d": True}),
    (3, 9, 4, 5, 3, {"bcast": True}),
    (2, 12, 4, 5, 3, {"weighted": True}),      # adj values other than 0 / 1, negative ones too, with a gradient
    (2, 12, 4, 5, 3, {"no_adj_grad": True}),
    (2, 12, 4, 5, 3, {"empty_relation": True}),
    (2, 12, 4, 5, 2, {"empty_rows": True}),
    (2, 12, 4, 5, 3, {"triple": True}),
    (2, 12, 4, 5, 3, {"high_bits": True, "weighted": True}),
    (2, 12, 4, 5, 3, {"int64": True, "high_bits": True}),
]

_LAYER_KEYS = ("aggr", "num_bases", "root_weight", "bias")


def layer_kwargs(opts):
    return {k: opts[k] for k in _LAYER_KEYS if k in opts}


def dense_id(case):
    B, N, Fi, Fo, R, opts = case
    return f"{B}x{N}x{Fi}x{Fo}xR{R}" + "".join("-" + k for k in opts)


def dense_operands(case):
    """-> dict(x, adj, rel, mask, g): CPU float32 tensors (rel int64 with "int64"), 2-D / [1,N,N] forms applied."""
    B, N, Fi, Fo, R, opts = case
    torch.manual_seed(1000 * B + 10 * N + Fi + 7 * R + 31 * len(opts))
    nb = 1 if opts.get("bcast") else B
    p = 0.9 if N == 1 else max(0.2, min(0.6, 4.0 / N))
    m = (torch.rand(R, nb, N, N) < p).long()
    if opts.get("empty_relation"):
        m[1] = 0
    if opts.get("empty_rows"):                 # the even rows: nothing in relation 0, something in relation 1
        m[0, :, 0::2, :] = 0
        m[1, :, 0::2, 1] = 1
    if opts.get("triple"):
        m[:3, :, 2, 3] = 1
    if opts.get("bit15"):
        m[15, :, 1, 2] = 1
    rel = sum(m[r] << r for r in range(R))
    adj = (rel > 0).float()
    if opts.get("weighted"):                   # weights on the pattern, and stray values off it that must not enter
        adj = torch.randn(nb, N, N)
    if opts.get("high_bits"):
        hi = (torch.rand(nb, N, N) < 0.5).long() * ((1 << R) | (1 << (R + 2)))
        rel = rel | hi                         # bits >= R: ignored, also where no low bit is set
        rel[:, 0, 0], rel[:, 0, 1] = -3, 0     # non-positive codes: no edge
        if not opts.get("weighted"):
            adj = (rel > 0).float()
    x = torch.randn(B, N, Fi)
    mask = (torch.rand(B, N) < 0.7) if opts.get("mask") else None
    g = torch.randn(B, N, Fo)
    rel = rel if opts.get("int64") else rel.float()
    if opts.get("two_d"):
        x, adj, rel = x[0], adj[0], rel[0]
    return {"x": x, "adj": adj, "rel": rel, "mask": mask, "g": g}


def dense_features(case, ops):
    """What the operands of a case really contain, by the names the table uses."""
    B, N, Fi, Fo, R, opts = case
    rel = ops["rel"].reshape(-1, N, N)
    m = bits(rel, R)
    cnt = m.sum(-1)                            # [R, nb, N]
    got = set()
    if ops["mask"] is not None and not bool(ops["mask"].all()):
        got.add("mask")
    if ops["x"].dim() == 2:
        got.add("two_d")
    if rel.shape[0] == 1 and B > 1:
        got.add("bcast")
    adj = ops["adj"].reshape(-1, N, N)
    on = (rel > 0) & (m.sum(0) > 0)
    if bool((adj[on] < 0).any()) and bool(((adj[on] != 0) & (adj[on] != 1)).any()):
        got.add("weighted")
    if any(int(m[r].sum()) == 0 for r in range(R)):
        got.add("empty_relation")
    if R >= 2 and bool(((cnt[0] == 0) & (cnt[1] > 0)).any()):
        got.add("empty_rows")
    if bool((m.sum(0) >= 3).any()):
        got.add("triple")
    if bool(((rel.long().clamp(min=0) >> R) > 0).any()) and bool((rel < 0).any()) and bool((rel == 0).any()):
        got.add("high_bits")
    if rel.dtype == torch.int64:
        got.add("int64")
    if R == 16 and int(m[15].sum()) > 0:
        got.add("bit15")
    return got


# (M, E, R, opts)
SPARSE = [
    (9, 0, 2, {}),
    (20, 60, 3, {}),
    (20, 60, 3, {"out_of_range": True}),
    (300, 2000, 5, {"hub": True}),             # one sink of in-degree >= 200, duplicate edges, self loops
]


def sparse_id(case):
    M, E, R, opts = case
    return f"{M}x{E}xR{R}" + "".join("-" + k for k in opts)


def sparse_operands(case, Fi=6, Fo=5):
    """-> dict(x, edge_index, ids, codes, g)."""
    M, E, R, opts = case
    torch.manual_seed(100 * M + E + R)
    src, dst = torch.randint(0, M, (E,)), torch.randint(0, M, (E,))
    if opts.get("hub"):
        dst[:230] = 5
        src[300:350], dst[300:350] = src[250:300], dst[250:300]      # duplicates
        src[400:430] = dst[400:430]                                   # self loops
    ids = torch.randint(0, R, (E,))
    codes = torch.randint(0, 1 << R, (E,))                            # 0: in no relation
    if opts.get("hub"):
        ids[300:350], codes[300:350] = ids[250:300], codes[250:300]
    if opts.get("out_of_range"):
        ids[::7], ids[1::7], ids[2::11] = R, -1, R + 40
        codes[::5] |= (1 << R) | (1 << 15)
        codes[3::9] = -2
    return {"x": torch.randn(M, Fi), "edge_index": torch.stack([src, dst]), "ids": ids, "codes": codes,
            "g": torch.randn(M, Fo)}


def sparse_features(case, ops):
    M, E, R, opts = case
    src, dst = ops["edge_index"]
    got = set()
    if E and int(torch.bincount(dst, minlength=M).max()) >= 200 and bool((src == dst).any()):
        key = (src * M + dst) * 64 + ops["ids"]
        if key.unique().numel() < E:
            got.add("hub")
    ids, codes = ops["ids"], ops["codes"]
    if E and bool((ids >= R).any()) and bool((ids < 0).any()) and bool((codes >> R > 0).any()) and bool((codes < 0).any()):
        got.add("out_of_range")
    return got
