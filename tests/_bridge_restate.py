"""Torch-only restatement of the dense <-> sparse bridge, the comparison side of tests/test_bridge_*.py.

DenseToSparse follows the reference's module line by line (src/gcm/gcm.py:24-53: torch.nonzero(adj > 0), rows and
columns offset by b*N, edge_index = (row, col)), with the two additions of gcm.gcm.DenseToSparse spelled out: the
swapped orientation and the gathered edge values.  SparseToDense (src/gcm/gcm.py:10-21) calls PyG's to_dense_batch and
to_dense_adj with max_num_nodes=N; torch_geometric is not installed beside this package, so their documented
semantics are restated: node m of graph b = batch[m] sits at position m - (first node of b), positions >= N are
dropped, absent rows are 0, and adj[b, source position, sink position] sums the weights (1 without weights) of the
edges, duplicates included.  dtype generic: where values are involved the tests evaluate it in float64."""
import torch


def dense_to_sparse(x, adj, transpose=False, edge_values=False):
    """-> (x_sp [B*N,F], edge_index [2,E] int64, batch_idx [B*N] int64[, edge_weight [E] in adj's dtype])."""
    assert x.dim() == adj.dim() == 3
    B, N = x.shape[0], x.shape[1]
    offset, row, col = torch.nonzero(adj > 0).t()               # gcm.py:44: (b, r, c) order, strict comparison
    values = adj[offset, row, col]
    row = row + offset * N                                      # gcm.py:45-46
    col = col + offset * N
    edge_index = torch.stack([col, row] if transpose else [row, col], dim=0).long()     # gcm.py:47
    x_sp = x.reshape(B * N, x.shape[-1])                        # gcm.py:48
    batch_idx = torch.arange(0, B).view(-1, 1).repeat(1, N).view(-1)                    # gcm.py:49-51
    if edge_values:
        return x_sp, edge_index, batch_idx, values
    return x_sp, edge_index, batch_idx


def places(batch_idx, B, N):
    """(position of each node in its graph, whether it has a place in [B, N]) for a non-decreasing batch_idx."""
    M = batch_idx.numel()
    first = torch.zeros(B + 1, dtype=torch.long)
    first[1:] = torch.cumsum(torch.bincount(batch_idx, minlength=B)[:B], 0)
    pos = torch.arange(M) - first[batch_idx]
    return pos, pos < N


def sparse_to_dense(x_sp, edge_index, batch_idx, B, N, edge_weight=None):
    """-> (x [B,N,F] in x_sp's dtype, adj [B,N,N] in edge_weight's dtype, float32 without weights).  Differentiable
    in x_sp and edge_weight (index_put; the sum of duplicates runs in list order on the CPU)."""
    pos, keep = places(batch_idx, B, N)
    x = torch.zeros(B, N, x_sp.shape[1], dtype=x_sp.dtype).index_put((batch_idx[keep], pos[keep]), x_sp[keep])
    src, dst = edge_index[0], edge_index[1]
    ok = keep[src] & keep[dst] & (batch_idx[src] == batch_idx[dst])
    w = torch.ones(src.numel()) if edge_weight is None else edge_weight
    adj = torch.zeros(B, N, N, dtype=w.dtype).index_put((batch_idx[src][ok], pos[src][ok], pos[dst][ok]), w[ok],
                                                        accumulate=True)
    return x, adj


def dense_adj_loop(edge_index, batch_idx, B, N, edge_weight=None):
    """The adjacency of sparse_to_dense once more, edge by edge in plain Python (float64): what the vectorised form
    above is checked against."""
    pos, keep = places(batch_idx, B, N)
    adj = torch.zeros(B, N, N, dtype=torch.float64)
    batch, pos, keep = batch_idx.tolist(), pos.tolist(), keep.tolist()
    w = [1.0] * edge_index.shape[1] if edge_weight is None else edge_weight.double().tolist()
    for e, (s, d) in enumerate(edge_index.t().tolist()):
        if keep[s] and keep[d] and batch[s] == batch[d]:
            adj[batch[s], pos[s], pos[d]] += w[e]
    return adj


# ---- adjacency patterns of the tests ---------------------------------------------------------------------------------
PATTERNS = ("empty", "full", "random", "single", "values", "int64")
SHAPES = [(1, 1), (5, 10), (3, 64), (2, 65), (2, 130), (2500, 3)]


def pattern(kind, B, N, seed=0):
    """adj [B,N,N] of one of PATTERNS: float32, int64 for "int64" (entries in {-1, 0, 1, 3})."""
    gen = torch.Generator().manual_seed(7919 * B + 31 * N + seed)
    if kind == "empty":
        return torch.zeros(B, N, N)
    if kind == "full":
        return torch.ones(B, N, N)
    if kind == "random":
        return (torch.rand(B, N, N, generator=gen) < 0.3).float()
    if kind == "single":
        adj = torch.zeros(B, N, N)
        adj[B - 1, N - 1, N - 1] = 1.0
        return adj
    pick = torch.randint(0, 4, (B, N, N), generator=gen)
    if kind == "values":
        return torch.tensor([-1.0, 0.0, 0.5, 2.0])[pick]
    assert kind == "int64"
    return torch.tensor([-1, 0, 1, 3])[pick]
