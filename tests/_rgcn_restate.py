"""Eager restatement of the relational GCN (Schlichtkrull et al.; PyG's RGCNConv) on a dense adjacency with a relation
plane and on an edge list, and of the TypedEdge selector over oracle.dense's selectors - the contract gcm.nn's
DenseRGCNConv / RGCNConv and gcm.edge_selectors.typed.TypedEdge implement.  dtype generic, so the tests evaluate it in
float64 to bound the kernels' fp32 error (tests/_gcn_restate.py's rule)."""
import torch


def bits(rel, R):
    """[R, ...] planes of the low R bits of the codes; codes <= 0 have none."""
    r = rel.clamp(min=0).to(torch.int64)
    return torch.stack([(r >> k) & 1 for k in range(R)], 0)


def compose(weight, comp):
    """[R, Fin, Fout]: the weights themselves, or comp . weight with bases (PyG)."""
    if comp is None:
        return weight
    return (comp @ weight.reshape(weight.shape[0], -1)).view(comp.shape[0], weight.shape[1], weight.shape[2])


def dense_rgcn(x, adj, rel, weight, root=None, bias=None, aggr="mean", mask=None, comp=None):
    """out[b,i] = sum_r s_r(b,i) sum_j m_r[b,i,j] adj[b,i,j] x[b,j] W_r + x[b,i] root + bias; s_r = 1 / max(1, count
    of the PATTERN m_r) for the mean.  adj enters only where a bit is set (torch.where: no 0 * inf)."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    rel = rel.unsqueeze(0) if rel.dim() == 2 else rel
    B, N, _ = x.shape
    adj, rel = adj.expand(B, N, N), rel.expand(B, N, N)
    W = compose(weight, comp)
    R = W.shape[0]
    m = bits(rel, R)
    out = x @ root if root is not None else x.new_zeros(B, N, W.shape[2])
    for r in range(R):
        a = torch.where(m[r] > 0, adj, torch.zeros_like(adj))
        agg = a @ x
        if aggr == "mean":
            agg = agg / m[r].sum(-1, keepdim=True).clamp(min=1).to(x.dtype)
        out = out + agg @ W[r]
    if bias is not None:
        out = out + bias
    if mask is not None:
        out = out * mask.view(B, N, 1).to(out.dtype)
    return out


def sparse_rgcn(x, edge_index, edge_type, weight, root=None, bias=None, aggr="mean", mask_mode=False, comp=None):
    """edge_index [2,E] = (source, sink); edge_type [E]: relation ids (an id outside [0, R) contributes nothing) or,
    in mask_mode, bit codes.  Duplicates count separately."""
    W = compose(weight, comp)
    R, M = W.shape[0], x.shape[0]
    out = x @ root if root is not None else x.new_zeros(M, W.shape[2])
    src, dst = edge_index[0], edge_index[1]
    et = edge_type.clamp(min=0).to(torch.int64) if mask_mode else edge_type
    for r in range(R):
        sel = ((et >> r) & 1) > 0 if mask_mode else (et == r)
        agg = x.new_zeros(M, x.shape[1]).index_add(0, dst[sel], x[src[sel]])
        if aggr == "mean":
            cnt = x.new_zeros(M).index_add(0, dst[sel], x.new_ones(int(sel.sum())))
            agg = agg / cnt.clamp(min=1)[:, None]
        out = out + agg @ W[r]
    return out if bias is None else out + bias


class RGCNRef(torch.nn.Module):
    """Parameter layout of gcm.nn.DenseRGCNConv / RGCNConv (weight, comp, root, bias): loads their state_dict."""

    def __init__(self, cin, cout, num_relations, num_bases=None, aggr="mean", root_weight=True, bias=True):
        super().__init__()
        self.aggr = aggr
        P = torch.nn.Parameter
        self.weight = P(torch.zeros(num_bases or num_relations, cin, cout))
        self.comp = P(torch.zeros(num_relations, num_bases)) if num_bases else None
        self.root = P(torch.zeros(cin, cout)) if root_weight else None
        self.bias = P(torch.zeros(cout)) if bias else None

    def forward(self, x, adj, rel, mask=None):
        return dense_rgcn(x, adj, rel, self.weight, self.root, self.bias, self.aggr, mask, self.comp)

    def sparse(self, x, edge_index, edge_type, mask_mode=False):
        return sparse_rgcn(x, edge_index, edge_type, self.weight, self.root, self.bias, self.aggr, mask_mode, self.comp)


def diff_or(tensors):
    res = torch.zeros_like(tensors[0])
    for t in tensors:
        res = res + t - res * t
    return res


class TypedEdge:
    """Every child (an oracle.dense selector) on a zero adjacency and a zero-size weights tensor; adj_out = diff_or of
    adj and the selections, rel_out = rel | sum_k 2^relations[k] [a_k > 0]."""

    def __init__(self, selectors, relations=None):
        self.selectors = list(selectors)
        self.relations = list(range(len(self.selectors))) if relations is None else list(relations)
        self.num_relations = max(self.relations) + 1

    def __call__(self, nodes, adj, weights, num_nodes, B):
        assert weights.shape == adj.shape
        picked = [s(nodes, torch.zeros_like(adj), weights.new_zeros(0), num_nodes, B)[0] for s in self.selectors]
        code = weights.detach().to(torch.int64)
        for r, a in zip(self.relations, picked):
            code = code | ((a.detach() > 0).to(torch.int64) << r)
        return diff_or([adj] + picked), code.to(weights.dtype)


def bridge_edges(rel):
    """The edge list DenseToSparse(transpose=True) gives for a plane [B,N,N]: entry (b,i,j) > 0 -> edge (bN+j -> bN+i)
    -> (edge_index [2,E], the codes [E])."""
    B, N, _ = rel.shape
    b, i, j = torch.nonzero(rel > 0).t()
    return torch.stack([b * N + j, b * N + i]), rel[b, i, j]
