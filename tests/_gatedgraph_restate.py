"""Eager restatement of PyG's GatedGraphConv (Li et al., Gated Graph Sequence Neural Networks) and of its dense form
(the contract gcm.nn's layers implement), dtype generic so the tests can evaluate it in float64 to bound the kernels'
fp32 error.  Written from the formulas:
    h_0 = x zero-padded on the right to C columns
    p = h_l @ weight[l];  m_i = sum_{j -> i} a_ij p_j
    gi = m W_ih^T + b_ih;  gh = h_l W_hh^T + b_hh                     (gate order r, z, n)
    r = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z);  n = tanh(gi_n + r * gh_n)
    h_{l+1} = (1 - z) * n + z * h_l;  out = h_L"""
import torch

WIDTH_ERROR = "The number of input channels is not allowed to be larger than the number of output channels"


def gru(m, h, w_ih, w_hh, b_ih=None, b_hh=None):
    """One GRU cell update of the state h by the input m."""
    C = h.shape[-1]
    gi, gh = m @ w_ih.t(), h @ w_hh.t()
    if b_ih is not None:
        gi = gi + b_ih
    if b_hh is not None:
        gh = gh + b_hh
    r = torch.sigmoid(gi[..., :C] + gh[..., :C])
    z = torch.sigmoid(gi[..., C:2 * C] + gh[..., C:2 * C])
    n = torch.tanh(gi[..., 2 * C:] + r * gh[..., 2 * C:])
    return (1 - z) * n + z * h


def pad(x, C):
    if x.shape[-1] > C:
        raise ValueError(WIDTH_ERROR)
    return torch.cat([x, x.new_zeros(*x.shape[:-1], C - x.shape[-1])], -1)


def dense_adjacency(adj, B, N, add_loop):
    """adj broadcast to [B, N, N], the diagonal overwritten with 1 when add_loop."""
    adj = adj.unsqueeze(0) if adj.dim() == 2 else adj
    A = adj.expand(B, N, N)
    if add_loop:
        A = torch.where(torch.eye(N, dtype=torch.bool), torch.ones_like(A), A)
    return A


def dense_gatedgraph(x, adj, weight, w_ih, w_hh, b_ih=None, b_hh=None, mask=None, add_loop=False):
    """adj[b, i, j]: the weight of the edge j -> i (0: no edge); add_loop overwrites the diagonal with 1."""
    x = x.unsqueeze(0) if x.dim() == 2 else x
    B, N, _ = x.shape
    A = dense_adjacency(adj, B, N, add_loop)
    h = pad(x, weight.shape[-1])
    for l in range(weight.shape[0]):
        h = gru(A @ (h @ weight[l]), h, w_ih, w_hh, b_ih, b_hh)
    if mask is not None:
        h = h * mask.view(B, N, 1).to(h.dtype)
    return h


def dense_gatedgraph_adj_grad(x, adj, g_out, weight, w_ih, w_hh, b_ih=None, b_hh=None, add_loop=False):
    """The stated gradient of the adjacency: g_adj[b,i,j] = sum_l <g_m_l[b,i,:], p_l[b,j,:]>, the diagonal zeroed
    when add_loop; g_m_l: the gradient autograd gives m_l with the adjacency held constant."""
    B, N, _ = x.shape
    A = dense_adjacency(adj.detach(), B, N, add_loop)
    h = pad(x.detach().requires_grad_(), weight.shape[-1])
    ms, ps = [], []
    for l in range(weight.shape[0]):
        p = h @ weight[l]
        m = A @ p
        m.retain_grad()
        ms.append(m)
        ps.append(p.detach())
        h = gru(m, h, w_ih, w_hh, b_ih, b_hh)
    h.backward(g_out)
    g = sum(m.grad @ p.transpose(1, 2) for m, p in zip(ms, ps))
    if add_loop:
        g = g * (1 - torch.eye(N, dtype=g.dtype))
    return g


def gatedgraph(x, edge_index, weight, w_ih, w_hh, b_ih=None, b_hh=None, edge_weight=None):
    """edge_index [2, E] = (source, sink), used as given: no loop is added or removed, duplicates are separate
    terms.  A weight vector of the wrong length is ignored (GraphConv's rule)."""
    src, dst = edge_index[0], edge_index[1]
    if edge_weight is not None and edge_weight.numel() != src.numel():
        edge_weight = None
    h = pad(x, weight.shape[-1])
    for l in range(weight.shape[0]):
        msg = (h @ weight[l])[src]
        if edge_weight is not None:
            msg = msg * edge_weight.view(-1, 1).to(msg.dtype)
        h = gru(torch.zeros_like(h).index_add(0, dst, msg), h, w_ih, w_hh, b_ih, b_hh)
    return h


class _GatedRefBase(torch.nn.Module):
    """Parameter layout of the gcm.nn layers and of PyG: weight [L, C, C] and rnn, a torch.nn.GRUCell whose forward
    is not used."""

    def __init__(self, out_channels, num_layers, bias=True):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(num_layers, out_channels, out_channels))
        self.rnn = torch.nn.GRUCell(out_channels, out_channels, bias=bias)
        torch.nn.init.uniform_(self.weight, -out_channels ** -0.5, out_channels ** -0.5)

    def _operands(self):
        return (self.weight, self.rnn.weight_ih, self.rnn.weight_hh, getattr(self.rnn, "bias_ih", None),
                getattr(self.rnn, "bias_hh", None))


class DenseGatedRef(_GatedRefBase):
    def forward(self, x, adj, mask=None, add_loop=False):
        return dense_gatedgraph(x, adj, *self._operands(), mask=mask, add_loop=add_loop)


class GatedRef(_GatedRefBase):
    def forward(self, x, edge_index, edge_weight=None):
        return gatedgraph(x, edge_index, *self._operands(), edge_weight=edge_weight)


def lively(conv):
    """Parameters off their init, so the gates are not all near 1/2: the biases drawn from U(-0.5, 0.5), the cell's
    weights doubled."""
    with torch.no_grad():
        for name, p in conv.rnn.named_parameters():
            if name.startswith("bias"):
                p.uniform_(-0.5, 0.5)
            else:
                p.mul_(2.0)
    return conv
