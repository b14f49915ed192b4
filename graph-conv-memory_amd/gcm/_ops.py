"""torch.autograd wrappers around the C-ABI kernels (include/gcm_hip.h).

Every function here launches HIP kernels on torch's current stream; none of
them synchronises with the host.
"""
import ctypes

import torch

from . import _ext, _hip

_f32 = torch.float32


def _call(name, *args):
    _hip.check(getattr(_hip.lib(), name)(*args), name)


def _empty_like(t):
    return torch.empty_like(t, memory_format=torch.contiguous_format)


# ---------------------------------------------------------------------------
# DenseGCM state: insert + overflow wrap (gcm.py:262-278, 323-355)
# ---------------------------------------------------------------------------
class _StateAdvance(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nodes, adj, weights, num_nodes, x, flags):
        B, N, F = nodes.shape
        has_w = weights.numel() != 0
        nodes, adj, x = nodes.contiguous(), adj.contiguous(), x.contiguous()
        weights = weights.contiguous()
        _hip.on_device(nodes, adj, weights, num_nodes, x, flags)
        nodes_out, adj_out = _empty_like(nodes), _empty_like(adj)
        weights_out = _empty_like(weights)
        cur = torch.empty_like(num_nodes)
        nn_out = torch.empty_like(num_nodes)
        _call(
            "gcm_state_advance_fwd", _hip.ptr(nodes), _hip.ptr(adj), _hip.ptr(weights) if has_w else None,
            _hip.ptr(num_nodes), _hip.ptr(x), _hip.ptr(nodes_out), _hip.ptr(adj_out),
            _hip.ptr(weights_out) if has_w else None, _hip.ptr(cur), _hip.ptr(nn_out),
            _hip.ptr(flags), B, N, F, _hip.stream())
        ctx.save_for_backward(num_nodes)
        ctx.shape = (B, N, F)
        ctx.has_w = has_w
        ctx.mark_non_differentiable(cur, nn_out)
        if not adj.requires_grad:
            ctx.mark_non_differentiable(adj_out)
        if not weights.requires_grad:
            ctx.mark_non_differentiable(weights_out)
        return nodes_out, adj_out, weights_out, cur, nn_out

    @staticmethod
    def backward(ctx, g_nodes, g_adj, g_weights, _g_cur, _g_nn):
        (num_nodes,) = ctx.saved_tensors
        B, N, F = ctx.shape
        lib = _hip.lib()
        need_nodes, need_adj, need_w, _, need_x, _ = ctx.needs_input_grad
        dev = num_nodes.device
        if g_nodes is None:
            g_nodes = torch.zeros(B, N, F, device=dev)
        g_nodes = g_nodes.contiguous()
        g_nodes_in = torch.empty_like(g_nodes)
        g_x = torch.empty(B, F, device=dev)
        planes = []
        if need_adj and g_adj is not None:
            planes.append(("adj", g_adj.contiguous()))
        if need_w and ctx.has_w and g_weights is not None:
            planes.append(("w", g_weights.contiguous()))
        outs = {}
        first = planes[0] if planes else None
        g_plane_in = torch.empty_like(first[1]) if first else None
        rc = lib.gcm_state_advance_bwd(
            _hip.ptr(g_nodes), _hip.ptr(first[1]) if first else None, _hip.ptr(num_nodes),
            _hip.ptr(g_nodes_in), _hip.ptr(g_plane_in), _hip.ptr(g_x), B, N, F, _hip.stream())
        _hip.check(rc, "gcm_state_advance_bwd")
        if first:
            outs[first[0]] = g_plane_in
        for name, g in planes[1:]:
            scratch_n, scratch_x = torch.empty_like(g_nodes), torch.empty_like(g_x)
            gp = torch.empty_like(g)
            rc = lib.gcm_state_advance_bwd(
                _hip.ptr(g_nodes), _hip.ptr(g), _hip.ptr(num_nodes), _hip.ptr(scratch_n),
                _hip.ptr(gp), _hip.ptr(scratch_x), B, N, F, _hip.stream())
            _hip.check(rc, "gcm_state_advance_bwd")
            outs[name] = gp
        return (g_nodes_in if need_nodes else None, outs.get("adj"), outs.get("w"), None,
                g_x if need_x else None, None)


def state_advance(nodes, adj, weights, num_nodes, x, flags):
    return _StateAdvance.apply(nodes, adj, weights, num_nodes, x, flags)


# ---------------------------------------------------------------------------
# masked clear of whole graphs (an episode's end): one launch, its own backward
# ---------------------------------------------------------------------------
def _state_reset_launch(nodes, nodes_out, adj, adj_out, weights, weights_out, count, count_out, mask):
    B, N, F = nodes.shape
    has_w = weights is not None and weights.numel() != 0
    _hip.on_device(nodes, nodes_out, adj, adj_out, count, count_out, mask, *((weights, weights_out) if has_w else ()))
    _call("gcm_state_reset", _hip.ptr(nodes), _hip.ptr(nodes_out), _hip.ptr(adj), _hip.ptr(adj_out),
          _hip.ptr(weights) if has_w else None, _hip.ptr(weights_out) if has_w else None, _hip.ptr(count),
          _hip.ptr(count_out), _hip.ptr(mask), B, N, F, _hip.stream())


class _StateReset(torch.autograd.Function):
    """(nodes, adj, weights, num_nodes) with the graphs of `mask` [B] (bool) emptied - gcm_state_reset.  inplace: the
    given tensors are written (only their masked graphs) and returned, their version counters bumped (mark_dirty),
    which is what tells the cached-step chains that the state is no longer the one they advanced."""

    @staticmethod
    def forward(ctx, nodes, adj, weights, num_nodes, mask, inplace):
        has_w = weights.numel() != 0
        if inplace:
            outs = (nodes, adj, weights, num_nodes)
        else:
            nodes, adj, weights = nodes.contiguous(), adj.contiguous(), weights.contiguous()
            num_nodes = num_nodes.contiguous()
            outs = (_empty_like(nodes), _empty_like(adj), _empty_like(weights), torch.empty_like(num_nodes))
        _state_reset_launch(nodes, outs[0], adj, outs[1], weights, outs[2], num_nodes, outs[3], mask)
        if inplace:
            ctx.mark_dirty(*((nodes, adj, weights, num_nodes) if has_w else (nodes, adj, num_nodes)))
        ctx.save_for_backward(mask)
        ctx.has_w = has_w
        ctx.mark_non_differentiable(outs[3], *(o for o, need in zip(outs[:3], ctx.needs_input_grad) if not need))
        return outs

    @staticmethod
    def backward(ctx, g_nodes, g_adj, g_weights, _g_count):
        (mask,) = ctx.saved_tensors
        B = mask.shape[0]
        if g_nodes is None:      # (one of the pair carries no gradient: the kernel takes both planes)
            g_nodes = torch.zeros(B, g_adj.shape[1], 1, device=mask.device)
        if g_adj is None:
            g_adj = torch.zeros(B, g_nodes.shape[1], g_nodes.shape[1], device=mask.device)
        g_nodes, g_adj = g_nodes.contiguous(), g_adj.contiguous()
        g_weights = g_weights.contiguous() if ctx.has_w else None
        gn, ga = torch.empty_like(g_nodes), torch.empty_like(g_adj)
        gw = torch.empty_like(g_weights) if ctx.has_w else None
        _state_reset_launch(g_nodes, gn, g_adj, ga, g_weights, gw, None, None, mask)
        need = ctx.needs_input_grad
        return (gn if need[0] else None, ga if need[1] else None, gw if need[2] and ctx.has_w else None, None, None,
                None)


def state_reset(nodes, adj, weights, num_nodes, mask, inplace=False):
    return _StateReset.apply(nodes, adj, weights, num_nodes, mask, inplace)


# ---------------------------------------------------------------------------
# belief row gather + finite flag (gcm.py:309-318)
# ---------------------------------------------------------------------------
class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, cur, flags):
        feats = feats.contiguous()
        _hip.on_device(feats, cur, flags)
        B, N, H = feats.shape
        out = torch.empty(B, H, device=feats.device, dtype=_f32)
        rc = _hip.lib().gcm_gather_rows_fwd(_hip.ptr(feats), _hip.ptr(cur), _hip.ptr(out),
                                            _hip.ptr(flags), B, N, H, _hip.stream())
        _hip.check(rc, "gcm_gather_rows_fwd")
        ctx.save_for_backward(cur)
        ctx.shape = (B, N, H)
        return out

    @staticmethod
    def backward(ctx, g_out):
        (cur,) = ctx.saved_tensors
        B, N, H = ctx.shape
        g_out = g_out.contiguous()
        g_feats = torch.empty(B, N, H, device=g_out.device, dtype=_f32)
        rc = _hip.lib().gcm_gather_rows_bwd(_hip.ptr(g_out), _hip.ptr(cur), _hip.ptr(g_feats),
                                            B, N, H, _hip.stream())
        _hip.check(rc, "gcm_gather_rows_bwd")
        return g_feats, None, None


def gather_rows(feats, cur, flags):
    return _GatherRows.apply(feats, cur, flags)


# ---------------------------------------------------------------------------
# DenseGraphConv (PyG; README.md:56-62)
# ---------------------------------------------------------------------------
class _DenseGraphConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj, w_rel, b_rel, w_root, act):
        x, adj = x.contiguous(), adj.contiguous()
        w_rel, w_root = w_rel.contiguous(), w_root.contiguous()
        b_rel = None if b_rel is None else b_rel.contiguous()
        _hip.on_device(x, adj, w_rel, b_rel, w_root)
        B, N, Fi = x.shape
        Fo = w_rel.shape[0]
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert w_rel.shape == (Fo, Fi) and w_root.shape == (Fo, Fi)
        out = torch.empty(B, N, Fo, device=x.device, dtype=_f32)
        need_bwd = any(ctx.needs_input_grad)
        agg = torch.empty(B, N, Fi, device=x.device, dtype=_f32) if need_bwd else None
        _call(
            "gcm_dense_graphconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w_rel), _hip.ptr(b_rel), _hip.ptr(w_root),
            _hip.ptr(out), _hip.ptr(agg), B, N, Fi, Fo, act, _hip.stream())
        ctx.save_for_backward(x, adj, w_rel, w_root, out, agg)
        ctx.act = act
        ctx.has_bias = b_rel is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, adj, w_rel, w_root, out, agg = ctx.saved_tensors
        B, N, Fi = x.shape
        Fo = w_rel.shape[0]
        need_x, need_adj, need_wrel, need_b, need_wroot, _ = ctx.needs_input_grad
        need_b = need_b and ctx.has_bias
        g_out = _hip.kernel_ready(g_out)
        dev = x.device
        lib = _hip.lib()
        g_x = torch.empty_like(x) if need_x else None
        g_adj = torch.empty_like(adj) if need_adj else None
        g_wrel = torch.empty_like(w_rel) if need_wrel else None
        g_wroot = torch.empty_like(w_root) if need_wroot else None
        g_b = torch.empty(Fo, device=dev, dtype=_f32) if need_b else None
        ws_bytes = lib.gcm_dense_graphconv_bwd_workspace_bytes(B, N, Fi, Fo)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _call(
            "gcm_dense_graphconv_bwd", _hip.ptr(g_out), _hip.ptr(out), _hip.ptr(x), _hip.ptr(adj), _hip.ptr(agg),
            _hip.ptr(w_rel), _hip.ptr(w_root), _hip.ptr(g_x), _hip.ptr(g_adj), _hip.ptr(g_wrel),
            _hip.ptr(g_b), _hip.ptr(g_wroot), _hip.ptr(ws), ws_bytes, B, N, Fi, Fo, ctx.act,
            _hip.stream())
        return g_x, g_adj, g_wrel, g_b, g_wroot, None


def dense_graphconv(x, adj, w_rel, b_rel, w_root, act=_hip.ACT_NONE):
    return _DenseGraphConv.apply(x, adj, w_rel, b_rel, w_root, act)


# ---------------------------------------------------------------------------
# index-writing / distance selectors: in place on a fresh adjacency buffer
# ---------------------------------------------------------------------------
def edge_temporal_(adj, cur, hops, direction):
    _hip.on_device(adj, cur)
    B, N, _ = adj.shape
    arr = (ctypes.c_int32 * len(hops))(*hops)
    rc = _hip.lib().gcm_edge_temporal(_hip.ptr(adj), _hip.ptr(cur), ctypes.addressof(arr),
                                      len(hops), _hip.DIR[direction], B, N, _hip.stream())
    _hip.check(rc, "gcm_edge_temporal")
    return adj


class _TemporalWindow(torch.autograd.Function):
    """TemporalBackedge(learned=True) (temporal.py:51-70): adj[b, n_b, :n_b] += the OR of the sampled
    one-hots, in place on `adj` like the reference's slice assignment."""

    @staticmethod
    def forward(ctx, adj, window, cur, noise, S, deterministic, flags):
        window = window.contiguous()
        _hip.on_device(adj, window, cur, noise, flags)
        B, N, _ = adj.shape
        W = window.numel()
        Wn = min(W, N)
        soft = torch.empty(1 if deterministic else S, B, Wn, device=adj.device, dtype=_f32)
        scratch = torch.empty(B, Wn, device=adj.device, dtype=_f32)
        _call("gcm_temporal_window_fwd", _hip.ptr(window), _hip.ptr(noise), _hip.ptr(cur), _hip.ptr(adj),
              _hip.ptr(soft), _hip.ptr(scratch), B, N, W, S, int(deterministic), _hip.ptr(flags), _hip.stream())
        ctx.mark_dirty(adj)
        ctx.save_for_backward(soft, cur)
        ctx.cfg = (W, S, int(deterministic))
        return adj

    @staticmethod
    def backward(ctx, g_adj):
        soft, cur = ctx.saved_tensors
        W, S, det = ctx.cfg
        _, B, Wn = soft.shape
        g_adj = g_adj.contiguous()
        part = torch.empty(B, Wn, device=g_adj.device, dtype=_f32)
        _call("gcm_temporal_window_bwd", _hip.ptr(g_adj), _hip.ptr(soft), _hip.ptr(cur), _hip.ptr(part),
              B, g_adj.shape[-1], W, S, det, _hip.stream())
        g_window = part.sum(0)
        if Wn < W:
            g_window = torch.cat([g_window, g_window.new_zeros(W - Wn)])
        return g_adj, g_window, None, None, None, None, None


def temporal_window_(adj, window, cur, noise, num_samples, deterministic, flags):
    """noise: [S, B, min(W, N)] standard gumbel draws (None when deterministic)"""
    if noise is not None:
        noise = noise.contiguous()
    return _TemporalWindow.apply(adj, window, cur, noise, num_samples, deterministic, flags)


def edge_dense_(adj, cur):
    _hip.on_device(adj, cur)
    B, N, _ = adj.shape
    rc = _hip.lib().gcm_edge_dense(_hip.ptr(adj), _hip.ptr(cur), B, N, _hip.stream())
    _hip.check(rc, "gcm_edge_dense")
    return adj


def edge_distance_(nodes, adj, cur, mode, max_distance, dist_param=None, a=(0, 0), b=(0, 0),
                   bidirectional=False, want_dist=False, cur_rows=None):
    """cur_rows [n, F]: the current nodes of every rank (all-gathered) when a batch-sharded
    EuclideanEdge takes its mean over the global batch; None: the local graphs' own."""
    nodes = nodes.contiguous()
    _hip.on_device(nodes, adj, cur, dist_param, cur_rows)
    B, N, F = nodes.shape
    lib = _hip.lib()
    n_cur = 0 if cur_rows is None else cur_rows.shape[0]
    ws_bytes = lib.gcm_edge_distance_workspace_bytes(mode, max(B, n_cur), N, F)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=nodes.device)
    dist = torch.empty(B, N, device=nodes.device, dtype=_f32) if want_dist else None
    rc = lib.gcm_edge_distance_ex(_hip.ptr(nodes), _hip.ptr(adj), _hip.ptr(cur), mode,
                                  float(max_distance), _hip.ptr(dist_param), a[0], a[1], b[0], b[1],
                                  int(bidirectional), _hip.ptr(dist), _hip.ptr(cur_rows), n_cur, _hip.ptr(ws),
                                  ws_bytes, B, N, F, _hip.stream())
    _hip.check(rc, "gcm_edge_distance")
    return adj, dist


# ===========================================================================
# sparse path (sparse_gcm.py:72-212)
# ===========================================================================
_i64 = torch.int64


def _hops_arg(hops):
    return (ctypes.c_int32 * len(hops))(*hops)


def sparse_plan(T, taus):
    """-> node_off [B+1], new_off [B+1], totals [4] (all device int64); no host sync."""
    _hip.on_device(T, taus)
    B = T.numel()
    node_off = torch.empty(B + 1, dtype=_i64, device=T.device)
    new_off = torch.empty(B + 1, dtype=_i64, device=T.device)
    totals = torch.empty(4, dtype=_i64, device=T.device)
    _call("gcm_sparse_plan", _hip.ptr(T), _hip.ptr(taus), _hip.ptr(node_off), _hip.ptr(new_off),
          _hip.ptr(totals), B, _hip.stream())
    return node_off, new_off, totals


class _SparseInsert(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nodes, x, T, taus, flags):
        nodes, x = nodes.contiguous(), x.contiguous()
        _hip.on_device(nodes, x, T, taus, flags)
        B, N, F = nodes.shape
        t_pad = x.shape[1]
        out = torch.empty_like(nodes)
        _call("gcm_sparse_insert_fwd", _hip.ptr(nodes), _hip.ptr(x), _hip.ptr(T), _hip.ptr(taus),
              _hip.ptr(out), _hip.ptr(flags), B, N, F, t_pad, _hip.stream())
        ctx.save_for_backward(T, taus)
        ctx.dims = (B, N, F, t_pad)
        return out

    @staticmethod
    def backward(ctx, g_out):
        T, taus = ctx.saved_tensors
        B, N, F, t_pad = ctx.dims
        g_out = g_out.contiguous()
        g_nodes = torch.empty_like(g_out)
        g_x = torch.empty(B, t_pad, F, device=g_out.device, dtype=_f32)
        _call("gcm_sparse_insert_bwd", _hip.ptr(g_out), _hip.ptr(T), _hip.ptr(taus),
              _hip.ptr(g_nodes), _hip.ptr(g_x), B, N, F, t_pad, _hip.stream())
        return g_nodes, g_x, None, None, None


def sparse_insert(nodes, x, T, taus, flags):
    return _SparseInsert.apply(nodes, x, T, taus, flags)


def sparse_temporal_count(T, taus, hops_desc):
    """edge_off [B+1] of the TemporalEdge selector (closed form per graph); no host sync."""
    _hip.on_device(T, taus)
    B = T.numel()
    edge_off = torch.empty(B + 1, dtype=_i64, device=T.device)
    arr = _hops_arg(hops_desc)
    _call("gcm_sparse_temporal_count", _hip.ptr(T), _hip.ptr(taus), ctypes.addressof(arr),
          len(hops_desc), _hip.ptr(edge_off), B, _hip.stream())
    return edge_off


def coo_merge_segments(old_idx, old_val, new_idx, new_val, new_bptr, B, flags):
    """sparse_gcm.py:132-139 without a sort, for new entries that sort behind the stored ones of
    their graph (gcm_coo_merge_segments).  -> (idx [3, Ea+Eb], values)."""
    old_idx, new_idx = old_idx.contiguous(), new_idx.contiguous()
    Ea, Eb = old_idx.shape[1], new_idx.shape[1]
    dev = new_idx.device
    if Eb == 0:
        return old_idx, old_val
    if Ea == 0:
        return new_idx, new_val
    old_bptr = ptr_from_sorted(old_idx[0], B) if Ea else torch.zeros(B + 1, dtype=_i64, device=dev)
    if new_bptr is None:
        new_bptr = ptr_from_sorted(new_idx[0], B)
    out_idx = torch.empty(3, Ea + Eb, dtype=_i64, device=dev)
    grad = old_val.requires_grad or new_val.requires_grad
    out_val = None if grad else torch.empty(Ea + Eb, dtype=_f32, device=dev)
    perm = torch.empty(Ea + Eb, dtype=_i64, device=dev) if grad else None
    _call("gcm_coo_merge_segments", _hip.ptr(old_idx) if Ea else None, _hip.ptr(new_idx) if Eb else None,
          None if grad else _hip.ptr(old_val.contiguous()), None if grad else _hip.ptr(new_val.contiguous()),
          _hip.ptr(old_bptr), _hip.ptr(new_bptr), _hip.ptr(out_idx), _hip.ptr(out_val), _hip.ptr(perm),
          _hip.ptr(flags), Ea, Eb, B, _hip.stream())
    if grad:
        out_val = torch.cat([old_val, new_val])[perm]
    return out_idx, out_val


def sparse_temporal_edges(T, taus, hops_desc, edge_off=None, E=None):
    """COO indices [3, E] (batch, sink, source) of the TemporalEdge selector, already in
    coalesced order.  One host sync (E) unless the caller already knows E."""
    _hip.on_device(T, taus)
    B = T.numel()
    arr = _hops_arg(hops_desc)
    if edge_off is None:
        edge_off = sparse_temporal_count(T, taus, hops_desc)
    if E is None:
        E = int(edge_off[B].item())
    idx = torch.empty(3, E, dtype=_i64, device=T.device)
    _call("gcm_sparse_temporal_fill", _hip.ptr(T), _hip.ptr(taus), ctypes.addressof(arr),
          len(hops_desc), _hip.ptr(edge_off), _hip.ptr(idx), E, B, _hip.stream())
    return idx


class _SparseFlatten(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nodes, T, taus, node_off, M):
        nodes = nodes.contiguous()
        _hip.on_device(nodes, T, taus, node_off)
        B, N, F = nodes.shape
        flat = torch.empty(M, F, device=nodes.device, dtype=_f32)
        _call("gcm_sparse_flatten_fwd", _hip.ptr(nodes), _hip.ptr(T), _hip.ptr(taus),
              _hip.ptr(node_off), _hip.ptr(flat), B, N, F, M, _hip.stream())
        ctx.save_for_backward(T, taus, node_off)
        ctx.dims = (B, N, F, M)
        return flat

    @staticmethod
    def backward(ctx, g_flat):
        T, taus, node_off = ctx.saved_tensors
        B, N, F, M = ctx.dims
        g_flat = g_flat.contiguous()
        g_nodes = torch.empty(B, N, F, device=g_flat.device, dtype=_f32)
        _call("gcm_sparse_flatten_bwd", _hip.ptr(g_flat), _hip.ptr(T), _hip.ptr(taus),
              _hip.ptr(node_off), _hip.ptr(g_nodes), B, N, F, M, _hip.stream())
        return g_nodes, None, None, None, None


def sparse_flatten(nodes, T, taus, node_off, M):
    return _SparseFlatten.apply(nodes, T, taus, node_off, M)


def ptr_from_sorted(keys, M):
    keys = keys.contiguous()
    ptr = torch.empty(M + 1, dtype=_i64, device=keys.device)
    _call("gcm_ptr_from_sorted", _hip.ptr(keys), _hip.ptr(ptr), keys.numel(), M, _hip.stream())
    return ptr


class GraphIndex:
    """Device-resident index of one flat edge list: CSR by destination (forward gather) and,
    built lazily, CSC by source (backward gather).  Attached to the edge_index tensor handed
    to the GNN (attribute `gcm_graph`) so GraphConv layers share it."""

    def __init__(self, edge_index, row_ptr, M, csr_perm=None, mask=None, batches=None, col=None, csc=None):
        self.edge_index = edge_index            # [2, E] (source, sink); CSR order unless csr_perm
        self.csr_perm = csr_perm                # positions of the CSR entries in edge_index
        self.row_ptr, self.M, self.mask = row_ptr, M, mask
        # (node_off [B+1], B, max nodes per graph) when the list is grouped by graph and no edge
        # leaves its graph (SparseGCM's flat list): the CSC view is then built without a sort
        self.batches = batches
        # col: the sources in CSR order, csc: the (col_ptr, rows, perm) of csc(), when the builder of the list has
        # them already (DenseToSparse: both orders of a dense adjacency come out of one pass)
        if col is None:
            col = edge_index[0] if csr_perm is None else edge_index[0][csr_perm]
        self.col = col.contiguous()
        self._csc = csc

    @property
    def E(self):
        return self.col.numel()

    def dst_csr(self):
        d = self.edge_index[1] if self.csr_perm is None else self.edge_index[1][self.csr_perm]
        return d.contiguous()

    def csc(self):
        """(col_ptr [M+1], rows [E], perm [E]): entry k of the CSC is CSR entry perm[k]."""
        if self._csc is None:
            bt = self.batches
            if bt is not None and self.csr_perm is None and bt[2] <= 8192:
                E, dev = self.E, self.col.device
                col_ptr = torch.empty(self.M + 1, dtype=_i64, device=dev)
                rows = torch.empty(E, dtype=_i64, device=dev)
                perm = torch.empty(E, dtype=_i64, device=dev)
                _call("gcm_csc_from_csr_batched", _hip.ptr(self.row_ptr), _hip.ptr(self.col),
                      _hip.ptr(self.dst_csr()), _hip.ptr(bt[0]), _hip.ptr(col_ptr), _hip.ptr(rows),
                      _hip.ptr(perm), bt[1], self.M, E, bt[2], _hip.stream())
                self._csc = (col_ptr, rows, perm)
            else:
                src_sorted, perm = torch.sort(self.col, stable=True)
                rows = self.dst_csr()[perm].contiguous()
                self._csc = (ptr_from_sorted(src_sorted, self.M), rows, perm.contiguous())
        return self._csc

    @staticmethod
    def from_edge_index(edge_index, M):
        """Generic entry: any [2, E] (source, sink) list -> CSR by destination."""
        dst_sorted, perm = torch.sort(edge_index[1], stable=True)
        return GraphIndex(edge_index, ptr_from_sorted(dst_sorted, M), M, csr_perm=perm)


def sparse_edges_to_csr(coo, node_off, M, B, flags, n_cap=None):
    """coo [3,E] sorted (batch, sink, source) -> (edge_index [2,E] (source, sink), GraphIndex).
    n_cap: the graph size (bound on the nodes of one graph), when known."""
    coo = coo.contiguous()
    _hip.on_device(coo, node_off, flags)
    E = coo.shape[1]
    edge_index = torch.empty(2, E, dtype=_i64, device=coo.device)
    row_ptr = torch.empty(M + 1, dtype=_i64, device=coo.device)
    _call("gcm_sparse_edges_to_csr", _hip.ptr(coo), _hip.ptr(node_off), _hip.ptr(edge_index),
          _hip.ptr(row_ptr), _hip.ptr(flags), E, M, B, _hip.stream())
    return edge_index, GraphIndex(edge_index, row_ptr, M,
                                  batches=None if n_cap is None else (node_off, B, int(n_cap)))


def khop_mask(graph, node_off, T, taus, hops, B, t_pad):
    M = graph.M
    mask = torch.empty(M, dtype=torch.uint8, device=graph.row_ptr.device)
    scratch = torch.empty(2 * M, dtype=torch.uint8, device=mask.device)
    # (a list without edges - the first one-node call of a stepwise run - has no col array to walk: the subgraph is the
    #  new nodes themselves, which is what 0 rounds leave)
    _call("gcm_khop_mask", _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(node_off),
          _hip.ptr(T), _hip.ptr(taus), hops if graph.E else 0, _hip.ptr(mask), _hip.ptr(scratch), M, B, t_pad,
          _hip.stream())
    return mask


class _SparseExtract(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, T, taus, node_off, B, t_pad, flags):
        feats = feats.contiguous()
        M, H = feats.shape
        out = torch.empty(B, t_pad, H, device=feats.device, dtype=_f32)
        _call("gcm_sparse_extract_fwd", _hip.ptr(feats), _hip.ptr(T), _hip.ptr(taus),
              _hip.ptr(node_off), _hip.ptr(out), _hip.ptr(flags), B, t_pad, H, M, _hip.stream())
        ctx.save_for_backward(T, taus, node_off)
        ctx.dims = (B, t_pad, H, M)
        return out

    @staticmethod
    def backward(ctx, g_out):
        T, taus, node_off = ctx.saved_tensors
        B, t_pad, H, M = ctx.dims
        g_out = g_out.contiguous()
        g_feats = torch.empty(M, H, device=g_out.device, dtype=_f32)
        _call("gcm_sparse_extract_bwd", _hip.ptr(g_out), _hip.ptr(T), _hip.ptr(taus),
              _hip.ptr(node_off), _hip.ptr(g_feats), B, t_pad, H, M, _hip.stream())
        return g_feats, None, None, None, None, None, None


def sparse_extract(feats, T, taus, node_off, B, t_pad, flags):
    return _SparseExtract.apply(feats, T, taus, node_off, B, t_pad, flags)


# ---------------------------------------------------------------------------
# SparseGCM's sliding window: drop the oldest k_b nodes of every graph (include/gcm_hip_window.h)
# ---------------------------------------------------------------------------
class _SparseDropOldest(torch.autograd.Function):
    """(nodes [B,N,F], values [E]; idx [3,E] coalesced, T [B], k [B]) -> (nodes', idx' [3,E'], values' [E'], T',
    bptr [B+1]): gcm_sparse_drop_plan, the one readback (E'), gcm_sparse_drop_nodes, gcm_sparse_drop_edges.  New
    tensors; the inputs are not written.  Gradients reach nodes and values (a row shift and a scatter)."""

    @staticmethod
    def forward(ctx, nodes, values, idx, T, k):
        nodes, values, idx = nodes.contiguous(), values.contiguous(), idx.contiguous()
        T, k = T.contiguous(), k.contiguous()
        _hip.on_device(nodes, values, idx, T, k)
        B, N, F = nodes.shape
        E, dev = idx.shape[1], nodes.device
        st = _hip.stream()
        n_chunks = -(-E // _hip.SPARSE_DROP_CHUNK)
        chunk_off = torch.empty(n_chunks + 1, dtype=_i64, device=dev)
        T_out = torch.empty_like(T)
        _call("gcm_sparse_drop_plan", _hip.ptr(idx) if E else None, _hip.ptr(k), _hip.ptr(T), _hip.ptr(T_out),
              _hip.ptr(chunk_off), E, B, N, st)
        nodes_out = torch.empty_like(nodes)
        _call("gcm_sparse_drop_nodes", _hip.ptr(nodes), _hip.ptr(k), _hip.ptr(T), _hip.ptr(nodes_out), B, N, F, 0, st)
        E_new = int(chunk_off[n_chunks].item()) if E else 0            # the one readback
        idx_out = torch.empty(3, E_new, dtype=_i64, device=dev)
        values_out = torch.empty(E_new, dtype=_f32, device=dev)
        src_pos = torch.empty(E_new, dtype=_i64, device=dev)
        bptr = torch.empty(B + 1, dtype=_i64, device=dev)
        _call("gcm_sparse_drop_edges", _hip.ptr(idx) if E else None, _hip.ptr(values) if E_new else None, _hip.ptr(k),
              _hip.ptr(T), _hip.ptr(chunk_off), _hip.ptr(idx_out) if E_new else None,
              _hip.ptr(values_out) if E_new else None, _hip.ptr(src_pos) if E_new else None, _hip.ptr(bptr), E, E_new,
              B, N, st)
        ctx.save_for_backward(T, k, src_pos)
        ctx.dims = (B, N, F, E, E_new)
        ctx.mark_non_differentiable(idx_out, T_out, bptr)
        return nodes_out, idx_out, values_out, T_out, bptr

    @staticmethod
    def backward(ctx, g_nodes, _g_idx, g_values, _g_T, _g_bptr):
        T, k, src_pos = ctx.saved_tensors
        B, N, F, E, E_new = ctx.dims
        st = _hip.stream()
        gn = gv = None
        if ctx.needs_input_grad[0] and g_nodes is not None:
            g_nodes = g_nodes.contiguous()
            gn = torch.empty_like(g_nodes)
            _call("gcm_sparse_drop_nodes", _hip.ptr(g_nodes), _hip.ptr(k), _hip.ptr(T), _hip.ptr(gn), B, N, F, 1, st)
        if ctx.needs_input_grad[1] and g_values is not None:
            g_values = g_values.contiguous()
            gv = torch.empty(E, dtype=_f32, device=T.device)
            _call("gcm_sparse_drop_values_bwd", _hip.ptr(g_values) if E_new else None,
                  _hip.ptr(src_pos) if E_new else None, _hip.ptr(gv) if E else None, E, E_new, st)
        return gn, gv, None, None, None


def sparse_drop_oldest(nodes, idx, values, T, k):
    """-> (nodes', idx', values', T', bptr): every graph without its oldest min(max(k_b, 0), T_b) nodes."""
    nodes_out, idx_out, values_out, T_out, bptr = _SparseDropOldest.apply(nodes, values, idx, T, k)
    return nodes_out, idx_out, values_out, T_out, bptr


# ---------------------------------------------------------------------------
# Episode resets inside one SparseGCM call: the segment layout (include/gcm_hip_segments.h)
# ---------------------------------------------------------------------------
class SegmentPlan:
    """gcm_sparse_seg_plan over (mask u8 [B,t], taus [B], T [B], the stored list idx [3,E] or None) and its ONE
    readback: Bp virtual graphs, tp columns, n_resets valid resets, E_keep stored edges that stay.  vbase [B+1],
    table [SEG_ROWS, cap], relabel [B], chunk_off: what the movement kernels below take."""

    def __init__(self, mask, taus, T, idx):
        mask, taus, T = mask.contiguous(), taus.contiguous(), T.contiguous()
        idx = None if idx is None or idx.shape[1] == 0 else idx.contiguous()
        _hip.on_device(mask, taus, T, idx)
        self.B, self.t = mask.shape
        self.E = 0 if idx is None else idx.shape[1]
        B, t, dev = self.B, self.t, mask.device
        self.cap = B * (t + 1)
        self.vbase = torch.empty(B + 1, dtype=_i64, device=dev)
        self.table = torch.empty(_hip.SPARSE_SEG_ROWS, self.cap, dtype=_i64, device=dev)
        self.relabel = torch.empty(B, dtype=_i64, device=dev)
        self.chunk_off = torch.empty(-(-self.E // _hip.SPARSE_SEG_CHUNK) + 1, dtype=_i64, device=dev)
        totals = torch.empty(_hip.SPARSE_SEG_TOTALS, dtype=_i64, device=dev)
        _call("gcm_sparse_seg_plan", _hip.ptr(mask), _hip.ptr(taus), _hip.ptr(T), _hip.ptr(idx), _hip.ptr(self.vbase),
              _hip.ptr(self.table), self.cap, _hip.ptr(self.relabel), _hip.ptr(self.chunk_off), _hip.ptr(totals),
              self.E, B, t, _hip.stream())
        self.Bp, self.tp, self.n_resets, self.E_keep = (int(v) for v in totals.tolist())      # the one readback

    def row(self, which):
        """Row `which` (a SPARSE_SEG_* constant) of the table, its Bp written entries."""
        return self.table[which, :self.Bp]


class _SegRows(torch.autograd.Function):
    """Rows between the batch layout [B,t,F] and the segment layout [Bp,tp,F] (gcm_sparse_seg_rows); each direction
    is the other's adjoint."""

    @staticmethod
    def forward(ctx, src, plan, to_segments):
        src = src.contiguous()
        _hip.on_device(src)
        p, F = plan, src.shape[-1]
        want = (p.B, p.t) if to_segments else (p.Bp, p.tp)
        if tuple(src.shape[:2]) != want:
            raise ValueError(f"expected rows of shape {list(want)}, got {list(src.shape[:2])}")
        out = torch.empty((p.Bp, p.tp, F) if to_segments else (p.B, p.t, F), dtype=_f32, device=src.device)
        if out.numel():
            _call("gcm_sparse_seg_rows", _hip.ptr(src), _hip.ptr(p.table), p.cap, _hip.ptr(out), p.Bp, p.tp, p.B, p.t,
                  F, 0 if to_segments else 1, _hip.stream())
        ctx.plan, ctx.to_segments = plan, to_segments
        return out

    @staticmethod
    def backward(ctx, g):
        return _SegRows.apply(g, ctx.plan, not ctx.to_segments), None, None


def seg_rows(src, plan, to_segments):
    return _SegRows.apply(src, plan, to_segments)


class _SegNodes(torch.autograd.Function):
    """Node matrices between [B,N,F] and [Bp,N,F] (gcm_sparse_seg_nodes): final=False pairs a graph with its first
    virtual graph unless that one enters empty, final=True with its last one."""

    @staticmethod
    def forward(ctx, src, plan, final, to_segments):
        src = src.contiguous()
        _hip.on_device(src)
        p = plan
        _, N, F = src.shape
        if src.shape[0] != (p.B if to_segments else p.Bp):
            raise ValueError(f"expected {p.B if to_segments else p.Bp} node matrices, got {src.shape[0]}")
        out = torch.empty(p.Bp if to_segments else p.B, N, F, dtype=_f32, device=src.device)
        if out.numel():
            _call("gcm_sparse_seg_nodes", _hip.ptr(src), _hip.ptr(p.vbase), _hip.ptr(p.table), p.cap, _hip.ptr(out),
                  p.Bp, p.B, N, F, int(final), int(to_segments), _hip.stream())
        ctx.plan, ctx.final, ctx.to_segments = plan, final, to_segments
        return out

    @staticmethod
    def backward(ctx, g):
        return _SegNodes.apply(g, ctx.plan, ctx.final, not ctx.to_segments), None, None, None


def seg_nodes(src, plan, final, to_segments):
    return _SegNodes.apply(src, plan, final, to_segments)


class _SegEdges(torch.autograd.Function):
    """The survivors of a coalesced list under a relabelling of its batches (gcm_sparse_seg_edges), order kept:
    (values [E]; idx [3,E], relabel [B_old], chunk_off, E_new) -> (idx' [3,E_new], values' [E_new])."""

    @staticmethod
    def forward(ctx, values, idx, relabel, chunk_off, E_new, B_old, B_new):
        values, idx = values.contiguous(), idx.contiguous()
        _hip.on_device(values, idx, relabel, chunk_off)
        E, dev = idx.shape[1], idx.device
        idx_out = torch.empty(3, E_new, dtype=_i64, device=dev)
        values_out = torch.empty(E_new, dtype=_f32, device=dev)
        src_pos = torch.empty(E_new, dtype=_i64, device=dev)
        if E_new:
            _call("gcm_sparse_seg_edges", _hip.ptr(idx), _hip.ptr(values), _hip.ptr(relabel), _hip.ptr(chunk_off),
                  _hip.ptr(idx_out), _hip.ptr(values_out), _hip.ptr(src_pos), E, E_new, B_old, B_new, _hip.stream())
        ctx.save_for_backward(src_pos)
        ctx.dims = (E, E_new)
        ctx.mark_non_differentiable(idx_out)
        return idx_out, values_out

    @staticmethod
    def backward(ctx, _g_idx, g_values):
        (src_pos,) = ctx.saved_tensors
        E, E_new = ctx.dims
        if g_values is None:
            return (None,) * 7
        g_values = g_values.contiguous()
        gv = torch.empty(E, dtype=_f32, device=src_pos.device)
        _call("gcm_sparse_drop_values_bwd", _hip.ptr(g_values) if E_new else None, _hip.ptr(src_pos) if E_new else None,
              _hip.ptr(gv) if E else None, E, E_new, _hip.stream())
        return gv, None, None, None, None, None, None


def seg_expand_edges(idx, values, plan):
    """The stored list in the segment layout: batch b -> vbase[b]; the graphs whose column 0 resets lose theirs."""
    return _SegEdges.apply(values, idx, plan.relabel, plan.chunk_off, plan.E_keep, plan.B, plan.Bp)


def seg_collect_edges(idx, values, plan):
    """The entries of the call's list that belong to the last virtual graph of every b, relabelled to b; one readback
    (their count)."""
    idx = idx.contiguous()
    _hip.on_device(idx)
    E = idx.shape[1]
    n_chunks = -(-E // _hip.SPARSE_SEG_CHUNK)
    chunk_off = torch.empty(n_chunks + 1, dtype=_i64, device=idx.device)
    final = plan.row(_hip.SPARSE_SEG_FINAL)
    _call("gcm_sparse_seg_edges_plan", _hip.ptr(idx) if E else None, _hip.ptr(final), _hip.ptr(chunk_off), E, plan.Bp,
          _hip.stream())
    E_new = int(chunk_off[n_chunks].item()) if E else 0            # the one readback
    return _SegEdges.apply(values, idx, final, chunk_off, E_new, plan.Bp, plan.B)


def seg_final_T(T_seg, plan):
    T_seg = T_seg.contiguous()
    _hip.on_device(T_seg)
    out = torch.empty(plan.B, dtype=_i64, device=T_seg.device)
    _call("gcm_sparse_seg_final_T", _hip.ptr(T_seg), _hip.ptr(plan.vbase), _hip.ptr(out), plan.Bp, plan.B, _hip.stream())
    return out


def _scratch(name, *dims, device):
    """(uint8 tensor, nbytes) of the size the library's `<name>_workspace_bytes(*dims)` asks for: a backward's
    workspace or what a forward saves for its backward."""
    nbytes = getattr(_hip.lib(), name + "_workspace_bytes")(*dims)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _csc_or_none(graph, wanted):
    """graph.csc() = (col_ptr, rows, perm) when wanted, else three Nones: building the CSC view launches work."""
    return graph.csc() if wanted else (None, None, None)


def _contig(t):
    return None if t is None else t.contiguous()


def _gcn_norm(graph, w_edge, normalize, add_self_loops, fill):
    """gcm_gcn_norm over the CSR entries (w_edge [E] in CSR order or None) -> (dst [E], coef [E], dinv [M], loop_w
    [M], loop_coef [M], loop_e [M])."""
    M, E, dev = graph.M, graph.E, graph.col.device
    dst = graph.dst_csr()
    coef = torch.empty(E, device=dev, dtype=_f32)
    dinv = torch.empty(M, device=dev, dtype=_f32)
    loop_w = torch.empty(M, device=dev, dtype=_f32)
    loop_coef = torch.empty(M, device=dev, dtype=_f32)
    loop_e = torch.empty(M, device=dev, dtype=_i64)
    _call("gcm_gcn_norm", _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(dst), _hip.ptr(w_edge),
          _hip.ptr(coef), _hip.ptr(dinv), _hip.ptr(loop_w), _hip.ptr(loop_coef), _hip.ptr(loop_e), M, E,
          int(normalize), int(add_self_loops), float(fill), _hip.stream())
    return dst, coef, dinv, loop_w, loop_coef, loop_e


class _CsrGraphConv(torch.autograd.Function):
    """x [M,Fi]; w_edge [E] in CSR order or None."""

    @staticmethod
    def forward(ctx, x, w_edge, w_rel, b_rel, w_root, graph, act):
        x = x.contiguous()
        w_rel, w_root = w_rel.contiguous(), w_root.contiguous()
        b_rel = _contig(b_rel)
        w_edge = _contig(w_edge)
        _hip.on_device(x, w_edge, w_rel, b_rel, w_root)
        M, Fi = x.shape
        Fo = w_rel.shape[0]
        assert M == graph.M
        out = torch.empty(M, Fo, device=x.device, dtype=_f32)
        need_bwd = any(ctx.needs_input_grad)
        agg = torch.empty(M, Fi, device=x.device, dtype=_f32) if need_bwd else None
        _call("gcm_csr_graphconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
              _hip.ptr(w_edge), _hip.ptr(graph.mask), _hip.ptr(w_rel), _hip.ptr(b_rel),
              _hip.ptr(w_root), _hip.ptr(out), _hip.ptr(agg), M, Fi, Fo, act, _hip.stream())
        ctx.save_for_backward(x, w_edge, w_rel, w_root, out, agg)
        ctx.graph, ctx.act, ctx.has_bias = graph, act, b_rel is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w_edge, w_rel, w_root, out, agg = ctx.saved_tensors
        graph = ctx.graph
        M, Fi = x.shape
        Fo = w_rel.shape[0]
        need_x, need_we, need_wrel, need_b, need_wroot, _, _ = ctx.needs_input_grad
        need_b = need_b and ctx.has_bias
        need_we = need_we and w_edge is not None
        g_out = _hip.kernel_ready(g_out)
        dev = x.device
        lib = _hip.lib()
        E = graph.E
        col_ptr, rows, perm = _csc_or_none(graph, (need_x or need_we) and E > 0)
        g_x = torch.empty_like(x) if need_x else None
        g_we = torch.zeros_like(w_edge) if need_we else None
        g_wrel = torch.empty_like(w_rel) if need_wrel else None
        g_wroot = torch.empty_like(w_root) if need_wroot else None
        g_b = torch.empty(Fo, device=dev, dtype=_f32) if need_b else None
        ws, ws_bytes = _scratch("gcm_csr_graphconv_bwd", M, Fi, Fo, device=dev)
        _call("gcm_csr_graphconv_bwd", _hip.ptr(g_out), _hip.ptr(out), _hip.ptr(x), _hip.ptr(agg),
              _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(col_ptr), _hip.ptr(rows),
              _hip.ptr(perm), _hip.ptr(w_edge), _hip.ptr(graph.mask), _hip.ptr(w_rel),
              _hip.ptr(w_root), _hip.ptr(g_x), _hip.ptr(g_we), _hip.ptr(g_wrel), _hip.ptr(g_b),
              _hip.ptr(g_wroot), _hip.ptr(ws), ws_bytes, M, E, Fi, Fo, ctx.act, _hip.stream())
        return g_x, g_we, g_wrel, g_b, g_wroot, None, None


def csr_graphconv(x, w_edge, w_rel, b_rel, w_root, graph, act=_hip.ACT_NONE):
    return _CsrGraphConv.apply(x, w_edge, w_rel, b_rel, w_root, graph, act)


# ---------------------------------------------------------------------------
# DenseGCNConv / GCNConv (PyG; csrc/gcnconv.hip)
# ---------------------------------------------------------------------------
class _DenseGCNConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj, w, bias, add_loop, loop_value):
        x, adj, w = x.contiguous(), adj.contiguous(), w.contiguous()
        bias = _contig(bias)
        _hip.on_device(x, adj, w, bias)
        B, N, Fi = x.shape
        Fo = w.shape[0]
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert w.shape == (Fo, Fi)
        dev = x.device
        out = torch.empty(B, N, Fo, device=dev, dtype=_f32)
        y = torch.empty(B, N, Fo, device=dev, dtype=_f32)
        deg = torch.empty(B, N, device=dev, dtype=_f32)
        dinv = torch.empty(B, N, device=dev, dtype=_f32)
        agg = torch.empty(B, N, Fo, device=dev, dtype=_f32) if any(ctx.needs_input_grad) else None
        _call("gcm_dense_gcnconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(out),
              _hip.ptr(y), _hip.ptr(agg), _hip.ptr(deg), _hip.ptr(dinv), B, N, Fi, Fo, int(add_loop),
              float(loop_value), _hip.stream())
        ctx.save_for_backward(x, adj, w, y, agg, deg, dinv)
        ctx.loop = (int(add_loop), float(loop_value))
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, adj, w, y, agg, deg, dinv = ctx.saved_tensors
        B, N, Fi = x.shape
        Fo = w.shape[0]
        need_x, need_adj, need_w, need_b, _, _ = ctx.needs_input_grad
        need_b = need_b and ctx.has_bias
        g_out = _hip.kernel_ready(g_out)
        dev = x.device
        lib = _hip.lib()
        g_x = torch.empty_like(x) if need_x else None
        g_adj = torch.empty_like(adj) if need_adj else None
        g_w = torch.empty_like(w) if need_w else None
        g_b = torch.empty(Fo, device=dev, dtype=_f32) if need_b else None
        ws, ws_bytes = _scratch("gcm_dense_gcnconv_bwd", B, N, Fi, Fo, device=dev)
        _call("gcm_dense_gcnconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w), _hip.ptr(y),
              _hip.ptr(agg), _hip.ptr(deg), _hip.ptr(dinv), _hip.ptr(g_x), _hip.ptr(g_adj), _hip.ptr(g_w),
              _hip.ptr(g_b), _hip.ptr(ws), ws_bytes, B, N, Fi, Fo, ctx.loop[0], ctx.loop[1], _hip.stream())
        return g_x, g_adj, g_w, g_b, None, None


def dense_gcnconv(x, adj, w, bias, add_loop, loop_value):
    return _DenseGCNConv.apply(x, adj, w, bias, add_loop, loop_value)


class _CsrGCNConv(torch.autograd.Function):
    """x [M,Fi]; w_edge [E] in CSR order or None (unit weights)."""

    @staticmethod
    def forward(ctx, x, w_edge, w, bias, graph, normalize, add_self_loops, fill):
        x, w = x.contiguous(), w.contiguous()
        bias = _contig(bias)
        w_edge = _contig(w_edge)
        _hip.on_device(x, w_edge, w, bias)
        M, Fi = x.shape
        Fo = w.shape[0]
        E = graph.E
        assert M == graph.M
        dev = x.device
        dst, coef, dinv, loop_w, loop_coef, loop_e = _gcn_norm(graph, w_edge, normalize, add_self_loops, fill)
        out = torch.empty(M, Fo, device=dev, dtype=_f32)
        agg = torch.empty(M, Fi, device=dev, dtype=_f32) if any(ctx.needs_input_grad) else None
        _call("gcm_csr_gcnconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(coef),
              _hip.ptr(loop_coef), _hip.ptr(w), _hip.ptr(bias), _hip.ptr(out), _hip.ptr(agg), M, E, Fi, Fo,
              _hip.stream())
        ctx.save_for_backward(x, w_edge, w, agg, dst, coef, dinv, loop_w, loop_coef, loop_e)
        ctx.graph, ctx.has_bias = graph, bias is not None
        ctx.norm = (int(normalize), int(add_self_loops))
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w_edge, w, agg, dst, coef, dinv, loop_w, loop_coef, loop_e = ctx.saved_tensors
        graph = ctx.graph
        M, Fi = x.shape
        Fo = w.shape[0]
        E = graph.E
        need_x, need_we, need_w, need_b, _, _, _, _ = ctx.needs_input_grad
        need_b = need_b and ctx.has_bias
        need_we = need_we and w_edge is not None
        g_out = _hip.kernel_ready(g_out)
        dev = x.device
        lib = _hip.lib()
        col_ptr, rows, perm = _csc_or_none(graph, (need_x or need_we) and E > 0)
        g_x = torch.empty_like(x) if need_x else None
        g_we = torch.zeros_like(w_edge) if need_we else None
        g_w = torch.empty_like(w) if need_w else None
        g_b = torch.empty(Fo, device=dev, dtype=_f32) if need_b else None
        ws, ws_bytes = _scratch("gcm_csr_gcnconv_bwd", M, E, Fi, Fo, device=dev)
        _call("gcm_csr_gcnconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(agg), _hip.ptr(graph.row_ptr),
              _hip.ptr(graph.col), _hip.ptr(dst), _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(perm),
              _hip.ptr(w_edge), _hip.ptr(coef), _hip.ptr(dinv), _hip.ptr(loop_w), _hip.ptr(loop_coef),
              _hip.ptr(loop_e), _hip.ptr(w), _hip.ptr(g_x), _hip.ptr(g_we), _hip.ptr(g_w), _hip.ptr(g_b),
              _hip.ptr(ws), ws_bytes, M, E, Fi, Fo, ctx.norm[0], ctx.norm[1], _hip.stream())
        return g_x, g_we, g_w, g_b, None, None, None, None


def csr_gcnconv(x, w_edge, w, bias, graph, normalize, add_self_loops, fill):
    return _CsrGCNConv.apply(x, w_edge, w, bias, graph, normalize, add_self_loops, fill)


# ---------------------------------------------------------------------------
# DenseGINConv / GINConv (PyG; csrc/ginconv.hip): the aggregation alone, the layer's `nn` stays in torch
# ---------------------------------------------------------------------------
class _DenseGINAggregate(torch.autograd.Function):
    """h = s x + adj @ x, s = 1 + eps if add_loop else 0; x [B,N,F], adj [B,N,N], eps [1] (read on the device)."""

    @staticmethod
    def forward(ctx, x, adj, eps, add_loop):
        x, adj, eps = x.contiguous(), adj.contiguous(), eps.contiguous()
        _hip.on_device(x, adj, eps)
        B, N, F = x.shape
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert eps.numel() == 1 and eps.dtype == _f32
        h = torch.empty(B, N, F, device=x.device, dtype=_f32)
        _call("gcm_dense_gin_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(eps), _hip.ptr(h), B, N, F, int(add_loop),
              _hip.stream())
        ctx.save_for_backward(x, adj, eps)
        ctx.add_loop = int(add_loop)
        return h

    @staticmethod
    def backward(ctx, g_h):
        x, adj, eps = ctx.saved_tensors
        B, N, F = x.shape
        need_x, need_adj, need_eps, _ = ctx.needs_input_grad
        g_h = _hip.kernel_ready(g_h)
        dev = x.device
        g_x = torch.empty_like(x) if need_x else None
        g_adj = torch.empty_like(adj) if need_adj else None
        g_eps = torch.empty_like(eps) if need_eps else None
        ws, ws_bytes = _scratch("gcm_dense_gin_bwd", B, N, F, device=dev)
        _call("gcm_dense_gin_bwd", _hip.ptr(g_h), _hip.ptr(x), _hip.ptr(adj), _hip.ptr(eps), _hip.ptr(g_x),
              _hip.ptr(g_adj), _hip.ptr(g_eps), _hip.ptr(ws), ws_bytes, B, N, F, ctx.add_loop, _hip.stream())
        return g_x, g_adj, g_eps, None


def dense_gin_aggregate(x, adj, eps, add_loop):
    return _DenseGINAggregate.apply(x, adj, eps, add_loop)


class _CsrGINAggregate(torch.autograd.Function):
    """h_i = (1 + eps) x_i + sum over the in-edges of i of x_source; x [M,F], eps [1] (read on the device)."""

    @staticmethod
    def forward(ctx, x, eps, graph):
        x, eps = x.contiguous(), eps.contiguous()
        _hip.on_device(x, eps)
        M, F = x.shape
        assert M == graph.M
        assert eps.numel() == 1 and eps.dtype == _f32
        h = torch.empty(M, F, device=x.device, dtype=_f32)
        _call("gcm_csr_gin_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(eps),
              _hip.ptr(h), M, graph.E, F, _hip.stream())
        ctx.save_for_backward(x, eps)
        ctx.graph = graph
        return h

    @staticmethod
    def backward(ctx, g_h):
        x, eps = ctx.saved_tensors
        graph = ctx.graph
        M, F = x.shape
        E = graph.E
        need_x, need_eps, _ = ctx.needs_input_grad
        g_h = _hip.kernel_ready(g_h)
        dev = x.device
        col_ptr, rows, _ = _csc_or_none(graph, need_x and E > 0)
        g_x = torch.empty_like(x) if need_x else None
        g_eps = torch.empty_like(eps) if need_eps else None
        ws, ws_bytes = _scratch("gcm_csr_gin_bwd", M, E, F, device=dev)
        _call("gcm_csr_gin_bwd", _hip.ptr(g_h), _hip.ptr(x), _hip.ptr(eps), _hip.ptr(col_ptr), _hip.ptr(rows),
              _hip.ptr(g_x), _hip.ptr(g_eps), _hip.ptr(ws), ws_bytes, M, E, F, _hip.stream())
        return g_x, g_eps, None


def csr_gin_aggregate(x, eps, graph):
    return _CsrGINAggregate.apply(x, eps, graph)


# ---------------------------------------------------------------------------
# DenseGINEConv / GINEConv and RelativeEdgeAttr (csrc/gineconv.hip): the aggregation alone, `nn` stays in torch.  The
# projected edge features and the messages are never materialised: what is saved is the inputs.
# ---------------------------------------------------------------------------
def _gine_lin(w_e, b_e, F, D):
    if w_e is None:
        assert b_e is None and D == F
        return None, None
    w_e, b_e = w_e.contiguous(), b_e.contiguous()
    assert w_e.shape == (F, D) and b_e.shape == (F,)
    return w_e, b_e


class _CsrGINEAggregate(torch.autograd.Function):
    """h_i = (1 + eps) x_i + sum over the in-edges k of i of relu(x_source + e_k), e_k = w_e a_k + b_e (a_k itself
    when w_e is None); x [M,F], edge_attr [E,D] in the order of graph.edge_index, eps [1] (read on the device)."""

    @staticmethod
    def forward(ctx, x, edge_attr, w_e, b_e, eps, graph):
        x, edge_attr, eps = x.contiguous(), edge_attr.contiguous(), eps.contiguous()
        M, F = x.shape
        E, D = edge_attr.shape
        w_e, b_e = _gine_lin(w_e, b_e, F, D)
        _hip.on_device(x, edge_attr, w_e, b_e, eps)
        assert M == graph.M and E == graph.E
        assert eps.numel() == 1 and eps.dtype == _f32
        h = torch.empty(M, F, device=x.device, dtype=_f32)
        _call("gcm_csr_gine_fwd", _hip.ptr(x), _hip.ptr(edge_attr), _hip.ptr(w_e), _hip.ptr(b_e), _hip.ptr(eps),
              _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(graph.csr_perm), _hip.ptr(h), M, E, F, D,
              _hip.stream())
        ctx.save_for_backward(x, edge_attr, w_e, b_e, eps)
        ctx.graph = graph
        return h

    @staticmethod
    def backward(ctx, g_h):
        x, edge_attr, w_e, b_e, eps = ctx.saved_tensors
        graph = ctx.graph
        M, F = x.shape
        E, D = edge_attr.shape
        need_x, need_ea, need_w, need_b, need_eps, _ = ctx.needs_input_grad
        g_h = _hip.kernel_ready(g_h)
        dev = x.device
        col_ptr = rows = csc_perm = None
        if need_x and E > 0:
            by_source = Segments.by_source(graph)
            col_ptr, rows, csc_perm = by_source.ptr, graph.csc()[1], by_source.perm
        g_x = torch.empty_like(x) if need_x else None
        g_ea = torch.empty_like(edge_attr) if need_ea else None
        g_w = torch.empty_like(w_e) if need_w else None
        g_b = torch.empty_like(b_e) if need_b else None
        g_eps = torch.empty_like(eps) if need_eps else None
        ws, ws_bytes = _scratch("gcm_csr_gine_bwd", M, E, F, D, device=dev)
        _call("gcm_csr_gine_bwd", _hip.ptr(g_h), _hip.ptr(x), _hip.ptr(edge_attr), _hip.ptr(w_e), _hip.ptr(b_e),
              _hip.ptr(eps), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(graph.csr_perm),
              _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(csc_perm), _hip.ptr(g_x), _hip.ptr(g_ea), _hip.ptr(g_w),
              _hip.ptr(g_b), _hip.ptr(g_eps), _hip.ptr(ws), ws_bytes, M, E, F, D, _hip.stream())
        return g_x, g_ea, g_w, g_b, g_eps, None


def csr_gine_aggregate(x, edge_attr, w_e, b_e, eps, graph):
    return _CsrGINEAggregate.apply(x, edge_attr, w_e, b_e, eps, graph)


class _DenseGINEAggregate(torch.autograd.Function):
    """h = s x + sum_j adj_ij relu(x_j + e_ij) over the set entries of adj, s = 1 + eps if add_loop else 0; x [B,N,F],
    adj [B,N,N], edge_attr [B,N,N,D].  With a gradient wanted for adj, the backward reads every entry of edge_attr."""

    @staticmethod
    def forward(ctx, x, adj, edge_attr, w_e, b_e, eps, add_loop):
        x, adj, edge_attr, eps = x.contiguous(), adj.contiguous(), edge_attr.contiguous(), eps.contiguous()
        B, N, F = x.shape
        D = edge_attr.shape[-1]
        w_e, b_e = _gine_lin(w_e, b_e, F, D)
        _hip.on_device(x, adj, edge_attr, w_e, b_e, eps)
        assert adj.shape == (B, N, N) and edge_attr.shape == (B, N, N, D)
        assert eps.numel() == 1 and eps.dtype == _f32
        h = torch.empty(B, N, F, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_dense_gine_fwd", B, N, F, D, device=x.device)
        _call("gcm_dense_gine_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(edge_attr), _hip.ptr(w_e), _hip.ptr(b_e),
              _hip.ptr(eps), _hip.ptr(h), _hip.ptr(saved), saved_bytes, B, N, F, D, int(add_loop), _hip.stream())
        ctx.save_for_backward(x, adj, edge_attr, w_e, b_e, eps, saved)
        ctx.add_loop = int(add_loop)
        return h

    @staticmethod
    def backward(ctx, g_h):
        x, adj, edge_attr, w_e, b_e, eps, saved = ctx.saved_tensors
        B, N, F = x.shape
        D = edge_attr.shape[-1]
        need_x, need_adj, need_ea, need_w, need_b, need_eps, _ = ctx.needs_input_grad
        g_h = _hip.kernel_ready(g_h)
        g_x = torch.empty_like(x) if need_x else None
        g_adj = torch.empty_like(adj) if need_adj else None
        g_ea = torch.empty_like(edge_attr) if need_ea else None
        g_w = torch.empty_like(w_e) if need_w else None
        g_b = torch.empty_like(b_e) if need_b else None
        g_eps = torch.empty_like(eps) if need_eps else None
        ws, ws_bytes = _scratch("gcm_dense_gine_bwd", B, N, F, D, device=x.device)
        _call("gcm_dense_gine_bwd", _hip.ptr(g_h), _hip.ptr(x), _hip.ptr(adj), _hip.ptr(edge_attr), _hip.ptr(w_e),
              _hip.ptr(b_e), _hip.ptr(eps), _hip.ptr(saved), _hip.ptr(g_x), _hip.ptr(g_adj), _hip.ptr(g_ea),
              _hip.ptr(g_w), _hip.ptr(g_b), _hip.ptr(g_eps), _hip.ptr(ws), ws_bytes, B, N, F, D, ctx.add_loop,
              _hip.stream())
        return g_x, g_adj, g_ea, g_w, g_b, g_eps, None


def dense_gine_aggregate(x, adj, edge_attr, w_e, b_e, eps, add_loop):
    return _DenseGINEAggregate.apply(x, adj, edge_attr, w_e, b_e, eps, add_loop)


class _RelEdgeAttr(torch.autograd.Function):
    """out [E,D] in edge_index order: [(sink - source) * time_scale, x[source, p0:p0+P] - x[sink, p0:p0+P]]; the
    gradient to x is gathered over the CSC column and the CSR row of every node (`graph`: the list's GraphIndex)."""

    @staticmethod
    def forward(ctx, x, edge_index, graph, p0, P, time, time_scale):
        x, edge_index = x.contiguous(), edge_index.contiguous()
        _hip.on_device(x, edge_index)
        M, F = x.shape
        E = edge_index.shape[1]
        out = torch.empty(E, time + P, device=x.device, dtype=_f32)
        _call("gcm_rel_edge_attr_fwd", _hip.ptr(x), _hip.ptr(edge_index), _hip.ptr(out), M, E, F, p0, P, time,
              float(time_scale), _hip.stream())
        ctx.graph, ctx.cfg = graph, (M, E, F, p0, P, time)
        return out

    @staticmethod
    def backward(ctx, g_out):
        M, E, F, p0, P, time = ctx.cfg
        graph = ctx.graph
        g_out = _hip.kernel_ready(g_out)
        g_x = torch.empty(M, F, device=g_out.device, dtype=_f32)
        col_ptr = csc_perm = None
        if E > 0:
            by_source = Segments.by_source(graph)
            col_ptr, csc_perm = by_source.ptr, by_source.perm
        _call("gcm_rel_edge_attr_bwd", _hip.ptr(g_out), _hip.ptr(graph.row_ptr), _hip.ptr(graph.csr_perm),
              _hip.ptr(col_ptr), _hip.ptr(csc_perm), _hip.ptr(g_x), M, E, F, p0, P, time, _hip.stream())
        return g_x, None, None, None, None, None, None


def rel_edge_attr(x, edge_index, graph, p0, P, time, time_scale):
    """graph: a callable that returns the list's GraphIndex, called only when x needs a gradient through the pose."""
    if P == 0 or not (x.requires_grad and torch.is_grad_enabled()):
        return _RelEdgeAttr.apply(x.detach(), edge_index, None, p0, P, time, time_scale)
    return _RelEdgeAttr.apply(x, edge_index, graph(), p0, P, time, time_scale)


class _DenseRelEdgeAttr(torch.autograd.Function):
    """out [B,N,N,D]: entry (b,i,j) = [(i - j) * time_scale, x[b,j,p0:p0+P] - x[b,i,p0:p0+P]]."""

    @staticmethod
    def forward(ctx, x, p0, P, time, time_scale):
        x = x.contiguous()
        _hip.on_device(x)
        B, N, F = x.shape
        out = torch.empty(B, N, N, time + P, device=x.device, dtype=_f32)
        _call("gcm_dense_rel_edge_attr_fwd", _hip.ptr(x), _hip.ptr(out), B, N, F, p0, P, time, float(time_scale),
              _hip.stream())
        ctx.cfg = (B, N, F, p0, P, time)
        return out

    @staticmethod
    def backward(ctx, g_out):
        B, N, F, p0, P, time = ctx.cfg
        g_out = _hip.kernel_ready(g_out)
        g_x = torch.empty(B, N, F, device=g_out.device, dtype=_f32)
        _call("gcm_dense_rel_edge_attr_bwd", _hip.ptr(g_out), _hip.ptr(g_x), B, N, F, p0, P, time, _hip.stream())
        return g_x, None, None, None, None


def dense_rel_edge_attr(x, p0, P, time, time_scale):
    return _DenseRelEdgeAttr.apply(x.detach() if P == 0 else x, p0, P, time, time_scale)


# ---------------------------------------------------------------------------
# GATv2Conv / DenseGATv2Conv (gcm.gatv2; csrc/gatv2conv.hip).  Nothing per edge is saved: x_l, x_r and the softmax's
# per-row maximum and sum are, and the backward recomputes the scores from them.
# ---------------------------------------------------------------------------
class GATv2Config:
    """What the kernels take beside tensors: heads, out_channels, concat, loops (add_self_loops / add_loop),
    fill_value ("mean" or a number) and negative_slope."""

    def __init__(self, heads, out_channels, concat, loops, fill_value, slope):
        self.H, self.C, self.concat, self.loops = int(heads), int(out_channels), int(bool(concat)), int(bool(loops))
        self.fill_mean = int(fill_value == "mean")
        self.fill = 0.0 if self.fill_mean else float(fill_value)
        self.slope = float(slope)

    def tail(self):
        return (self.concat, self.loops, self.fill_mean, self.fill, self.slope, _hip.stream())


def _gatv2_operands(cfg, x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr):
    """Contiguous operands, checked against each other -> (operands, Fi, D)."""
    ops = [_contig(t) for t in (x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr)]
    x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr = ops
    _hip.on_device(*ops)
    Fi, HC = x.shape[-1], cfg.H * cfg.C
    assert w_l.shape == (HC, Fi) and att.numel() == HC
    assert w_r is None or w_r.shape == (HC, Fi)
    assert w_r is not None or b_r is None
    D = 0 if w_e is None else w_e.shape[1]
    assert w_e is None or (w_e.shape == (HC, D) and edge_attr is not None and edge_attr.shape[-1] == D)
    return ops, Fi, D


def _gatv2_grads(ctx, cfg, x, w_l, w_r, w_e, edge_attr):
    """The outputs the backward call is to fill (None: skip), in the order of the forward's inputs."""
    need = ctx.needs_input_grad
    HC, dev = cfg.H * cfg.C, x.device
    new = lambda wanted, like=None, n=None: (None if not wanted else torch.empty_like(like) if like is not None
                                             else torch.empty(n, device=dev, dtype=_f32))
    return [new(need[0], x), new(need[1], w_l), new(need[2], n=HC), new(need[3], w_r), new(need[4], n=HC),
            new(need[5], n=HC), new(need[6], w_e), new(need[7], n=HC if cfg.concat else cfg.C),
            new(need[8], edge_attr)]


class _CsrGATv2Conv(torch.autograd.Function):
    """x [M,Fi], edge_attr [E,D] in the order of graph.edge_index (None without edge features), w_r None: shared."""

    @staticmethod
    def forward(ctx, x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr, graph, cfg):
        ops, Fi, D = _gatv2_operands(cfg, x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr)
        x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr = ops
        M, E, H, C = x.shape[0], graph.E, cfg.H, cfg.C
        assert M == graph.M and (edge_attr is None or edge_attr.shape[0] == E)
        dev = x.device
        out = torch.empty(M, H * C if cfg.concat else C, device=dev, dtype=_f32)
        xl = torch.empty(M, H * C, device=dev, dtype=_f32)
        xr = torch.empty(M, H * C, device=dev, dtype=_f32) if w_r is not None else None
        stats = torch.empty(2, M, H, device=dev, dtype=_f32)          # row max, row sum
        ws, ws_bytes = _scratch("gcm_csr_gatv2_fwd", M, H, C, cfg.concat, device=dev)
        _call("gcm_csr_gatv2_fwd", _hip.ptr(x), _hip.ptr(w_l), _hip.ptr(b_l), _hip.ptr(w_r), _hip.ptr(b_r),
              _hip.ptr(att), _hip.ptr(w_e), _hip.ptr(bias), _hip.ptr(edge_attr), _hip.ptr(graph.row_ptr),
              _hip.ptr(graph.col), _hip.ptr(graph.csr_perm), _hip.ptr(out), _hip.ptr(xl), _hip.ptr(xr),
              _hip.ptr(stats[0]), _hip.ptr(stats[1]), _hip.ptr(ws), ws_bytes, M, E, Fi, H, C, D, *cfg.tail())
        ctx.save_for_backward(x, w_l, w_r, att, w_e, edge_attr, xl, xr, stats)
        ctx.graph, ctx.cfg = graph, cfg
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w_l, w_r, att, w_e, edge_attr, xl, xr, stats = ctx.saved_tensors
        graph, cfg = ctx.graph, ctx.cfg
        M, Fi = x.shape
        E, D = graph.E, 0 if w_e is None else w_e.shape[1]
        g_out = _hip.kernel_ready(g_out)
        need = ctx.needs_input_grad
        col_ptr = rows = csc_perm = None
        if E > 0 and (need[0] or need[1] or need[2]):
            by_source = Segments.by_source(graph)
            col_ptr, rows, csc_perm = by_source.ptr, graph.csc()[1], by_source.perm
        g = _gatv2_grads(ctx, cfg, x, w_l, w_r, w_e, edge_attr)
        g_x, g_wl, g_bl, g_wr, g_br, g_att, g_we, g_bias, g_ea = g
        ws, ws_bytes = _scratch("gcm_csr_gatv2_bwd", M, E, Fi, cfg.H, cfg.C, D, cfg.concat, device=x.device)
        _call("gcm_csr_gatv2_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(w_l), _hip.ptr(w_r), _hip.ptr(att),
              _hip.ptr(w_e), _hip.ptr(edge_attr), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
              _hip.ptr(graph.csr_perm), _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(csc_perm), _hip.ptr(xl),
              _hip.ptr(xr), _hip.ptr(stats[0]), _hip.ptr(stats[1]), _hip.ptr(g_x), _hip.ptr(g_wl), _hip.ptr(g_bl),
              _hip.ptr(g_wr), _hip.ptr(g_br), _hip.ptr(g_att), _hip.ptr(g_we), _hip.ptr(g_ea), _hip.ptr(g_bias),
              _hip.ptr(ws), ws_bytes, M, E, Fi, cfg.H, cfg.C, D, *cfg.tail())
        return g_x, g_wl, g_bl, g_wr, g_br, g_att, g_we, g_bias, g_ea, None, None


def csr_gatv2conv(x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr, graph, cfg):
    """-> out [M, H*C or C]; att is viewed flat [H*C]; w_r None: lin_r is lin_l."""
    return _CsrGATv2Conv.apply(x, w_l, b_l, w_r, b_r, att.view(-1), w_e, bias, edge_attr, graph, cfg)


class _DenseGATv2Conv(torch.autograd.Function):
    """x [B,N,Fi], adj [B,N,N] (only its nonzero pattern is read: no gradient), edge_attr [B,N,N,D] or None."""

    @staticmethod
    def forward(ctx, x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr, adj, cfg):
        ops, Fi, D = _gatv2_operands(cfg, x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr)
        x, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr = ops
        adj = adj.contiguous()
        _hip.on_device(adj)
        B, N, H, C = x.shape[0], x.shape[1], cfg.H, cfg.C
        assert adj.shape == (B, N, N) and (edge_attr is None or edge_attr.shape == (B, N, N, D))
        dev = x.device
        out = torch.empty(B, N, H * C if cfg.concat else C, device=dev, dtype=_f32)
        xl = torch.empty(B, N, H * C, device=dev, dtype=_f32)
        xr = torch.empty(B, N, H * C, device=dev, dtype=_f32) if w_r is not None else None
        stats = torch.empty(2, B, N, H, device=dev, dtype=_f32)
        bits = torch.empty(B, N, (N + 31) // 32, device=dev, dtype=torch.int32)
        ws, ws_bytes = _scratch("gcm_dense_gatv2_fwd", B, N, H, C, cfg.concat, device=dev)
        _call("gcm_dense_gatv2_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w_l), _hip.ptr(b_l), _hip.ptr(w_r),
              _hip.ptr(b_r), _hip.ptr(att), _hip.ptr(w_e), _hip.ptr(bias), _hip.ptr(edge_attr), _hip.ptr(out),
              _hip.ptr(xl), _hip.ptr(xr), _hip.ptr(stats[0]), _hip.ptr(stats[1]), _hip.ptr(bits), _hip.ptr(ws),
              ws_bytes, B, N, Fi, H, C, D, *cfg.tail())
        ctx.save_for_backward(x, w_l, w_r, att, w_e, edge_attr, xl, xr, stats, bits)
        ctx.cfg = cfg
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w_l, w_r, att, w_e, edge_attr, xl, xr, stats, bits = ctx.saved_tensors
        cfg = ctx.cfg
        B, N, Fi = x.shape
        D = 0 if w_e is None else w_e.shape[1]
        g_out = _hip.kernel_ready(g_out)
        g = _gatv2_grads(ctx, cfg, x, w_l, w_r, w_e, edge_attr)
        g_x, g_wl, g_bl, g_wr, g_br, g_att, g_we, g_bias, g_ea = g
        ws, ws_bytes = _scratch("gcm_dense_gatv2_bwd", B, N, Fi, cfg.H, cfg.C, D, cfg.concat, device=x.device)
        _call("gcm_dense_gatv2_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(w_l), _hip.ptr(w_r), _hip.ptr(att),
              _hip.ptr(w_e), _hip.ptr(edge_attr), _hip.ptr(bits), _hip.ptr(xl), _hip.ptr(xr), _hip.ptr(stats[0]),
              _hip.ptr(stats[1]), _hip.ptr(g_x), _hip.ptr(g_wl), _hip.ptr(g_bl), _hip.ptr(g_wr), _hip.ptr(g_br),
              _hip.ptr(g_att), _hip.ptr(g_we), _hip.ptr(g_ea), _hip.ptr(g_bias), _hip.ptr(ws), ws_bytes, B, N, Fi,
              cfg.H, cfg.C, D, *cfg.tail())
        return g_x, g_wl, g_bl, g_wr, g_br, g_att, g_we, g_bias, g_ea, None, None


def dense_gatv2conv(x, adj, w_l, b_l, w_r, b_r, att, w_e, bias, edge_attr, cfg):
    return _DenseGATv2Conv.apply(x, w_l, b_l, w_r, b_r, att.view(-1), w_e, bias, edge_attr, adj.detach(), cfg)


# ---------------------------------------------------------------------------
# DenseGATConv / GATConv (PyG, GAT v1; csrc/gatconv.hip)
# ---------------------------------------------------------------------------
class _DenseGATConv(torch.autograd.Function):
    """x [B,N,Fi], adj [B,N,N] (only its nonzero pattern is read: no gradient), w [H*C,Fi], att_* [H*C]."""

    @staticmethod
    def forward(ctx, x, adj, w, att_src, att_dst, bias, heads, concat, add_loop, slope):
        x, adj, w = x.contiguous(), adj.contiguous(), w.contiguous()
        att_src, att_dst = att_src.contiguous().view(-1), att_dst.contiguous().view(-1)
        bias = _contig(bias)
        _hip.on_device(x, adj, w, att_src, att_dst, bias)
        B, N, Fi = x.shape
        HC = w.shape[0]
        H, C = heads, HC // heads
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert w.shape == (H * C, Fi) and att_src.numel() == HC and att_dst.numel() == HC
        dev = x.device
        out = torch.empty(B, N, HC if concat else C, device=dev, dtype=_f32)
        y = torch.empty(B, N, HC, device=dev, dtype=_f32)
        o = torch.empty(B, N, HC, device=dev, dtype=_f32)
        stats = torch.empty(4, B, N, H, device=dev, dtype=_f32)       # s_src, s_dst, row max, row sum
        bits = torch.empty(B, N, (N + 31) // 32, device=dev, dtype=torch.int32)
        _call("gcm_dense_gatconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w), _hip.ptr(att_src),
              _hip.ptr(att_dst), _hip.ptr(bias), _hip.ptr(out), _hip.ptr(y), _hip.ptr(o), _hip.ptr(stats[0]),
              _hip.ptr(stats[1]), _hip.ptr(stats[2]), _hip.ptr(stats[3]), _hip.ptr(bits), B, N, Fi, H, C,
              int(concat), int(add_loop), float(slope), _hip.stream())
        ctx.save_for_backward(x, w, att_src, att_dst, y, stats, bits)
        ctx.cfg = (H, C, int(concat), float(slope), bias is not None)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w, att_src, att_dst, y, stats, bits = ctx.saved_tensors
        H, C, concat, slope, has_bias = ctx.cfg
        B, N, Fi = x.shape
        need_x, _, need_w, need_as, need_ad, need_b = ctx.needs_input_grad[:6]
        g_out = _hip.kernel_ready(g_out)
        lib = _hip.lib()
        g_x = torch.empty_like(x) if need_x else None
        g_w = torch.empty_like(w) if need_w else None
        g_as = torch.empty(H * C, device=x.device, dtype=_f32) if need_as else None
        g_ad = torch.empty(H * C, device=x.device, dtype=_f32) if need_ad else None
        g_b = torch.empty(H * C if concat else C, device=x.device, dtype=_f32) if need_b and has_bias else None
        ws, ws_bytes = _scratch("gcm_dense_gatconv_bwd", B, N, Fi, H, C, concat, device=x.device)
        _call("gcm_dense_gatconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(w), _hip.ptr(att_src),
              _hip.ptr(att_dst), _hip.ptr(y), _hip.ptr(stats[0]), _hip.ptr(stats[1]), _hip.ptr(stats[2]),
              _hip.ptr(stats[3]), _hip.ptr(bits), _hip.ptr(g_x), _hip.ptr(g_w),
              _hip.ptr(g_as), _hip.ptr(g_ad), _hip.ptr(g_b), _hip.ptr(ws), ws_bytes, B, N, Fi, H, C, concat,
              slope, _hip.stream())
        return g_x, None, g_w, g_as, g_ad, g_b, None, None, None, None


def dense_gatconv(x, adj, w, att_src, att_dst, bias, heads, concat, add_loop, slope):
    """-> out; att_src / att_dst are viewed flat [H*C] (their gradients come back in the same shape)."""
    return _DenseGATConv.apply(x, adj, w, att_src.view(-1), att_dst.view(-1), bias, heads, concat, add_loop,
                               slope)


class _CsrGATConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, att_src, att_dst, bias, graph, heads, concat, add_self_loops, slope):
        x, w = x.contiguous(), w.contiguous()
        att_src, att_dst = att_src.contiguous().view(-1), att_dst.contiguous().view(-1)
        bias = _contig(bias)
        _hip.on_device(x, w, att_src, att_dst, bias)
        M, Fi = x.shape
        HC = w.shape[0]
        H, C = heads, HC // heads
        assert M == graph.M and w.shape == (H * C, Fi)
        dev = x.device
        out = torch.empty(M, HC if concat else C, device=dev, dtype=_f32)
        y = torch.empty(M, HC, device=dev, dtype=_f32)
        o = torch.empty(M, HC, device=dev, dtype=_f32)
        stats = torch.empty(4, M, H, device=dev, dtype=_f32)
        _call("gcm_csr_gatconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(w),
              _hip.ptr(att_src), _hip.ptr(att_dst), _hip.ptr(bias), _hip.ptr(out), _hip.ptr(y), _hip.ptr(o),
              _hip.ptr(stats[0]), _hip.ptr(stats[1]), _hip.ptr(stats[2]), _hip.ptr(stats[3]), M, graph.E, Fi,
              H, C, int(concat), int(add_self_loops), float(slope), _hip.stream())
        ctx.save_for_backward(x, w, att_src, att_dst, y, stats)
        ctx.graph = graph
        ctx.cfg = (H, C, int(concat), int(add_self_loops), float(slope), bias is not None)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w, att_src, att_dst, y, stats = ctx.saved_tensors
        H, C, concat, loops, slope, has_bias = ctx.cfg
        graph = ctx.graph
        M, Fi = x.shape
        E = graph.E
        need_x, need_w, need_as, need_ad, need_b = ctx.needs_input_grad[:5]
        g_out = _hip.kernel_ready(g_out)
        lib = _hip.lib()
        col_ptr, rows, perm = _csc_or_none(graph, E > 0 and (need_x or need_w or need_as or need_ad))
        g_x = torch.empty_like(x) if need_x else None
        g_w = torch.empty_like(w) if need_w else None
        g_as = torch.empty(H * C, device=x.device, dtype=_f32) if need_as else None
        g_ad = torch.empty(H * C, device=x.device, dtype=_f32) if need_ad else None
        g_b = torch.empty(H * C if concat else C, device=x.device, dtype=_f32) if need_b and has_bias else None
        ws, ws_bytes = _scratch("gcm_csr_gatconv_bwd", M, E, Fi, H, C, concat, device=x.device)
        _call("gcm_csr_gatconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
              _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(perm), _hip.ptr(w), _hip.ptr(att_src),
              _hip.ptr(att_dst), _hip.ptr(y), _hip.ptr(stats[0]), _hip.ptr(stats[1]), _hip.ptr(stats[2]),
              _hip.ptr(stats[3]), _hip.ptr(g_x), _hip.ptr(g_w), _hip.ptr(g_as),
              _hip.ptr(g_ad), _hip.ptr(g_b), _hip.ptr(ws), ws_bytes, M, E, Fi, H, C, concat, loops, slope,
              _hip.stream())
        return g_x, g_w, g_as, g_ad, g_b, None, None, None, None, None


def csr_gatconv(x, w, att_src, att_dst, bias, graph, heads, concat, add_self_loops, slope):
    return _CsrGATConv.apply(x, w, att_src.view(-1), att_dst.view(-1), bias, graph, heads, concat,
                             add_self_loops, slope)


# ---------------------------------------------------------------------------
# DenseTransformerConv / TransformerConv (PyG; csrc/transformerconv.hip)
# ---------------------------------------------------------------------------
def _transformer_dims(w_all, heads, concat, root):
    """(H, C, D) from the stacked weight [3 H C + (D if root), Fi]: D = H C (concat) or C."""
    H = heads
    C = w_all.shape[0] // (3 * H + ((H if concat else 1) if root else 0))
    D = H * C if concat else C
    assert w_all.shape[0] == 3 * H * C + (D if root else 0), "w_all must stack [W_query; W_key; W_value; W_skip]"
    return H, C, D


class _DenseTransformerConv(torch.autograd.Function):
    """x [B,N,Fi], adj [B,N,N] (only its nonzero pattern is read: no gradient), w_all [P,Fi] / b_all [P] the stacked
    query, key, value (and skip) projections, w_beta [3 D] or None."""

    @staticmethod
    def forward(ctx, x, adj, w_all, b_all, w_beta, heads, concat, root, add_loop):
        x, adj, w_all, b_all = x.contiguous(), adj.contiguous(), w_all.contiguous(), b_all.contiguous()
        w_beta = None if w_beta is None else w_beta.contiguous().view(-1)
        _hip.on_device(x, adj, w_all, b_all, w_beta)
        B, N, Fi = x.shape
        H, C, D = _transformer_dims(w_all, heads, concat, root)
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert w_all.shape[1] == Fi and b_all.numel() == w_all.shape[0]
        assert w_beta is None or w_beta.numel() == 3 * D
        dims = (B, N, Fi, H, C, int(concat), int(root))
        out = torch.empty(B, N, D, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_dense_transformerconv_fwd", *dims, device=x.device)
        _call("gcm_dense_transformerconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w_all), _hip.ptr(b_all),
              _hip.ptr(w_beta), _hip.ptr(out), _hip.ptr(saved), saved_bytes, *dims, int(add_loop), _hip.stream())
        ctx.save_for_backward(x, w_all, w_beta, saved)
        ctx.dims = dims
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w_all, w_beta, saved = ctx.saved_tensors
        need_x, _, need_w, need_b, need_beta = ctx.needs_input_grad[:5]
        g_out = _hip.kernel_ready(g_out)
        g_x = torch.empty_like(x) if need_x else None
        g_w = torch.empty_like(w_all) if need_w else None
        g_b = torch.empty(w_all.shape[0], device=x.device, dtype=_f32) if need_b else None
        g_beta = torch.empty_like(w_beta) if need_beta and w_beta is not None else None
        ws, ws_bytes = _scratch("gcm_dense_transformerconv_bwd", *ctx.dims, device=x.device)
        _call("gcm_dense_transformerconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(w_all), _hip.ptr(w_beta),
              _hip.ptr(saved), _hip.ptr(g_x), _hip.ptr(g_w), _hip.ptr(g_b), _hip.ptr(g_beta), _hip.ptr(ws), ws_bytes,
              *ctx.dims, _hip.stream())
        return g_x, None, g_w, g_b, g_beta, None, None, None, None


def dense_transformerconv(x, adj, w_all, b_all, w_beta, heads, concat, root, add_loop):
    """-> out [B,N,D]; w_beta is viewed flat [3 D] (its gradient comes back in its own shape)."""
    return _DenseTransformerConv.apply(x, adj, w_all, b_all, w_beta, heads, concat, root, add_loop)


class _CsrTransformerConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_all, b_all, w_beta, graph, heads, concat, root):
        x, w_all, b_all = x.contiguous(), w_all.contiguous(), b_all.contiguous()
        w_beta = None if w_beta is None else w_beta.contiguous().view(-1)
        _hip.on_device(x, w_all, b_all, w_beta)
        M, Fi = x.shape
        H, C, D = _transformer_dims(w_all, heads, concat, root)
        assert M == graph.M and w_all.shape[1] == Fi and b_all.numel() == w_all.shape[0]
        assert w_beta is None or w_beta.numel() == 3 * D
        dims = (M, graph.E, Fi, H, C, int(concat), int(root))
        out = torch.empty(M, D, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_csr_transformerconv_fwd", *dims, device=x.device)
        _call("gcm_csr_transformerconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
              _hip.ptr(w_all), _hip.ptr(b_all), _hip.ptr(w_beta), _hip.ptr(out), _hip.ptr(saved), saved_bytes, *dims,
              _hip.stream())
        ctx.save_for_backward(x, w_all, w_beta, saved)
        ctx.graph, ctx.dims = graph, dims
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w_all, w_beta, saved = ctx.saved_tensors
        graph = ctx.graph
        need_x, need_w, need_b, need_beta = ctx.needs_input_grad[:4]
        g_out = _hip.kernel_ready(g_out)
        col_ptr, rows, perm = _csc_or_none(graph, graph.E > 0)
        g_x = torch.empty_like(x) if need_x else None
        g_w = torch.empty_like(w_all) if need_w else None
        g_b = torch.empty(w_all.shape[0], device=x.device, dtype=_f32) if need_b else None
        g_beta = torch.empty_like(w_beta) if need_beta and w_beta is not None else None
        ws, ws_bytes = _scratch("gcm_csr_transformerconv_bwd", *ctx.dims, device=x.device)
        _call("gcm_csr_transformerconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(graph.row_ptr),
              _hip.ptr(graph.col), _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(perm), _hip.ptr(w_all),
              _hip.ptr(w_beta), _hip.ptr(saved), _hip.ptr(g_x), _hip.ptr(g_w), _hip.ptr(g_b), _hip.ptr(g_beta),
              _hip.ptr(ws), ws_bytes, *ctx.dims, _hip.stream())
        return g_x, g_w, g_b, g_beta, None, None, None, None


def csr_transformerconv(x, w_all, b_all, w_beta, graph, heads, concat, root):
    return _CsrTransformerConv.apply(x, w_all, b_all, w_beta, graph, heads, concat, root)


# ---------------------------------------------------------------------------
# TransformerConv / DenseTransformerConv with edge_dim (gcm.transformer; csrc/transformer_edge.hip).  w_e [H*C, D] is
# lin_edge's weight; nothing per edge wider than D is formed, the forward saves u and abar [rows, H, D] beside what the
# edge-free forward saves.
# ---------------------------------------------------------------------------
def _tre_operands(x, edge_attr, w_all, b_all, w_e, w_beta, heads, concat, root):
    """Contiguous operands, checked against each other -> (operands, (Fi, H, C, D, Do))."""
    ops = [_contig(t) for t in (x, edge_attr, w_all, b_all, w_e, w_beta)]
    if ops[5] is not None:
        ops[5] = ops[5].view(-1)
    x, edge_attr, w_all, b_all, w_e, w_beta = ops
    _hip.on_device(*ops)
    Fi = x.shape[-1]
    H, C, Do = _transformer_dims(w_all, heads, concat, root)
    D = w_e.shape[1]
    assert w_all.shape[1] == Fi and b_all.numel() == w_all.shape[0]
    assert w_e.shape == (H * C, D) and edge_attr.shape[-1] == D
    assert w_beta is None or w_beta.numel() == 3 * Do
    return ops, (Fi, H, C, D, Do)


def _tre_grads(ctx, x, edge_attr, w_all, w_e, w_beta):
    """The outputs the backward call is to fill (None: skip): g_x, g_edge_attr, g_w_all, g_b_all, g_w_e, g_w_beta."""
    need = ctx.needs_input_grad
    return (torch.empty_like(x) if need[0] else None, torch.empty_like(edge_attr) if need[1] else None,
            torch.empty_like(w_all) if need[2] else None,
            torch.empty(w_all.shape[0], device=x.device, dtype=_f32) if need[3] else None,
            torch.empty_like(w_e) if need[4] else None,
            torch.empty_like(w_beta) if need[5] and w_beta is not None else None)


class _CsrTransformerEdge(torch.autograd.Function):
    """x [M,Fi], edge_attr [E,D] in the order of graph.edge_index."""

    @staticmethod
    def forward(ctx, x, edge_attr, w_all, b_all, w_e, w_beta, graph, heads, concat, root):
        ops, (Fi, H, C, D, Do) = _tre_operands(x, edge_attr, w_all, b_all, w_e, w_beta, heads, concat, root)
        x, edge_attr, w_all, b_all, w_e, w_beta = ops
        M = x.shape[0]
        assert M == graph.M and edge_attr.shape[0] == graph.E
        dims = (M, graph.E, Fi, H, C, D, int(concat), int(root))
        out = torch.empty(M, Do, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_csr_transformer_edge_fwd", *dims, device=x.device)
        _call("gcm_csr_transformer_edge_fwd", _hip.ptr(x), _hip.ptr(edge_attr), _hip.ptr(graph.row_ptr),
              _hip.ptr(graph.col), _hip.ptr(graph.csr_perm), _hip.ptr(w_all), _hip.ptr(b_all), _hip.ptr(w_e),
              _hip.ptr(w_beta), _hip.ptr(out), _hip.ptr(saved), saved_bytes, *dims, _hip.stream())
        ctx.save_for_backward(x, edge_attr, w_all, w_e, w_beta, saved)
        ctx.graph, ctx.dims = graph, dims
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, edge_attr, w_all, w_e, w_beta, saved = ctx.saved_tensors
        graph = ctx.graph
        g_out = _hip.kernel_ready(g_out)
        col_ptr, rows, perm = _csc_or_none(graph, graph.E > 0)
        g_x, g_ea, g_w, g_b, g_we, g_beta = _tre_grads(ctx, x, edge_attr, w_all, w_e, w_beta)
        ws, ws_bytes = _scratch("gcm_csr_transformer_edge_bwd", *ctx.dims, device=x.device)
        _call("gcm_csr_transformer_edge_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(edge_attr),
              _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(graph.csr_perm), _hip.ptr(col_ptr),
              _hip.ptr(rows), _hip.ptr(perm), _hip.ptr(w_all), _hip.ptr(w_e), _hip.ptr(w_beta), _hip.ptr(saved),
              _hip.ptr(g_x), _hip.ptr(g_w), _hip.ptr(g_b), _hip.ptr(g_we), _hip.ptr(g_beta), _hip.ptr(g_ea),
              _hip.ptr(ws), ws_bytes, *ctx.dims, _hip.stream())
        return g_x, g_ea, g_w, g_b, g_we, g_beta, None, None, None, None


def csr_transformer_edge(x, edge_attr, w_all, b_all, w_e, w_beta, graph, heads, concat, root):
    """-> out [M, H*C or C]; w_all / b_all / w_beta as csr_transformerconv's, w_e [H*C, D]."""
    return _CsrTransformerEdge.apply(x, edge_attr, w_all, b_all, w_e, w_beta, graph, heads, concat, root)


class _DenseTransformerEdge(torch.autograd.Function):
    """x [B,N,Fi], adj [B,N,N] (only its nonzero pattern is read: no gradient), edge_attr [B,N,N,D]."""

    @staticmethod
    def forward(ctx, x, edge_attr, w_all, b_all, w_e, w_beta, adj, heads, concat, root, add_loop):
        ops, (Fi, H, C, D, Do) = _tre_operands(x, edge_attr, w_all, b_all, w_e, w_beta, heads, concat, root)
        x, edge_attr, w_all, b_all, w_e, w_beta = ops
        adj = adj.contiguous()
        _hip.on_device(adj)
        B, N = x.shape[0], x.shape[1]
        assert adj.shape == (B, N, N) and edge_attr.shape == (B, N, N, D)
        dims = (B, N, Fi, H, C, D, int(concat), int(root))
        out = torch.empty(B, N, Do, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_dense_transformer_edge_fwd", *dims, device=x.device)
        _call("gcm_dense_transformer_edge_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(edge_attr), _hip.ptr(w_all),
              _hip.ptr(b_all), _hip.ptr(w_e), _hip.ptr(w_beta), _hip.ptr(out), _hip.ptr(saved), saved_bytes, *dims,
              int(add_loop), _hip.stream())
        ctx.save_for_backward(x, edge_attr, w_all, w_e, w_beta, saved)
        ctx.dims = dims
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, edge_attr, w_all, w_e, w_beta, saved = ctx.saved_tensors
        g_out = _hip.kernel_ready(g_out)
        g_x, g_ea, g_w, g_b, g_we, g_beta = _tre_grads(ctx, x, edge_attr, w_all, w_e, w_beta)
        ws, ws_bytes = _scratch("gcm_dense_transformer_edge_bwd", *ctx.dims, device=x.device)
        _call("gcm_dense_transformer_edge_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(edge_attr), _hip.ptr(w_all),
              _hip.ptr(w_e), _hip.ptr(w_beta), _hip.ptr(saved), _hip.ptr(g_x), _hip.ptr(g_w), _hip.ptr(g_b),
              _hip.ptr(g_we), _hip.ptr(g_beta), _hip.ptr(g_ea), _hip.ptr(ws), ws_bytes, *ctx.dims, _hip.stream())
        return g_x, g_ea, g_w, g_b, g_we, g_beta, None, None, None, None, None


def dense_transformer_edge(x, adj, edge_attr, w_all, b_all, w_e, w_beta, heads, concat, root, add_loop):
    """-> out [B,N, H*C or C]; g_edge_attr is written whole (zero where there is no term)."""
    return _DenseTransformerEdge.apply(x, edge_attr, w_all, b_all, w_e, w_beta, adj.detach(), heads, concat, root,
                                       add_loop)


# ---------------------------------------------------------------------------
# DenseResGatedGraphConv / ResGatedGraphConv (PyG; csrc/resgatedconv.hip)
# ---------------------------------------------------------------------------
def _resgated_dims(w_all, root):
    """C from the stacked weight [(4 if root else 3) C, Fi] = [W_key; W_query; W_value; W_skip]."""
    C, rest = divmod(w_all.shape[0], 4 if root else 3)
    assert rest == 0, "w_all must stack [W_key; W_query; W_value; W_skip]"
    return C


class _DenseResGatedConv(torch.autograd.Function):
    """x [B,N,Fi], adj [B,N,N] (values are weights, 0 is no edge; gets a gradient when it asks for one), w_all [P,Fi] /
    b_all [P] the stacked key, query, value (and skip) projections, bias [C] or None."""

    @staticmethod
    def forward(ctx, x, adj, w_all, b_all, bias, root, add_loop):
        x, adj, w_all, b_all = x.contiguous(), adj.contiguous(), w_all.contiguous(), b_all.contiguous()
        bias = _contig(bias)
        _hip.on_device(x, adj, w_all, b_all, bias)
        B, N, Fi = x.shape
        C = _resgated_dims(w_all, root)
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert w_all.shape[1] == Fi and b_all.numel() == w_all.shape[0]
        assert bias is None or bias.numel() == C
        dims = (B, N, Fi, C, int(root))
        out = torch.empty(B, N, C, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_dense_resgatedconv_fwd", *dims, device=x.device)
        _call("gcm_dense_resgatedconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w_all), _hip.ptr(b_all),
              _hip.ptr(bias), _hip.ptr(out), _hip.ptr(saved), saved_bytes, *dims, int(add_loop), _hip.stream())
        ctx.save_for_backward(x, adj, w_all, saved)
        ctx.dims, ctx.add_loop, ctx.has_bias = dims, int(add_loop), bias is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, adj, w_all, saved = ctx.saved_tensors
        need_x, need_adj, need_w, need_b, need_bias = ctx.needs_input_grad[:5]
        g_out = _hip.kernel_ready(g_out)
        C = ctx.dims[3]
        g_x = torch.empty_like(x) if need_x else None
        g_adj = torch.empty_like(adj) if need_adj else None
        g_w = torch.empty_like(w_all) if need_w else None
        g_b = torch.empty(w_all.shape[0], device=x.device, dtype=_f32) if need_b else None
        g_bias = torch.empty(C, device=x.device, dtype=_f32) if need_bias and ctx.has_bias else None
        ws, ws_bytes = _scratch("gcm_dense_resgatedconv_bwd", *ctx.dims, device=x.device)
        _call("gcm_dense_resgatedconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w_all),
              _hip.ptr(saved), _hip.ptr(g_x), _hip.ptr(g_w), _hip.ptr(g_b), _hip.ptr(g_bias), _hip.ptr(g_adj),
              _hip.ptr(ws), ws_bytes, *ctx.dims, ctx.add_loop, _hip.stream())
        return g_x, g_adj, g_w, g_b, g_bias, None, None


def dense_resgatedconv(x, adj, w_all, b_all, bias, root, add_loop):
    """-> out [B,N,C]."""
    return _DenseResGatedConv.apply(x, adj, w_all, b_all, bias, root, add_loop)


class _CsrResGatedConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_all, b_all, bias, graph, root):
        x, w_all, b_all = x.contiguous(), w_all.contiguous(), b_all.contiguous()
        bias = _contig(bias)
        _hip.on_device(x, w_all, b_all, bias)
        M, Fi = x.shape
        C = _resgated_dims(w_all, root)
        assert M == graph.M and w_all.shape[1] == Fi and b_all.numel() == w_all.shape[0]
        assert bias is None or bias.numel() == C
        dims = (M, graph.E, Fi, C, int(root))
        out = torch.empty(M, C, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_csr_resgatedconv_fwd", *dims, device=x.device)
        _call("gcm_csr_resgatedconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(w_all),
              _hip.ptr(b_all), _hip.ptr(bias), _hip.ptr(out), _hip.ptr(saved), saved_bytes, *dims, _hip.stream())
        ctx.save_for_backward(x, w_all, saved)
        ctx.graph, ctx.dims, ctx.has_bias = graph, dims, bias is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w_all, saved = ctx.saved_tensors
        graph = ctx.graph
        need_x, need_w, need_b, need_bias = ctx.needs_input_grad[:4]
        g_out = _hip.kernel_ready(g_out)
        col_ptr, rows, _ = _csc_or_none(graph, graph.E > 0)
        g_x = torch.empty_like(x) if need_x else None
        g_w = torch.empty_like(w_all) if need_w else None
        g_b = torch.empty(w_all.shape[0], device=x.device, dtype=_f32) if need_b else None
        g_bias = torch.empty(ctx.dims[3], device=x.device, dtype=_f32) if need_bias and ctx.has_bias else None
        ws, ws_bytes = _scratch("gcm_csr_resgatedconv_bwd", *ctx.dims, device=x.device)
        _call("gcm_csr_resgatedconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
              _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(w_all), _hip.ptr(saved), _hip.ptr(g_x), _hip.ptr(g_w),
              _hip.ptr(g_b), _hip.ptr(g_bias), _hip.ptr(ws), ws_bytes, *ctx.dims, _hip.stream())
        return g_x, g_w, g_b, g_bias, None, None


def csr_resgatedconv(x, w_all, b_all, bias, graph, root):
    return _CsrResGatedConv.apply(x, w_all, b_all, bias, graph, root)


# ---------------------------------------------------------------------------
# DenseGatedGraphConv / GatedGraphConv (PyG; csrc/gatedgraphconv.hip)
# ---------------------------------------------------------------------------
def _gated_operands(weight, w_ih, w_hh, b_ih, b_hh):
    """The contiguous parameters and (L, C) from weight [L,C,C], w_ih / w_hh [3C,C], b_ih / b_hh [3C] or None."""
    weight, w_ih, w_hh = weight.contiguous(), w_ih.contiguous(), w_hh.contiguous()
    b_ih = _contig(b_ih)
    b_hh = _contig(b_hh)
    L, C = weight.shape[0], weight.shape[1]
    assert weight.shape == (L, C, C) and w_ih.shape == (3 * C, C) and w_hh.shape == (3 * C, C)
    assert (b_ih is None or b_ih.numel() == 3 * C) and (b_hh is None or b_hh.numel() == 3 * C)
    return weight, w_ih, w_hh, b_ih, b_hh, L, C


def _gated_grads(ctx, weight, w_ih, first):
    """Empty gradients of (weight, w_ih, w_hh, b_ih, b_hh) where asked for; `first`: the index of weight among the
    inputs."""
    need = ctx.needs_input_grad[first:first + 5]
    C = weight.shape[1]
    g_weight = torch.empty_like(weight) if need[0] else None
    g_w_ih = torch.empty_like(w_ih) if need[1] else None
    g_w_hh = torch.empty_like(w_ih) if need[2] else None
    g_b_ih = torch.empty(3 * C, device=weight.device, dtype=_f32) if need[3] and ctx.has_bias[0] else None
    g_b_hh = torch.empty(3 * C, device=weight.device, dtype=_f32) if need[4] and ctx.has_bias[1] else None
    return g_weight, g_w_ih, g_w_hh, g_b_ih, g_b_hh


class _DenseGatedGraphConv(torch.autograd.Function):
    """x [B,N,Fi] (Fi <= C), adj [B,N,N] (values are weights, 0 is no edge; gets a gradient when it asks for one),
    weight [L,C,C], the GRU cell's w_ih / w_hh [3C,C] and b_ih / b_hh [3C] or None."""

    @staticmethod
    def forward(ctx, x, adj, weight, w_ih, w_hh, b_ih, b_hh, add_loop):
        x, adj = x.contiguous(), adj.contiguous()
        weight, w_ih, w_hh, b_ih, b_hh, L, C = _gated_operands(weight, w_ih, w_hh, b_ih, b_hh)
        _hip.on_device(x, adj, weight, w_ih, w_hh, b_ih, b_hh)
        B, N, Fi = x.shape
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        out = torch.empty(B, N, C, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_dense_gatedgraphconv_fwd", B, N, C, L, device=x.device)
        _call("gcm_dense_gatedgraphconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(weight), _hip.ptr(w_ih),
              _hip.ptr(w_hh), _hip.ptr(b_ih), _hip.ptr(b_hh), _hip.ptr(out), _hip.ptr(saved), saved_bytes, B, N, Fi,
              C, L, int(add_loop), _hip.stream())
        ctx.save_for_backward(adj, weight, w_ih, w_hh, saved)
        ctx.dims, ctx.add_loop, ctx.has_bias = (B, N, Fi, C, L), int(add_loop), (b_ih is not None, b_hh is not None)
        return out

    @staticmethod
    def backward(ctx, g_out):
        adj, weight, w_ih, w_hh, saved = ctx.saved_tensors
        B, N, Fi, C, L = ctx.dims
        need_x, need_adj = ctx.needs_input_grad[:2]
        g_out = _hip.kernel_ready(g_out)
        g_x = torch.empty(B, N, Fi, device=adj.device, dtype=_f32) if need_x else None
        g_adj = torch.empty_like(adj) if need_adj else None
        g_weight, g_w_ih, g_w_hh, g_b_ih, g_b_hh = _gated_grads(ctx, weight, w_ih, 2)
        ws, ws_bytes = _scratch("gcm_dense_gatedgraphconv_bwd", B, N, C, L, device=adj.device)
        _call("gcm_dense_gatedgraphconv_bwd", _hip.ptr(g_out), _hip.ptr(adj), _hip.ptr(weight), _hip.ptr(w_ih),
              _hip.ptr(w_hh), _hip.ptr(saved), _hip.ptr(g_x), _hip.ptr(g_weight), _hip.ptr(g_w_ih), _hip.ptr(g_w_hh),
              _hip.ptr(g_b_ih), _hip.ptr(g_b_hh), _hip.ptr(g_adj), _hip.ptr(ws), ws_bytes, B, N, Fi, C, L,
              ctx.add_loop, _hip.stream())
        return g_x, g_adj, g_weight, g_w_ih, g_w_hh, g_b_ih, g_b_hh, None


def dense_gatedgraphconv(x, adj, weight, w_ih, w_hh, b_ih, b_hh, add_loop):
    """-> out [B,N,C]."""
    return _DenseGatedGraphConv.apply(x, adj, weight, w_ih, w_hh, b_ih, b_hh, add_loop)


class _CsrGatedGraphConv(torch.autograd.Function):
    """x [M,Fi] (Fi <= C); w_edge [E] in CSR order or None."""

    @staticmethod
    def forward(ctx, x, w_edge, weight, w_ih, w_hh, b_ih, b_hh, graph):
        x = x.contiguous()
        w_edge = _contig(w_edge)
        weight, w_ih, w_hh, b_ih, b_hh, L, C = _gated_operands(weight, w_ih, w_hh, b_ih, b_hh)
        _hip.on_device(x, w_edge, weight, w_ih, w_hh, b_ih, b_hh)
        M, Fi = x.shape
        assert M == graph.M and (w_edge is None or w_edge.numel() == graph.E)
        out = torch.empty(M, C, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_csr_gatedgraphconv_fwd", M, graph.E, C, L, device=x.device)
        _call("gcm_csr_gatedgraphconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
              _hip.ptr(w_edge), _hip.ptr(weight), _hip.ptr(w_ih), _hip.ptr(w_hh), _hip.ptr(b_ih), _hip.ptr(b_hh),
              _hip.ptr(out), _hip.ptr(saved), saved_bytes, M, graph.E, Fi, C, L, _hip.stream())
        ctx.save_for_backward(w_edge, weight, w_ih, w_hh, saved)
        ctx.graph, ctx.dims, ctx.has_bias = graph, (M, graph.E, Fi, C, L), (b_ih is not None, b_hh is not None)
        return out

    @staticmethod
    def backward(ctx, g_out):
        w_edge, weight, w_ih, w_hh, saved = ctx.saved_tensors
        graph = ctx.graph
        M, E, Fi, C, L = ctx.dims
        need_x, need_we = ctx.needs_input_grad[:2]
        need_we = need_we and w_edge is not None
        g_out = _hip.kernel_ready(g_out)
        col_ptr, rows, perm = _csc_or_none(graph, E > 0)
        g_x = torch.empty(M, Fi, device=g_out.device, dtype=_f32) if need_x else None
        g_we = torch.zeros_like(w_edge) if need_we else None
        g_weight, g_w_ih, g_w_hh, g_b_ih, g_b_hh = _gated_grads(ctx, weight, w_ih, 2)
        ws, ws_bytes = _scratch("gcm_csr_gatedgraphconv_bwd", M, E, C, L, device=g_out.device)
        _call("gcm_csr_gatedgraphconv_bwd", _hip.ptr(g_out), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
              _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(perm), _hip.ptr(w_edge), _hip.ptr(weight), _hip.ptr(w_ih),
              _hip.ptr(w_hh), _hip.ptr(saved), _hip.ptr(g_x), _hip.ptr(g_weight), _hip.ptr(g_w_ih), _hip.ptr(g_w_hh),
              _hip.ptr(g_b_ih), _hip.ptr(g_b_hh), _hip.ptr(g_we), _hip.ptr(ws), ws_bytes, M, E, Fi, C, L,
              _hip.stream())
        return g_x, g_we, g_weight, g_w_ih, g_w_hh, g_b_ih, g_b_hh, None


def csr_gatedgraphconv(x, w_edge, weight, w_ih, w_hh, b_ih, b_hh, graph):
    return _CsrGatedGraphConv.apply(x, w_edge, weight, w_ih, w_hh, b_ih, b_hh, graph)


# ---------------------------------------------------------------------------
# DenseTAGConv / TAGConv (PyG; csrc/tagconv.hip)
# ---------------------------------------------------------------------------
class _DenseTagConv(torch.autograd.Function):
    """x [B,N,Fi], adj [B,N,N] (adj[b,i,j]: the weight of j -> i; gets a gradient when it asks for one), weight
    [K+1,Fo,Fi] (the hop matrices stacked), bias [Fo] or None."""

    @staticmethod
    def forward(ctx, x, adj, weight, bias, normalize, add_loop):
        x, adj, weight = x.contiguous(), adj.contiguous(), weight.contiguous()
        bias = _contig(bias)
        _hip.on_device(x, adj, weight, bias)
        B, N, Fi = x.shape
        K, Fo = weight.shape[0] - 1, weight.shape[1]
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert weight.shape == (K + 1, Fo, Fi) and (bias is None or bias.numel() == Fo)
        out = torch.empty(B, N, Fo, device=x.device, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_dense_tagconv_fwd", B, N, Fi, K, device=x.device)
        _call("gcm_dense_tagconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(weight), _hip.ptr(bias), _hip.ptr(out),
              _hip.ptr(saved), saved_bytes, B, N, Fi, Fo, K, int(normalize), int(add_loop), _hip.stream())
        ctx.save_for_backward(x, adj, weight, saved)
        ctx.dims, ctx.flags, ctx.has_bias = (B, N, Fi, Fo, K), (int(normalize), int(add_loop)), bias is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, adj, weight, saved = ctx.saved_tensors
        B, N, Fi, Fo, K = ctx.dims
        need_x, need_adj, need_w, need_b = ctx.needs_input_grad[:4]
        need_b = need_b and ctx.has_bias
        g_out = _hip.kernel_ready(g_out)
        g_x = torch.empty_like(x) if need_x else None
        g_adj = torch.empty_like(adj) if need_adj else None
        g_w = torch.empty_like(weight) if need_w else None
        g_b = torch.empty(Fo, device=x.device, dtype=_f32) if need_b else None
        ws, ws_bytes = _scratch("gcm_dense_tagconv_bwd", B, N, Fi, Fo, K, device=x.device)
        _call("gcm_dense_tagconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(adj), _hip.ptr(weight), _hip.ptr(saved),
              _hip.ptr(g_x), _hip.ptr(g_adj), _hip.ptr(g_w), _hip.ptr(g_b), _hip.ptr(ws), ws_bytes, B, N, Fi, Fo, K,
              ctx.flags[0], ctx.flags[1], _hip.stream())
        return g_x, g_adj, g_w, g_b, None, None


def dense_tagconv(x, adj, weight, bias, normalize, add_loop):
    """-> out [B,N,Fo]."""
    return _DenseTagConv.apply(x, adj, weight, bias, normalize, add_loop)


class _CsrTagConv(torch.autograd.Function):
    """x [M,Fi]; w_edge [E] in CSR order or None (unit weights); weight [K+1,Fo,Fi]."""

    @staticmethod
    def forward(ctx, x, w_edge, weight, bias, graph, normalize):
        x, weight = x.contiguous(), weight.contiguous()
        bias = _contig(bias)
        w_edge = _contig(w_edge)
        _hip.on_device(x, w_edge, weight, bias)
        M, Fi = x.shape
        K, Fo = weight.shape[0] - 1, weight.shape[1]
        E = graph.E
        assert M == graph.M and (w_edge is None or w_edge.numel() == E)
        assert weight.shape == (K + 1, Fo, Fi) and (bias is None or bias.numel() == Fo)
        dev = x.device
        dst, coef, dinv, _, _, _ = _gcn_norm(graph, w_edge, normalize, 0, 0.0)     # no loop terms are added here
        out = torch.empty(M, Fo, device=dev, dtype=_f32)
        saved, saved_bytes = _scratch("gcm_csr_tagconv_fwd", M, Fi, K, device=dev)
        _call("gcm_csr_tagconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(coef),
              _hip.ptr(weight), _hip.ptr(bias), _hip.ptr(out), _hip.ptr(saved), saved_bytes, M, E, Fi, Fo, K,
              _hip.stream())
        ctx.save_for_backward(x, weight, dst, coef, dinv, saved)
        ctx.graph, ctx.dims, ctx.has_bias = graph, (M, E, Fi, Fo, K), bias is not None
        ctx.normalize, ctx.has_w = int(normalize), w_edge is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, weight, dst, coef, dinv, saved = ctx.saved_tensors
        graph = ctx.graph
        M, E, Fi, Fo, K = ctx.dims
        need_x, need_we, need_w, need_b = ctx.needs_input_grad[:4]
        need_b = need_b and ctx.has_bias
        need_we = need_we and ctx.has_w
        g_out = _hip.kernel_ready(g_out)
        dev = x.device
        col_ptr, rows, perm = _csc_or_none(graph, (need_x or need_we) and E > 0)
        g_x = torch.empty_like(x) if need_x else None
        g_we = torch.zeros(E, device=dev, dtype=_f32) if need_we else None
        g_w = torch.empty_like(weight) if need_w else None
        g_b = torch.empty(Fo, device=dev, dtype=_f32) if need_b else None
        ws, ws_bytes = _scratch("gcm_csr_tagconv_bwd", M, E, Fi, Fo, K, device=dev)
        _call("gcm_csr_tagconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
              _hip.ptr(dst), _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(perm), _hip.ptr(coef), _hip.ptr(dinv),
              _hip.ptr(weight), _hip.ptr(saved), _hip.ptr(g_x), _hip.ptr(g_we), _hip.ptr(g_w), _hip.ptr(g_b),
              _hip.ptr(ws), ws_bytes, M, E, Fi, Fo, K, ctx.normalize, _hip.stream())
        return g_x, g_we, g_w, g_b, None, None


def csr_tagconv(x, w_edge, weight, bias, graph, normalize):
    return _CsrTagConv.apply(x, w_edge, weight, bias, graph, normalize)


# ---------------------------------------------------------------------------
# mean / max aggregation: GraphConv(aggr=...), SAGEConv and their dense forms (csrc/aggrconv.hip)
# ---------------------------------------------------------------------------
AGGR = {"mean": _hip.AGGR_MEAN, "max": _hip.AGGR_MAX}


class _DenseAggrConv(torch.autograd.Function):
    """out = agg(adj, x) W_rel^T + x W_root^T + bias; w_root and bias may be None."""

    @staticmethod
    def forward(ctx, x, adj, w_rel, w_root, bias, aggr):
        x, adj, w_rel = x.contiguous(), adj.contiguous(), w_rel.contiguous()
        w_root = _contig(w_root)
        bias = _contig(bias)
        _hip.on_device(x, adj, w_rel, w_root, bias)
        B, N, Fi = x.shape
        Fo = w_rel.shape[0]
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert w_rel.shape == (Fo, Fi) and (w_root is None or w_root.shape == (Fo, Fi))
        dev = x.device
        out = torch.empty(B, N, Fo, device=dev, dtype=_f32)
        agg = torch.empty(B, N, Fi, device=dev, dtype=_f32)
        deg = dinv = winner = None
        if aggr == _hip.AGGR_MEAN:
            deg = torch.empty(B, N, device=dev, dtype=_f32)
            dinv = torch.empty(B, N, device=dev, dtype=_f32)
        else:
            winner = torch.empty(B, N, Fi, device=dev, dtype=torch.int16)
        _call("gcm_dense_aggrconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w_rel), _hip.ptr(w_root), _hip.ptr(bias),
              _hip.ptr(out), _hip.ptr(agg), _hip.ptr(deg), _hip.ptr(dinv), _hip.ptr(winner), B, N, Fi, Fo, aggr,
              _hip.stream())
        ctx.save_for_backward(x, adj, w_rel, w_root, agg, deg, dinv, winner)
        ctx.aggr, ctx.has_bias = aggr, bias is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, adj, w_rel, w_root, agg, deg, dinv, winner = ctx.saved_tensors
        B, N, Fi = x.shape
        Fo = w_rel.shape[0]
        need_x, need_adj, need_wrel, need_wroot, need_b, _ = ctx.needs_input_grad
        need_b = need_b and ctx.has_bias
        need_wroot = need_wroot and w_root is not None
        need_adj = need_adj and ctx.aggr == _hip.AGGR_MEAN
        g_out = _hip.kernel_ready(g_out)
        dev = x.device
        g_x = torch.empty_like(x) if need_x else None
        g_adj = torch.empty_like(adj) if need_adj else None
        g_wrel = torch.empty_like(w_rel) if need_wrel else None
        g_wroot = torch.empty_like(w_root) if need_wroot else None
        g_b = torch.empty(Fo, device=dev, dtype=_f32) if need_b else None
        ws, ws_bytes = _scratch("gcm_dense_aggrconv_bwd", B, N, Fi, Fo, device=dev)
        _call("gcm_dense_aggrconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w_rel), _hip.ptr(w_root),
              _hip.ptr(agg), _hip.ptr(deg), _hip.ptr(dinv), _hip.ptr(winner), _hip.ptr(g_x), _hip.ptr(g_adj),
              _hip.ptr(g_wrel), _hip.ptr(g_wroot), _hip.ptr(g_b), _hip.ptr(ws), ws_bytes, B, N, Fi, Fo, ctx.aggr,
              _hip.stream())
        return g_x, g_adj, g_wrel, g_wroot, g_b, None


def dense_aggrconv(x, adj, w_rel, w_root, bias, aggr):
    """aggr: "mean" (adj values are weights and get a gradient) or "max" (pattern only: pass adj detached)."""
    return _DenseAggrConv.apply(x, adj, w_rel, w_root, bias, AGGR[aggr])


class _CsrAggrConv(torch.autograd.Function):
    """x [M,Fi]; w_edge [E] in CSR order or None (unit weights)."""

    @staticmethod
    def forward(ctx, x, w_edge, w_rel, w_root, bias, graph, aggr):
        x, w_rel = x.contiguous(), w_rel.contiguous()
        w_root = _contig(w_root)
        bias = _contig(bias)
        w_edge = _contig(w_edge)
        _hip.on_device(x, w_edge, w_rel, w_root, bias)
        M, Fi = x.shape
        Fo = w_rel.shape[0]
        E = graph.E
        assert M == graph.M
        assert w_rel.shape == (Fo, Fi) and (w_root is None or w_root.shape == (Fo, Fi))
        dev = x.device
        out = torch.empty(M, Fo, device=dev, dtype=_f32)
        agg = torch.empty(M, Fi, device=dev, dtype=_f32)
        winner = torch.empty(M, Fi, device=dev, dtype=torch.int32) if aggr == _hip.AGGR_MAX else None
        _call("gcm_csr_aggrconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(w_edge),
              _hip.ptr(w_rel), _hip.ptr(w_root), _hip.ptr(bias), _hip.ptr(out), _hip.ptr(agg), _hip.ptr(winner), M, E,
              Fi, Fo, aggr, _hip.stream())
        ctx.save_for_backward(x, w_edge, w_rel, w_root, agg, winner)
        ctx.graph, ctx.aggr, ctx.has_bias = graph, aggr, bias is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w_edge, w_rel, w_root, agg, winner = ctx.saved_tensors
        graph = ctx.graph
        M, Fi = x.shape
        Fo = w_rel.shape[0]
        E = graph.E
        need_x, need_we, need_wrel, need_wroot, need_b, _, _ = ctx.needs_input_grad
        need_b = need_b and ctx.has_bias
        need_wroot = need_wroot and w_root is not None
        need_we = need_we and w_edge is not None
        g_out = _hip.kernel_ready(g_out)
        dev = x.device
        wanted = (need_x or need_we) and E > 0
        col_ptr, rows, perm = _csc_or_none(graph, wanted)
        dst = graph.dst_csr() if wanted else None
        g_x = torch.empty_like(x) if need_x else None
        g_we = torch.zeros_like(w_edge) if need_we else None
        g_wrel = torch.empty_like(w_rel) if need_wrel else None
        g_wroot = torch.empty_like(w_root) if need_wroot else None
        g_b = torch.empty(Fo, device=dev, dtype=_f32) if need_b else None
        ws, ws_bytes = _scratch("gcm_csr_aggrconv_bwd", M, E, Fi, Fo, device=dev)
        _call("gcm_csr_aggrconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(agg), _hip.ptr(graph.row_ptr),
              _hip.ptr(graph.col), _hip.ptr(dst), _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(perm), _hip.ptr(w_edge),
              _hip.ptr(winner), _hip.ptr(w_rel), _hip.ptr(w_root), _hip.ptr(g_x), _hip.ptr(g_we), _hip.ptr(g_wrel),
              _hip.ptr(g_wroot), _hip.ptr(g_b), _hip.ptr(ws), ws_bytes, M, E, Fi, Fo, ctx.aggr, _hip.stream())
        return g_x, g_we, g_wrel, g_wroot, g_b, None, None


def csr_aggrconv(x, w_edge, w_rel, w_root, bias, graph, aggr):
    return _CsrAggrConv.apply(x, w_edge, w_rel, w_root, bias, graph, AGGR[aggr])


# ---------------------------------------------------------------------------
# PNAConv / DensePNAConv (csrc/pnaconv.hip)
# ---------------------------------------------------------------------------
PNA_AGGREGATORS = {"sum": _hip.PNA_SUM, "mean": _hip.PNA_MEAN, "min": _hip.PNA_MIN, "max": _hip.PNA_MAX,
                   "var": _hip.PNA_VAR, "std": _hip.PNA_STD}
PNA_SCALERS = {"identity": _hip.PNA_IDENTITY, "amplification": _hip.PNA_AMPLIFICATION,
               "attenuation": _hip.PNA_ATTENUATION, "linear": _hip.PNA_LINEAR,
               "inverse_linear": _hip.PNA_INVERSE_LINEAR}


def _pna_codes(names, table):
    """The list's codes packed 3 bits each from bit 0, as the C ABI takes them."""
    return sum(table[n] << (3 * i) for i, n in enumerate(names))


class PNAConfig:
    """What the kernels need to know of a PNA layer besides its tensors."""

    def __init__(self, in_channels, out_channels, towers, divide_input, aggregators, scalers):
        self.cin, self.cout, self.T, self.divide = in_channels, out_channels, towers, int(divide_input)
        self.A, self.S = len(aggregators), len(scalers)
        self.aggrs, self.scalers = _pna_codes(aggregators, PNA_AGGREGATORS), _pna_codes(scalers, PNA_SCALERS)
        self.Fi = in_channels // towers if divide_input else in_channels
        self.K1 = (1 + self.A * self.S) * self.Fi
        self.need_var = any(a in ("var", "std") for a in aggregators)
        self.need_mm = any(a in ("min", "max") for a in aggregators)

    def dims(self):
        return self.cin, self.cout, self.T, self.divide

    def lists(self):
        return self.aggrs, self.A, self.scalers, self.S


def _pna_saved(cfg, rows, dev, winner_dtype, has_lin):
    """What the forward keeps for the backward: ab, cat, h, cnt, stat, winner (None where the layer has no use)."""
    C = cfg.T * cfg.Fi
    ab = torch.empty(rows, 2 * C, device=dev, dtype=_f32)
    cat = torch.empty(rows, cfg.T * cfg.K1, device=dev, dtype=_f32)
    h = torch.empty(rows, cfg.cout, device=dev, dtype=_f32) if has_lin else None
    cnt = torch.empty(rows, device=dev, dtype=torch.int32)
    stat = torch.empty(rows, 2 * C, device=dev, dtype=_f32) if cfg.need_var else None
    winner = torch.empty(rows, 2 * C, device=dev, dtype=winner_dtype) if cfg.need_mm else None
    return ab, cat, h, cnt, stat, winner


def _pna_grads(ctx, operands):
    """Empty gradients for (x, w_pre, b_pre, w_post, b_post, w_lin, b_lin) where they are asked for."""
    return [torch.empty_like(t) if t is not None and need else None
            for t, need in zip(operands, ctx.needs_input_grad)]


class _DensePNAConv(torch.autograd.Function):
    """x [B,N,in], adj [B,N,N] (pattern only: no gradient); the operands stacked by tower as include/gcm_hip_pna.h
    lays them out; w_lin / b_lin None: the output is h (the towers' post linears side by side)."""

    @staticmethod
    def forward(ctx, x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, adj, cfg, add_loop):
        x, adj = x.contiguous(), adj.contiguous()
        w_pre, b_pre, w_post, b_post = (t.contiguous() for t in (w_pre, b_pre, w_post, b_post))
        w_lin, b_lin = _contig(w_lin), _contig(b_lin)
        _hip.on_device(x, adj, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg)
        B, N, cin = x.shape
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert cin == cfg.cin, f"x has {cin} channels, the layer takes {cfg.cin}"
        dev = x.device
        out = torch.empty(B, N, cfg.cout, device=dev, dtype=_f32)
        saved = _pna_saved(cfg, B * N, dev, torch.int16, w_lin is not None)
        _call("gcm_dense_pnaconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w_pre), _hip.ptr(b_pre), _hip.ptr(w_post),
              _hip.ptr(b_post), _hip.ptr(w_lin), _hip.ptr(b_lin), _hip.ptr(avg_deg), _hip.ptr(out),
              *[_hip.ptr(t) for t in saved], B, N, *cfg.dims(), *cfg.lists(), int(add_loop), _hip.stream())
        ctx.save_for_backward(x, adj, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, *saved)
        ctx.cfg, ctx.add_loop = cfg, int(add_loop)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, adj, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, ab, cat, h, cnt, stat, winner = ctx.saved_tensors
        cfg = ctx.cfg
        B, N, _ = x.shape
        g_out = _hip.kernel_ready(g_out)
        grads = _pna_grads(ctx, (x, w_pre, b_pre, w_post, b_post, w_lin, b_lin))
        ws, ws_bytes = _scratch("gcm_dense_pnaconv_bwd", B, N, *cfg.dims(), cfg.A, cfg.S, device=x.device)
        _call("gcm_dense_pnaconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(adj), _hip.ptr(w_pre), _hip.ptr(w_post),
              _hip.ptr(w_lin), _hip.ptr(avg_deg), _hip.ptr(ab), _hip.ptr(cat), _hip.ptr(h), _hip.ptr(cnt),
              _hip.ptr(stat), _hip.ptr(winner), *[_hip.ptr(g) for g in grads], _hip.ptr(ws), ws_bytes, B, N,
              *cfg.dims(), *cfg.lists(), ctx.add_loop, _hip.stream())
        return (*grads, None, None, None, None)


def dense_pnaconv(x, adj, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, cfg, add_loop):
    return _DensePNAConv.apply(x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, adj, cfg, add_loop)


class _CsrPNAConv(torch.autograd.Function):
    """x [M,in]; every CSR entry of `graph` is one message."""

    @staticmethod
    def forward(ctx, x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, graph, cfg):
        x = x.contiguous()
        w_pre, b_pre, w_post, b_post = (t.contiguous() for t in (w_pre, b_pre, w_post, b_post))
        w_lin, b_lin = _contig(w_lin), _contig(b_lin)
        _hip.on_device(x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg)
        M, cin = x.shape
        assert M == graph.M
        assert cin == cfg.cin, f"x has {cin} channels, the layer takes {cfg.cin}"
        dev = x.device
        out = torch.empty(M, cfg.cout, device=dev, dtype=_f32)
        saved = _pna_saved(cfg, M, dev, torch.int32, w_lin is not None)
        _call("gcm_csr_pnaconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(w_pre),
              _hip.ptr(b_pre), _hip.ptr(w_post), _hip.ptr(b_post), _hip.ptr(w_lin), _hip.ptr(b_lin), _hip.ptr(avg_deg),
              _hip.ptr(out), *[_hip.ptr(t) for t in saved], M, graph.E, *cfg.dims(), *cfg.lists(), _hip.stream())
        ctx.save_for_backward(x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, *saved)
        ctx.cfg, ctx.graph = cfg, graph
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, ab, cat, h, cnt, stat, winner = ctx.saved_tensors
        cfg, graph = ctx.cfg, ctx.graph
        M, E = graph.M, graph.E
        g_out = _hip.kernel_ready(g_out)
        grads = _pna_grads(ctx, (x, w_pre, b_pre, w_post, b_post, w_lin, b_lin))
        col_ptr, rows, perm = _csc_or_none(graph, E > 0 and any(g is not None for g in grads[:3]))
        ws, ws_bytes = _scratch("gcm_csr_pnaconv_bwd", M, E, *cfg.dims(), cfg.A, cfg.S, device=x.device)
        _call("gcm_csr_pnaconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(perm),
              _hip.ptr(w_pre), _hip.ptr(w_post), _hip.ptr(w_lin), _hip.ptr(avg_deg), _hip.ptr(ab), _hip.ptr(cat),
              _hip.ptr(h), _hip.ptr(cnt), _hip.ptr(stat), _hip.ptr(winner), *[_hip.ptr(g) for g in grads], _hip.ptr(ws),
              ws_bytes, M, E, *cfg.dims(), *cfg.lists(), _hip.stream())
        return (*grads, None, None, None)


def csr_pnaconv(x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, graph, cfg):
    return _CsrPNAConv.apply(x, w_pre, b_pre, w_post, b_post, w_lin, b_lin, avg_deg, graph, cfg)


# ---------------------------------------------------------------------------
# RGCNConv / DenseRGCNConv and TypedEdge's merge (csrc/rgcnconv.hip)
# ---------------------------------------------------------------------------
RGCN_MAX_RELATIONS = 16
RGCN_MAX_WIDTH = 128


def _rgcn_limits(Fi, Fo, R):
    if Fi > RGCN_MAX_WIDTH or Fo > RGCN_MAX_WIDTH or R > RGCN_MAX_RELATIONS:
        raise NotImplementedError(f"RGCNConv kernels cover in/out channels <= {RGCN_MAX_WIDTH} and <= "
                                  f"{RGCN_MAX_RELATIONS} relations; got {Fi} -> {Fo}, {R} relations")


def _rgcn_call(name, *args):
    rc = getattr(_hip.lib(), name)(*args)
    if rc == _hip.GCM_EUNSUPPORTED:
        raise NotImplementedError(f"{name}: shape outside what the kernels are built for")
    _hip.check(rc, name)


class _DenseRGCNConv(torch.autograd.Function):
    """x [B,N,Fi], adj / rel [B,N,N] float32, weight [R,Fi,Fo], root [Fi,Fo] or None, bias [Fo] or None."""

    @staticmethod
    def forward(ctx, x, adj, rel, weight, root, bias, mean):
        x, adj, rel, weight = x.contiguous(), adj.contiguous(), rel.contiguous(), weight.contiguous()
        root, bias = _contig(root), _contig(bias)
        _hip.on_device(x, adj, rel, weight, root, bias)
        B, N, Fi = x.shape
        R, _, Fo = weight.shape
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        assert rel.shape == (B, N, N) and rel.dtype == _f32, "rel must be a float32 [B, N, N]"
        assert weight.shape == (R, Fi, Fo) and (root is None or root.shape == (Fi, Fo))
        _rgcn_limits(Fi, Fo, R)
        dev = x.device
        out = torch.empty(B, N, Fo, device=dev, dtype=_f32)
        scale = torch.empty(B, R, N, device=dev, dtype=_f32) if mean else None
        ws, ws_bytes = _scratch("gcm_dense_rgcnconv_fwd", B, N, Fi, Fo, R, device=dev)
        _rgcn_call("gcm_dense_rgcnconv_fwd", _hip.ptr(x), _hip.ptr(adj), _hip.ptr(rel), _hip.ptr(weight),
                   _hip.ptr(root), _hip.ptr(bias), _hip.ptr(out), _hip.ptr(scale), _hip.ptr(ws), ws_bytes, B, N, Fi,
                   Fo, R, int(mean), _hip.stream())
        ctx.save_for_backward(x, adj, rel, weight, root, scale)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, adj, rel, weight, root, scale = ctx.saved_tensors
        B, N, Fi = x.shape
        R, _, Fo = weight.shape
        need_x, need_adj, _, need_w, need_root, need_b, _ = ctx.needs_input_grad
        need_root = need_root and root is not None
        need_b = need_b and ctx.has_bias
        g_out = _hip.kernel_ready(g_out)
        dev = x.device
        g_x = torch.empty_like(x) if need_x else None
        g_adj = torch.empty_like(adj) if need_adj else None
        g_w = torch.empty_like(weight) if need_w else None
        g_root = torch.empty_like(root) if need_root else None
        g_b = torch.empty(Fo, device=dev, dtype=_f32) if need_b else None
        ws, ws_bytes = _scratch("gcm_dense_rgcnconv_bwd", B, N, Fi, Fo, R, device=dev)
        _rgcn_call("gcm_dense_rgcnconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(adj), _hip.ptr(rel),
                   _hip.ptr(weight), _hip.ptr(root), _hip.ptr(scale), _hip.ptr(g_x), _hip.ptr(g_adj), _hip.ptr(g_w),
                   _hip.ptr(g_root), _hip.ptr(g_b), _hip.ptr(ws), ws_bytes, B, N, Fi, Fo, R, _hip.stream())
        return g_x, g_adj, None, g_w, g_root, g_b, None


def dense_rgcnconv(x, adj, rel, weight, root, bias, mean):
    return _DenseRGCNConv.apply(x, adj, rel, weight, root, bias, mean)


class _CsrRGCNConv(torch.autograd.Function):
    """x [M,Fi]; edge_type [E] int64 in CSR order: relation ids, or bit codes when mask_mode."""

    @staticmethod
    def forward(ctx, x, edge_type, weight, root, bias, graph, mean, mask_mode):
        x, weight = x.contiguous(), weight.contiguous()
        root, bias, edge_type = _contig(root), _contig(bias), edge_type.contiguous()
        _hip.on_device(x, edge_type, weight, root, bias)
        M, Fi = x.shape
        R, _, Fo = weight.shape
        E = graph.E
        assert M == graph.M and edge_type.numel() == E and edge_type.dtype == _i64
        assert weight.shape == (R, Fi, Fo) and (root is None or root.shape == (Fi, Fo))
        _rgcn_limits(Fi, Fo, R)
        dev = x.device
        out = torch.empty(M, Fo, device=dev, dtype=_f32)
        scale = torch.empty(M, R, device=dev, dtype=_f32) if mean else None
        ws, ws_bytes = _scratch("gcm_csr_rgcnconv_fwd", M, E, Fi, Fo, R, device=dev)
        _rgcn_call("gcm_csr_rgcnconv_fwd", _hip.ptr(x), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
                   _hip.ptr(edge_type), _hip.ptr(weight), _hip.ptr(root), _hip.ptr(bias), _hip.ptr(out),
                   _hip.ptr(scale), _hip.ptr(ws), ws_bytes, M, E, Fi, Fo, R, int(mean), int(mask_mode), _hip.stream())
        ctx.save_for_backward(x, edge_type, weight, root, scale)
        ctx.graph, ctx.has_bias, ctx.mask_mode = graph, bias is not None, int(mask_mode)
        return out

    @staticmethod
    def backward(ctx, g_out):
        x, edge_type, weight, root, scale = ctx.saved_tensors
        graph = ctx.graph
        M, Fi = x.shape
        R, _, Fo = weight.shape
        E = graph.E
        need_x, _, need_w, need_root, need_b, _, _, _ = ctx.needs_input_grad
        need_root = need_root and root is not None
        need_b = need_b and ctx.has_bias
        g_out = _hip.kernel_ready(g_out)
        dev = x.device
        col_ptr, rows, perm = _csc_or_none(graph, (need_x or need_w) and E > 0)
        g_x = torch.empty_like(x) if need_x else None
        g_w = torch.empty_like(weight) if need_w else None
        g_root = torch.empty_like(root) if need_root else None
        g_b = torch.empty(Fo, device=dev, dtype=_f32) if need_b else None
        ws, ws_bytes = _scratch("gcm_csr_rgcnconv_bwd", M, E, Fi, Fo, R, device=dev)
        _rgcn_call("gcm_csr_rgcnconv_bwd", _hip.ptr(g_out), _hip.ptr(x), _hip.ptr(edge_type), _hip.ptr(col_ptr),
                   _hip.ptr(rows), _hip.ptr(perm), _hip.ptr(weight), _hip.ptr(root), _hip.ptr(scale), _hip.ptr(g_x),
                   _hip.ptr(g_w), _hip.ptr(g_root), _hip.ptr(g_b), _hip.ptr(ws), ws_bytes, M, E, Fi, Fo, R,
                   ctx.mask_mode, _hip.stream())
        return g_x, None, g_w, g_root, g_b, None, None, None


def csr_rgcnconv(x, edge_type, weight, root, bias, graph, mean, mask_mode):
    return _CsrRGCNConv.apply(x, edge_type, weight, root, bias, graph, mean, mask_mode)


def typed_merge(adj, rel, children, bits, with_adj):
    """rel | the bits of the children's selections, and with_adj the diff_or of adj and the children: one launch.
    -> (adj_out or None, rel_out); nothing here carries a gradient."""
    adj, rel = adj.contiguous(), rel.contiguous()
    children = [c.detach().contiguous() for c in children]
    _hip.on_device(adj, rel, *children)
    assert rel.dtype == _f32 and all(c.shape == rel.shape and c.dtype == _f32 for c in children)
    K = len(children)
    adj_out = torch.empty_like(adj) if with_adj else None
    rel_out = torch.empty_like(rel)
    ptrs = (ctypes.c_void_p * K)(*[c.data_ptr() for c in children])
    codes = (ctypes.c_int * K)(*bits)
    _rgcn_call("gcm_typed_merge", _hip.ptr(adj), _hip.ptr(rel), ctypes.cast(ptrs, ctypes.c_void_p),
               ctypes.cast(codes, ctypes.c_void_p), K, _hip.ptr(adj_out), _hip.ptr(rel_out), rel.numel(),
               _hip.stream())
    return adj_out, rel_out


# ---------------------------------------------------------------------------
# GENConv / DenseGENConv (PyG, aggr="softmax"; csrc/genconv.hip): the softmax aggregation alone - lin_src / lin_dst,
# the message norm and the mlp stay in torch
# ---------------------------------------------------------------------------
def _gen_operands(xs, t):
    xs, t = xs.contiguous(), t.contiguous()
    _hip.on_device(xs, t)
    assert xs.dtype == _f32, "the GEN aggregation is float32 only"
    assert t.numel() == 1 and t.dtype == _f32
    return xs, t


class _DenseGENAgg(torch.autograd.Function):
    """agg_ic = sum_j a_ijc m_jc over {j: adj[b,i,j] != 0}, m = relu(xs) + eps, a = softmax_j(t m_jc); xs [B,N,C],
    adj [B,N,N] (pattern only: no gradient), t [1] (read on the device)."""

    @staticmethod
    def forward(ctx, xs, adj, t, eps):
        xs, t = _gen_operands(xs, t)
        adj = adj.contiguous()
        _hip.on_device(adj)
        B, N, C = xs.shape
        assert adj.shape == (B, N, N), "adj must be [B, N, N]"
        agg = torch.empty(B, N, C, device=xs.device, dtype=_f32)
        lse = torch.empty(2, B, N, C, device=xs.device, dtype=_f32)
        bits = torch.empty(B * N, (N + 63) // 64, device=xs.device, dtype=torch.int64)   # the pattern, 1 bit an entry
        _call("gcm_dense_gen_fwd", _hip.ptr(xs), _hip.ptr(adj), _hip.ptr(t), eps, _hip.ptr(agg), _hip.ptr(lse),
              _hip.ptr(bits), B, N, C, _hip.stream())
        ctx.save_for_backward(xs, bits, t, agg, lse)
        ctx.eps = eps
        return agg

    @staticmethod
    def backward(ctx, g_agg):
        xs, bits, t, agg, lse = ctx.saved_tensors
        B, N, C = xs.shape
        need_x, _, need_t, _ = ctx.needs_input_grad
        g_agg = _hip.kernel_ready(g_agg)
        g_xs = torch.empty_like(xs) if need_x else None
        g_t = torch.empty_like(t) if need_t else None
        ws, ws_bytes = _scratch("gcm_dense_gen_bwd", B, N, C, device=xs.device) if need_t else (None, 0)
        _call("gcm_dense_gen_bwd", _hip.ptr(g_agg), _hip.ptr(xs), _hip.ptr(bits), _hip.ptr(t), ctx.eps, _hip.ptr(agg),
              _hip.ptr(lse), _hip.ptr(g_xs), _hip.ptr(g_t), _hip.ptr(ws), ws_bytes, B, N, C, _hip.stream())
        return g_xs, None, g_t, None


def dense_genagg(xs, adj, t, eps=1e-7):
    return _DenseGENAgg.apply(xs, adj.detach(), t, float(eps))


class _CsrGENAgg(torch.autograd.Function):
    """The same aggregation over the in-edges of every node of `graph` (every CSR entry is one term); xs [M,C]."""

    @staticmethod
    def forward(ctx, xs, t, graph, eps):
        xs, t = _gen_operands(xs, t)
        M, C = xs.shape
        assert M == graph.M
        agg = torch.empty(M, C, device=xs.device, dtype=_f32)
        lse = torch.empty(2, M, C, device=xs.device, dtype=_f32)
        _call("gcm_csr_gen_fwd", _hip.ptr(xs), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(t), eps,
              _hip.ptr(agg), _hip.ptr(lse), M, graph.E, C, _hip.stream())
        ctx.save_for_backward(xs, t, agg, lse)
        ctx.graph, ctx.eps = graph, eps
        return agg

    @staticmethod
    def backward(ctx, g_agg):
        xs, t, agg, lse = ctx.saved_tensors
        graph = ctx.graph
        M, C = xs.shape
        E = graph.E
        need_x, need_t, _, _ = ctx.needs_input_grad
        g_agg = _hip.kernel_ready(g_agg)
        col_ptr, rows, _ = _csc_or_none(graph, need_x and E > 0)
        g_xs = torch.empty_like(xs) if need_x else None
        g_t = torch.empty_like(t) if need_t else None
        ws, ws_bytes = _scratch("gcm_csr_gen_bwd", M, E, C, device=xs.device) if need_t else (None, 0)
        _call("gcm_csr_gen_bwd", _hip.ptr(g_agg), _hip.ptr(xs), _hip.ptr(t), ctx.eps, _hip.ptr(agg), _hip.ptr(lse),
              _hip.ptr(graph.row_ptr), _hip.ptr(graph.col), _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(g_xs),
              _hip.ptr(g_t), _hip.ptr(ws), ws_bytes, M, E, C, _hip.stream())
        return g_xs, g_t, None, None


def csr_genagg(xs, t, graph, eps=1e-7):
    return _CsrGENAgg.apply(xs, t, graph, float(eps))


# ---------------------------------------------------------------------------
# EdgeConv / DenseEdgeConv (PyG, aggr="max"; csrc/edgeconv.hip): the per-edge stage - activation, second Linear and the
# running max with its winner.  The two node-level products P, Q of the first Linear stay in torch.
# ---------------------------------------------------------------------------
def _edgemax_operands(P, Q, w2, b2):
    P, Q, w2, b2 = P.contiguous(), Q.contiguous(), w2.contiguous(), _contig(b2)
    _hip.on_device(P, Q, w2, b2)
    assert P.dtype == _f32 and Q.dtype == _f32 and w2.dtype == _f32, "the EdgeConv kernels are float32 only"
    assert P.shape == Q.shape and w2.dim() == 2 and w2.shape[1] == P.shape[-1], "P, Q [.., H], W2 [C, H]"
    assert b2 is None or (b2.dtype == _f32 and b2.shape == (w2.shape[0],))
    return P, Q, w2, b2


def _edgemax_grads(ctx, slots, P, w2, b2_shape):
    """(g_P, g_Q, g_w2, g_b2): a fresh tensor for every input that needs a gradient, None (= skipped by the kernels) for
    the others; slots: the positions of P, Q, W2, b2 among the inputs."""
    need_p, need_q, need_w, need_b = (ctx.needs_input_grad[i] for i in slots)
    return (torch.empty_like(P) if need_p else None, torch.empty_like(P) if need_q else None,
            torch.empty_like(w2) if need_w else None,
            torch.empty(b2_shape, device=P.device, dtype=_f32) if need_b and b2_shape is not None else None)


class _DenseEdgeMax(torch.autograd.Function):
    """out_ic = max over {j: adj[b,i,j] != 0} of (W2 leaky_relu(P_i + Q_j) + b2)_c, 0 for an empty row; P, Q [B,N,H],
    adj [B,N,N] (pattern only: no gradient).  -> (out [B,N,C], winner [B,N,C] int32: the source index, -1 for none)."""
    @staticmethod
    def forward(ctx, P, Q, adj, w2, b2, slope):
        P, Q, w2, b2 = _edgemax_operands(P, Q, w2, b2)
        adj = adj.contiguous()
        _hip.on_device(adj)
        B, N, H = P.shape
        C = w2.shape[0]
        assert adj.shape == (B, N, N) and adj.dtype == _f32, "adj must be float32 [B, N, N]"
        out = torch.empty(B, N, C, device=P.device, dtype=_f32)
        winner = torch.empty(B, N, C, device=P.device, dtype=torch.int32)
        _call("gcm_dense_edgemax_fwd", _hip.ptr(P), _hip.ptr(Q), _hip.ptr(adj), _hip.ptr(w2), _hip.ptr(b2), slope,
              _hip.ptr(out), _hip.ptr(winner), B, N, H, C, _hip.stream())
        ctx.save_for_backward(P, Q, w2, winner)
        ctx.slope, ctx.b2_shape = slope, None if b2 is None else b2.shape
        ctx.mark_non_differentiable(winner)
        return out, winner

    @staticmethod
    def backward(ctx, g_out, _):
        P, Q, w2, winner = ctx.saved_tensors
        B, N, H = P.shape
        C = w2.shape[0]
        g_out = _hip.kernel_ready(g_out)
        g_P, g_Q, g_w2, g_b2 = _edgemax_grads(ctx, (0, 1, 3, 4), P, w2, ctx.b2_shape)
        ws, ws_bytes = (_scratch("gcm_dense_edgemax_bwd", B, N, H, C, device=P.device)
                        if g_w2 is not None or g_b2 is not None else (None, 0))
        _call("gcm_dense_edgemax_bwd", _hip.ptr(g_out), _hip.ptr(P), _hip.ptr(Q), _hip.ptr(winner), _hip.ptr(w2),
              ctx.slope, _hip.ptr(g_P), _hip.ptr(g_Q), _hip.ptr(g_w2), _hip.ptr(g_b2), _hip.ptr(ws), ws_bytes, B, N, H,
              C, _hip.stream())
        return g_P, g_Q, None, g_w2, g_b2, None


def dense_edgemax(P, Q, adj, W2, b2, slope, with_winner=False):
    out, winner = _DenseEdgeMax.apply(P, Q, adj.detach(), W2, b2, float(slope))
    return (out, winner) if with_winner else out


class _CsrEdgeMax(torch.autograd.Function):
    """The same over the in-edges of every node of `graph` (every CSR entry competes on its own); P, Q [M,H].
    -> (out [M,C], winner [M,C] int32: the CSR position of the winning entry, -1 for none)."""
    @staticmethod
    def forward(ctx, P, Q, w2, b2, slope, graph):
        P, Q, w2, b2 = _edgemax_operands(P, Q, w2, b2)
        M, H = P.shape
        C = w2.shape[0]
        assert M == graph.M
        out = torch.empty(M, C, device=P.device, dtype=_f32)
        winner = torch.empty(M, C, device=P.device, dtype=torch.int32)
        _call("gcm_csr_edgemax_fwd", _hip.ptr(P), _hip.ptr(Q), _hip.ptr(graph.row_ptr), _hip.ptr(graph.col),
              _hip.ptr(w2), _hip.ptr(b2), slope, _hip.ptr(out), _hip.ptr(winner), M, graph.E, H, C, _hip.stream())
        ctx.save_for_backward(P, Q, w2, winner)
        ctx.slope, ctx.b2_shape, ctx.graph = slope, None if b2 is None else b2.shape, graph
        ctx.mark_non_differentiable(winner)
        return out, winner

    @staticmethod
    def backward(ctx, g_out, _):
        P, Q, w2, winner = ctx.saved_tensors
        graph = ctx.graph
        M, H = P.shape
        C, E = w2.shape[0], graph.E
        g_out = _hip.kernel_ready(g_out)
        g_P, g_Q, g_w2, g_b2 = _edgemax_grads(ctx, (0, 1, 2, 3), P, w2, ctx.b2_shape)
        col_ptr, rows, perm = _csc_or_none(graph, g_Q is not None and E > 0)
        ws, ws_bytes = (_scratch("gcm_csr_edgemax_bwd", M, E, H, C, device=P.device)
                        if g_w2 is not None or g_b2 is not None else (None, 0))
        _call("gcm_csr_edgemax_bwd", _hip.ptr(g_out), _hip.ptr(P), _hip.ptr(Q), _hip.ptr(winner), _hip.ptr(graph.col),
              _hip.ptr(col_ptr), _hip.ptr(rows), _hip.ptr(perm), _hip.ptr(w2), ctx.slope, _hip.ptr(g_P), _hip.ptr(g_Q),
              _hip.ptr(g_w2), _hip.ptr(g_b2), _hip.ptr(ws), ws_bytes, M, E, H, C, _hip.stream())
        return g_P, g_Q, g_w2, g_b2, None, None


def csr_edgemax(P, Q, W2, b2, slope, graph, with_winner=False):
    out, winner = _CsrEdgeMax.apply(P, Q, W2, b2, float(slope), graph)
    return (out, winner) if with_winner else out


# ---------------------------------------------------------------------------
# gcm.nn.MessagePassing / gcm.graph_utils (csrc/message_passing.hip): rows gathered by an index, segments of rows
# reduced, a softmax over the rows of a segment.  Tensors are [rows, ...] float32; the kernels see C = the product of
# the trailing dimensions.
# ---------------------------------------------------------------------------
MP_OPS = {"sum": _hip.MP_SUM, "add": _hip.MP_SUM, "mean": _hip.MP_MEAN, "max": _hip.MP_MAX, "min": _hip.MP_MIN}


class Segments:
    """E rows grouped into M segments: `index` [E] is the segment of each row, (ptr [M+1], perm [E] | None) the list
    per segment - position p of segment i is row perm[p], or row p when the rows are in segment order already."""

    def __init__(self, index, ptr, perm, M):
        self.index, self.ptr, self.perm, self.M = index, ptr, perm, M
        self._inv_count = None

    @property
    def E(self):
        return self.index.numel()

    def inv_count(self):
        """1 / max(rows of the segment, 1) [M] float32: the scale of the mean's gradient."""
        if self._inv_count is None:
            self._inv_count = (self.ptr[1:] - self.ptr[:-1]).clamp_(min=1).to(_f32).reciprocal_()
        return self._inv_count

    @staticmethod
    def by_sink(graph):
        """The segments of GraphIndex `graph` by sink, rows in the order of graph.edge_index; cached on the graph."""
        seg = getattr(graph, "_mp_by_sink", None)
        if seg is None:
            seg = graph._mp_by_sink = Segments(graph.edge_index[1].contiguous(), graph.row_ptr, graph.csr_perm, graph.M)
        return seg

    @staticmethod
    def by_source(graph):
        """By source: the CSC view (built without a sort for SparseGCM's lists) composed with csr_perm."""
        seg = getattr(graph, "_mp_by_source", None)
        if seg is None:
            col_ptr, _, perm = graph.csc()
            if graph.csr_perm is not None:
                perm = graph.csr_perm[perm]
            seg = graph._mp_by_source = Segments(graph.edge_index[0].contiguous(), col_ptr, perm.contiguous(), graph.M)
        return seg

    @staticmethod
    def from_index(index, M):
        """Any [E] int64 index: a stable sort, as GraphIndex.from_edge_index."""
        index = index.contiguous()
        srt, perm = torch.sort(index, stable=True)
        return Segments(index, ptr_from_sorted(srt, M), perm, M)


def _mp_rows(t):
    """(contiguous t, C) of a float32 device tensor [rows, ...]."""
    t = t.contiguous()
    _hip.on_device(t)
    assert t.dtype == _f32 and t.dim() >= 1
    return t, torch.Size(t.shape[1:]).numel()


def _mp_gather(x, idx, scale, M):
    x, C = _mp_rows(x)
    out = torch.empty((idx.numel(),) + tuple(x.shape[1:]), device=x.device, dtype=_f32)
    _call("gcm_mp_gather", _hip.ptr(x), _hip.ptr(idx), _hip.ptr(scale), _hip.ptr(out), M, idx.numel(), C,
          _hip.stream())
    return out


def _mp_reduce(src, seg, op, arg=None):
    src, C = _mp_rows(src)
    out = torch.empty((seg.M,) + tuple(src.shape[1:]), device=src.device, dtype=_f32)
    _call("gcm_mp_reduce", _hip.ptr(src), _hip.ptr(seg.ptr), _hip.ptr(seg.perm), op, _hip.ptr(out), _hip.ptr(arg),
          seg.M, seg.E, C, _hip.stream())
    return out


class _MPGather(torch.autograd.Function):
    """out[e] = x[seg.index[e]]; the gradient is the segment sum of g over seg.  x [M, ...]."""

    @staticmethod
    def forward(ctx, x, seg):
        assert x.shape[0] == seg.M
        ctx.seg = seg
        return _mp_gather(x, seg.index, None, seg.M)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        return _mp_reduce(g, ctx.seg, _hip.MP_SUM), None


def mp_gather(x, seg):
    return _MPGather.apply(x, seg)


class _MPReduce(torch.autograd.Function):
    """out[i] = op over the rows of segment i of src [E, ...]; 0 for a segment without rows.  The gradient of max /
    min goes to the winning row alone, the first of its segment on a tie."""

    @staticmethod
    def forward(ctx, src, seg, op):
        assert src.shape[0] == seg.E
        arg = None
        if op in (_hip.MP_MAX, _hip.MP_MIN) and ctx.needs_input_grad[0]:
            arg = torch.empty((seg.M,) + tuple(src.shape[1:]), device=src.device, dtype=_i64)
            ctx.save_for_backward(arg)
        ctx.seg, ctx.op = seg, op
        return _mp_reduce(src, seg, op, arg)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        seg, op = ctx.seg, ctx.op
        if op in (_hip.MP_SUM, _hip.MP_MEAN):
            return _mp_gather(g, seg.index, seg.inv_count() if op == _hip.MP_MEAN else None, seg.M), None, None
        (arg,) = ctx.saved_tensors
        g, C = _mp_rows(g)
        g_src = torch.empty((seg.E,) + tuple(g.shape[1:]), device=g.device, dtype=_f32)
        _call("gcm_mp_select_bwd", _hip.ptr(g), _hip.ptr(arg), _hip.ptr(seg.index), _hip.ptr(g_src), seg.M, seg.E, C,
              _hip.stream())
        return g_src, None, None


def mp_reduce(src, seg, reduce):
    return _MPReduce.apply(src, seg, MP_OPS[reduce])


class _MPSoftmax(torch.autograd.Function):
    """out[e] = exp(src[e]) / sum over the rows of e's segment of exp(src), per trailing element."""

    @staticmethod
    def forward(ctx, src, seg):
        assert src.shape[0] == seg.E
        src, C = _mp_rows(src)
        out = torch.empty_like(src)
        _call("gcm_mp_softmax_fwd", _hip.ptr(src), _hip.ptr(seg.ptr), _hip.ptr(seg.perm), _hip.ptr(out), seg.M, seg.E,
              C, _hip.stream())
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(out)
        ctx.seg = seg
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        (out,) = ctx.saved_tensors
        seg = ctx.seg
        g, C = _mp_rows(g)
        g_src = torch.empty_like(out)
        _call("gcm_mp_softmax_bwd", _hip.ptr(g), _hip.ptr(out), _hip.ptr(seg.ptr), _hip.ptr(seg.perm), _hip.ptr(g_src),
              seg.M, seg.E, C, _hip.stream())
        return g_src, None


def mp_softmax(src, seg):
    return _MPSoftmax.apply(src, seg)


# ===========================================================================
# The dense <-> sparse bridge (gcm.gcm.DenseToSparse / SparseToDense; csrc/dense_sparse.hip, gcm_hip_bridge.h)
# ===========================================================================
BRIDGE_MAX_N = _hip.BRIDGE_MAX_N
_node_off_cache = {}


def _node_off(B, N, device):
    """[0, N, 2N, ..., B*N] on the device (GraphIndex.batches of a padded batch); kept per shape."""
    key = (B, N, device)
    off = _node_off_cache.get(key)
    if off is None:
        if len(_node_off_cache) >= 16:
            _node_off_cache.clear()
        off = _node_off_cache[key] = torch.arange(0, B * N + 1, N, dtype=_i64, device=device)
    return off


def dense_to_sparse(adj, transpose, with_values):
    """adj [B,N,N] (float32 or int64, N <= BRIDGE_MAX_N) -> (edge_index [2,E], GraphIndex, values [E] | None): the
    entries > 0 in (b, r, c) order as (b*N + r, b*N + c) - swapped with `transpose` - and their index by sink and by
    source, built by counting (no sort).  Three launches and ONE host read, of E; not differentiable (the caller
    wraps the values)."""
    adj = adj.contiguous()
    _hip.on_device(adj)
    assert adj.dim() == 3 and adj.shape[1] == adj.shape[2] and adj.dtype in (_f32, _i64)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("DenseToSparse reads the number of edges back to the host to size the edge list, which "
                           "a stream capture cannot do: run it outside torch.cuda.graph(...)")
    B, N = adj.shape[0], adj.shape[1]
    M, W, dev, st = B * N, (N + 63) // 64, adj.device, _hip.stream()
    is_i64 = int(adj.dtype == _i64)
    image = torch.empty(M * W, dtype=_i64, device=dev)
    counts = torch.empty(2 * M + B, dtype=torch.int32, device=dev)      # row counts | column counts | graph totals
    row_cnt, col_cnt, total = counts[:M], counts[M:2 * M], counts[2 * M:]
    graph_off = torch.empty(B + 1, dtype=_i64, device=dev)
    _call("gcm_bridge_image", _hip.ptr(adj), is_i64, _hip.ptr(image), _hip.ptr(row_cnt), _hip.ptr(col_cnt),
          _hip.ptr(total), B, N, st)
    _call("gcm_bridge_scan", _hip.ptr(total), _hip.ptr(graph_off), B, st)
    E = int(graph_off[B])                                               # the host read
    edge_index = torch.empty(2, E, dtype=_i64, device=dev)
    ptrs = torch.empty(2, M + 1, dtype=_i64, device=dev)
    by_col = torch.empty(E, dtype=_i64, device=dev)
    col_rows = torch.empty(E, dtype=_i64, device=dev)
    col_pos = None if transpose else torch.empty(E, dtype=_i64, device=dev)
    values = torch.empty(E, dtype=_f32, device=dev) if with_values else None
    _call("gcm_bridge_fill", _hip.ptr(adj), is_i64, _hip.ptr(image), _hip.ptr(row_cnt), _hip.ptr(col_cnt),
          _hip.ptr(graph_off), _hip.ptr(edge_index), _hip.ptr(ptrs[0]), _hip.ptr(ptrs[1]), _hip.ptr(by_col),
          _hip.ptr(col_pos), _hip.ptr(col_rows), _hip.ptr(values), B, N, E, int(transpose), st)
    batches = (_node_off(B, N, dev), B, N)
    if transpose:   # the row is the sink: the list is in CSR order already, the column-major order is its CSC
        graph = GraphIndex(edge_index, ptrs[0], M, batches=batches, col=edge_index[0],
                           csc=(ptrs[1], col_rows, by_col))
    else:           # the row is the source: the column-major order is the CSR, the list order its CSC
        graph = GraphIndex(edge_index, ptrs[1], M, csr_perm=by_col, batches=batches, col=col_rows,
                           csc=(ptrs[0], edge_index[1], col_pos))
    return edge_index, graph, values


class _BridgeValues(torch.autograd.Function):
    """DenseToSparse with edge values: values[e] = adj[b, r, c] of edge e, differentiable in adj (the gradient is
    scattered into a zero [B,N,N]); `out` receives (edge_index, graph)."""

    @staticmethod
    def forward(ctx, adj, transpose, out):
        edge_index, graph, values = dense_to_sparse(adj, transpose, True)
        out.extend((edge_index, graph))
        ctx.edge_index, ctx.transpose, ctx.dims = edge_index, transpose, adj.shape[:2]
        return values

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        B, N = ctx.dims
        g = g.contiguous()
        g_adj = torch.empty(B, N, N, dtype=_f32, device=g.device)
        _call("gcm_bridge_values_bwd", _hip.ptr(g), _hip.ptr(ctx.edge_index), _hip.ptr(g_adj), B, N, g.numel(),
              int(ctx.transpose), _hip.stream())
        return g_adj, None, None


def dense_to_sparse_values(adj, transpose):
    """-> (edge_index, graph, values) with values differentiable in a float32 adj."""
    if adj.dtype != _f32:
        return dense_to_sparse(adj, transpose, True)
    out = []
    values = _BridgeValues.apply(adj, transpose, out)
    return out[0], out[1], values


class _BridgeDenseNodes(torch.autograd.Function):
    """x [B,N,F] from x_sp [M,F]: node m at (its graph, m - first node of the graph), positions >= N dropped, the rest 0."""

    @staticmethod
    def forward(ctx, x_sp, batch_idx, node_ptr, B, N):
        x_sp = x_sp.contiguous()
        M, F = x_sp.shape
        x = torch.empty(B, N, F, dtype=_f32, device=x_sp.device)
        _call("gcm_bridge_dense_nodes", _hip.ptr(x_sp), _hip.ptr(node_ptr), _hip.ptr(x), M, B, N, F, _hip.stream())
        ctx.save_for_backward(batch_idx, node_ptr)
        ctx.dims = (M, B, N, F)
        return x

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        batch_idx, node_ptr = ctx.saved_tensors
        M, B, N, F = ctx.dims
        g = g.contiguous()
        g_sp = torch.empty(M, F, dtype=_f32, device=g.device)
        _call("gcm_bridge_dense_nodes_bwd", _hip.ptr(g), _hip.ptr(batch_idx), _hip.ptr(node_ptr), _hip.ptr(g_sp), M, B,
              N, F, _hip.stream())
        return g_sp, None, None, None, None


class _BridgeDenseAdj(torch.autograd.Function):
    """adj [B,N,N]: adj[b, s, d] += weight (or 1) per edge, summed per sink in CSR order; the gradient of the weights
    is a gather."""

    @staticmethod
    def forward(ctx, edge_weight, graph, batch_idx, node_ptr, B, N):
        dev = batch_idx.device
        adj = torch.empty(B, N, N, dtype=_f32, device=dev)
        _call("gcm_bridge_dense_adj", _hip.ptr(graph.row_ptr), _hip.ptr(graph.csr_perm), _hip.ptr(graph.edge_index),
              _hip.ptr(edge_weight), _hip.ptr(batch_idx), _hip.ptr(node_ptr), _hip.ptr(adj), graph.M, graph.E, B, N,
              _hip.stream())
        ctx.save_for_backward(batch_idx, node_ptr)
        ctx.graph, ctx.dims = graph, (B, N)
        return adj

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        batch_idx, node_ptr = ctx.saved_tensors
        graph, (B, N) = ctx.graph, ctx.dims
        g = g.contiguous()
        g_w = torch.empty(graph.E, dtype=_f32, device=g.device)
        _call("gcm_bridge_dense_adj_bwd", _hip.ptr(g), _hip.ptr(graph.edge_index), _hip.ptr(batch_idx),
              _hip.ptr(node_ptr), _hip.ptr(g_w), graph.M, graph.E, B, N, _hip.stream())
        return g_w, None, None, None, None, None


def sparse_to_dense(x_sp, graph, batch_idx, B, N, edge_weight=None):
    """(x [B,N,F], adj [B,N,N]) of flat nodes x_sp [M,F] float32, their non-decreasing graph ids batch_idx [M] and
    the edges of `graph` (a GraphIndex over the M nodes)."""
    batch_idx = batch_idx.contiguous()
    edge_index = graph.edge_index.contiguous()
    if edge_weight is not None:
        edge_weight = edge_weight.contiguous()
        assert edge_weight.dtype == _f32 and edge_weight.numel() == graph.E
    _hip.on_device(x_sp.contiguous(), batch_idx, edge_index, edge_weight)
    assert x_sp.dim() == 2 and x_sp.dtype == _f32 and batch_idx.dtype == _i64 and batch_idx.numel() == x_sp.shape[0]
    assert graph.M == x_sp.shape[0] and x_sp.shape[1] > 0
    if edge_index is not graph.edge_index:      # (a strided list: the kernels read [2,E] rows)
        graph = GraphIndex(edge_index, graph.row_ptr, graph.M, csr_perm=graph.csr_perm, col=graph.col)
    node_ptr = ptr_from_sorted(batch_idx, B)
    x = _BridgeDenseNodes.apply(x_sp, batch_idx, node_ptr, B, N)
    adj = _BridgeDenseAdj.apply(edge_weight, graph, batch_idx, node_ptr, B, N)
    return x, adj


# ===========================================================================
# LearnedEdge (edge_selectors/learned.py:53-125)
# ===========================================================================
class _LearnedPairs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nodes, cur):
        nodes = nodes.contiguous()
        _hip.on_device(nodes, cur)
        B, N, F = nodes.shape
        pairs = torch.empty(B, N, 2 * F, device=nodes.device, dtype=_f32)
        _call("gcm_learned_pairs_fwd", _hip.ptr(nodes), _hip.ptr(cur), _hip.ptr(pairs), B, N, F,
              _hip.stream())
        ctx.save_for_backward(cur)
        ctx.dims = (B, N, F)
        return pairs

    @staticmethod
    def backward(ctx, g_pairs):
        (cur,) = ctx.saved_tensors
        B, N, F = ctx.dims
        g_pairs = g_pairs.contiguous()
        g_nodes = torch.empty(B, N, F, device=g_pairs.device, dtype=_f32)
        _call("gcm_learned_pairs_bwd", _hip.ptr(g_pairs), _hip.ptr(cur), _hip.ptr(g_nodes), B, N, F,
              _hip.stream())
        return g_nodes, None


def learned_pairs(nodes, cur):
    return _LearnedPairs.apply(nodes, cur)


class _LearnedSelect(torch.autograd.Function):
    """new_adj = adj with row cur rewritten (in place on `adj`, which the caller owns)."""

    @staticmethod
    def forward(ctx, adj, logits, noise, cur, cutoff):
        logits, noise = logits.contiguous(), noise.contiguous()
        _hip.on_device(adj, logits, noise, cur)
        B, N, _ = adj.shape
        soft = torch.empty(B, N, device=adj.device, dtype=_f32)
        _call("gcm_learned_select_fwd", _hip.ptr(logits), _hip.ptr(noise), _hip.ptr(cur),
              float(cutoff), _hip.ptr(adj), _hip.ptr(soft), B, N, _hip.stream())
        ctx.mark_dirty(adj)
        ctx.save_for_backward(soft, cur)
        return adj

    @staticmethod
    def backward(ctx, g_adj):
        soft, cur = ctx.saved_tensors
        B, N = soft.shape
        g_adj = g_adj.contiguous()
        g_logits = torch.empty(B, N, device=g_adj.device, dtype=_f32)
        _call("gcm_learned_select_bwd", _hip.ptr(g_adj), _hip.ptr(soft), _hip.ptr(cur),
              _hip.ptr(g_logits), B, N, _hip.stream())
        # both straight-through estimators are identities, so the incoming adjacency receives
        # g_adj unchanged - also at the rewritten entries (learned.py:108-110 adds adj inside
        # the STE)
        return g_adj, g_logits, None, None, None


def learned_select_(adj, logits, noise, cur, cutoff):
    return _LearnedSelect.apply(adj, logits, noise, cur, cutoff)


class _LearnedSparsemax(torch.autograd.Function):
    """_LearnedSelect for LearnedEdge(deterministic=True) (learned.py:85-86): row cur of `adj` rewritten in place
    with the hard sparsemax of the logits (util.Spardmax) - no noise, no cutoff, no sample count."""

    @staticmethod
    def forward(ctx, adj, logits, cur):
        logits = logits.contiguous()
        _hip.on_device(adj, logits, cur)
        B, N, _ = adj.shape
        soft = torch.empty(B, N, device=adj.device, dtype=_f32)
        _call("gcm_learned_sparsemax_fwd", _hip.ptr(logits), _hip.ptr(cur), _hip.ptr(adj), _hip.ptr(soft), B, N,
              _hip.stream())
        ctx.mark_dirty(adj)
        ctx.save_for_backward(soft, cur)
        return adj

    @staticmethod
    def backward(ctx, g_adj):
        soft, cur = ctx.saved_tensors
        B, N = soft.shape
        g_adj = g_adj.contiguous()
        g_logits = torch.empty(B, N, device=g_adj.device, dtype=_f32)
        _call("gcm_learned_sparsemax_bwd", _hip.ptr(g_adj), _hip.ptr(soft), _hip.ptr(cur), _hip.ptr(g_logits),
              B, N, _hip.stream())
        # as _LearnedSelect: both straight-through estimators are identities
        return g_adj, g_logits, None


def learned_sparsemax_select_(adj, logits, cur):
    return _LearnedSparsemax.apply(adj, logits, cur)


# ===========================================================================
# fused canonical step / time-batched rollout (csrc/fused.hip, csrc/rollout.hip)
# ===========================================================================
def gnn2_supported(N, F, H1, H2):
    return bool(_hip.lib().gcm_dense_gnn2_row_supported(N, F, H1, H2))


class StepConfig:
    """Everything static about a fused DenseGCM configuration (built once per module/shape)."""

    def __init__(self, descs, acts, has_bias, N, F, H1, H2, device):
        lib = _hip.lib()
        self.descs = descs
        self.arr = (_hip.SelectorDesc * max(1, len(descs)))(*descs)
        self.arr_ptr = ctypes.addressof(self.arr)
        self.n_desc = len(descs)
        self.acts, self.has_bias = acts, has_bias
        self.N, self.F, self.H1, self.H2 = N, F, H1, H2
        self.P = lib.gcm_dense_gnn2_param_count(F, H1, H2)
        self.ws_bytes = 0
        self.ws = None
        self.device = device
        self.has_distance = any(d.kind == _hip.SEL_DISTANCE for d in descs)
        self._cpp, self._cpp_handle, self._cpp_call = None, None, None
        # the live-row step (rows_step.hip): index-writing selectors (<= 16 hops in all) and at most
        # one distance selector, which then runs ahead of the step on the incoming state
        n_dist = sum(1 for d in descs if d.kind == _hip.SEL_DISTANCE)
        self.rows_ok = bool(
            all(d.kind in (_hip.SEL_TEMPORAL, _hip.SEL_DENSE, _hip.SEL_DISTANCE) for d in descs)
            and n_dist <= 1 and not any(d.kind == _hip.SEL_DISTANCE and d.bidirectional for d in descs)
            and sum(d.n_hops for d in descs if d.kind == _hip.SEL_TEMPORAL) <= 16
            and lib.gcm_dense_rows_supported(N, F, H1, H2))
        self._rows_fast = None
        # ... and its form that also differentiates w.r.t. the observations / the incoming nodes
        self.dx_ok = bool(self.rows_ok and lib.gcm_dense_rows_dx_supported(N, F, H1, H2))

    # (Linear preprocessor | None, PositionalEncoding in "add" mode | None) folded into the live-row
    # step, or None (gcm.py:_fold_config)
    fold = None
    # Distance selectors of a batch-sharded run (EuclideanEdge(shard_group=...)): their current rows are
    # all-gathered ahead of every step (DenseGCM._gather_sharded)
    sharded = ()

    # -- DenseGCM + LearnedEdge (csrc/learned_step.hip) ----------------------------------------
    learned_sel = None          # the LearnedEdge module when this config is the fused learned step

    def set_learned(self, sel, mods):
        """sel: LearnedEdge with the default edge network `mods` (default_edge_network)."""
        lib = _hip.lib()
        self.learned_sel, self.mlp_mods = sel, mods
        self.Pm = lib.gcm_learned_mlp_param_count(self.F)
        self.P_total = self.P + self.Pm
        self.eps = (float(mods[2].eps), float(mods[5].eps))
        self.cutoff = 1.0 / (1 + sel.num_edge_samples)
        self.rows_ok = False

    def learned_cpp_handle(self):
        """address of the C++ twin of the learned-step config"""
        h = getattr(self, "_learned_cpp_h", None)
        if h is None:
            self._learned_cpp = _ext.module().LearnedCfg(self.N, self.F, self.H1, self.H2, self.acts[0], self.acts[1],
                                                         self.has_bias, self.eps[0], self.eps[1], self.cutoff)
            h = self._learned_cpp_h = self._learned_cpp.handle()
        return h

    _learned_fast = None

    def learned_fast(self, module):
        """The host path of a continuing LearnedEdge chain (C++: LearnedFast in csrc/torch_ext/step_ext.cpp), one per
        configuration - RowsFast's twin: parameters read through the modules' own `_parameters` dicts, the hook dicts
        torch.nn.Module.__call__ would consult, the selector's `__dict__` (an injected `noise_fn` declines)."""
        f = self._learned_fast
        if f is None:
            rel0, root0, rel1, root1 = self.lins
            specs = [(rel0._parameters, "weight"), (root0._parameters, "weight"), (rel0._parameters, "bias"),
                     (rel1._parameters, "weight"), (root1._parameters, "weight"), (rel1._parameters, "bias")]
            l0, _, n0, l1, _, n1, l2 = self.mlp_mods
            for m in (l0, n0, l1, n1, l2):
                specs += [(m._parameters, "weight"), (m._parameters, "bias")]
            from torch.nn.modules import module as M
            hooks = [module._forward_hooks, module._forward_pre_hooks, module._backward_hooks,
                     module._backward_pre_hooks, M._global_backward_pre_hooks, M._global_backward_hooks,
                     M._global_forward_pre_hooks, M._global_forward_hooks,
                     M._global_forward_hooks_always_called, M._global_forward_hooks_with_kwargs]
            f = self._learned_fast = _ext.module().LearnedFast(specs, hooks, self.learned_sel.__dict__)
        return f

    def rows_fast(self, module):
        """The host path of the live-row step (C++: RowsFast in csrc/torch_ext/step_ext.cpp), one per
        configuration: it validates a continuing chain by itself - hidden state returned by the
        previous call, same parameter objects at the same versions (read through the modules' own
        `_parameters` dicts) - and runs the step without the interpreter."""
        f = self._rows_fast
        if f is None:
            rel0, root0, rel1, root1 = self.lins
            specs = [(rel0._parameters, "weight"), (root0._parameters, "weight"), (rel0._parameters, "bias"),
                     (rel1._parameters, "weight"), (root1._parameters, "weight"), (rel1._parameters, "bias")]
            if self.fold is not None and self.fold[0] is not None:
                specs += [(self.fold[0]._parameters, "weight"), (self.fold[0]._parameters, "bias")]
            # the dicts torch.nn.Module.__call__ would consult: with any of them non-empty the unchecked
            # entry declines and the call goes through nn.Module.__call__
            from torch.nn.modules import module as M
            hooks = [module._forward_hooks, module._forward_pre_hooks, module._backward_hooks,
                     module._backward_pre_hooks, M._global_backward_pre_hooks, M._global_backward_hooks,
                     M._global_forward_pre_hooks, M._global_forward_hooks,
                     M._global_forward_hooks_always_called, M._global_forward_hooks_with_kwargs]
            f = self._rows_fast = _ext.module().RowsFast(specs, hooks)
        return f

    def cpp_handle(self):
        """address of the C++ twin of this config"""
        h = self._cpp_handle
        if h is None:
            self._cpp = _ext.module().StepCfg(self.arr_ptr, self.n_desc, self.acts[0], self.acts[1],
                                              self.has_bias, self.N, self.F, self.H1, self.H2)
            h = self._cpp_handle = self._cpp.handle()
        return h

    def cpp_call(self):
        """(ext.fused_step, config handle, device index): the C++ node of the per-step fused step"""
        c = self._cpp_call
        if c is None:
            c = self._cpp_call = (_ext.module().fused_step, self.cpp_handle(), self.device.index)
        return c

    def refresh_pointers(self):
        """re-read the device pointers baked into the selector descriptors (a re-assigned
        Distance.dist_param, the gathered current rows of a sharded EuclideanEdge) into this config and
        its C++ twin"""
        for i, (d, src) in enumerate(zip(self.descs, getattr(self, "desc_sources", ()))):
            if d.kind == _hip.SEL_DISTANCE and src is not None:
                p, rows, n_rows = src()
                d.dist_param = p
                self.arr[i].dist_param = p
                d.cur_rows, d.n_cur_rows = rows, n_rows
                self.arr[i].cur_rows, self.arr[i].n_cur_rows = rows, n_rows
        if self._cpp is not None:
            self._cpp.update_descs(self.arr_ptr, self.n_desc)

    def workspace(self, B):
        if not self.has_distance:
            return None, 0
        need = 0
        for d in self.descs:
            if d.kind == _hip.SEL_DISTANCE:
                need = max(need, _hip.lib().gcm_edge_distance_workspace_bytes(d.mode, max(B, d.n_cur_rows),
                                                                               self.N, self.F))
        if need > self.ws_bytes:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self.ws_bytes = need
        return (self.ws.data_ptr() if self.ws is not None else None), self.ws_bytes

    def unpack_ptrs(self, packed):
        """device pointers (w_rel1, b1, w_root1, w_rel2, b2, w_root2) into the packed vector"""
        F, H1, H2 = self.F, self.H1, self.H2
        base = packed.data_ptr()
        w_rel1 = base
        w_root1 = w_rel1 + 4 * H1 * F
        b1 = w_root1 + 4 * H1 * F
        w_rel2 = b1 + 4 * H1
        w_root2 = w_rel2 + 4 * H2 * H1
        b2 = w_root2 + 4 * H2 * H1
        return (w_rel1, b1 if self.has_bias & 1 else None, w_root1,
                w_rel2, b2 if self.has_bias & 2 else None, w_root2)


class SlabHolder:
    """The parameter-gradient slab arrays [B, P] of one packed parameter vector (one per batch size
    seen): every step's backward kernel accumulates into them, _ParamGate sums them once."""

    def __init__(self, P, device):
        self.P, self.device = P, device
        self.slabs = {}

    def get(self, B):
        t = self.slabs.get(B)
        if t is None:
            t = torch.zeros(B, self.P, device=self.device, dtype=_f32)
            self.slabs[B] = t
        return t


class _ParamGate(torch.autograd.Function):
    """Identity on the packed parameter vector, placed between it and the step nodes: its backward
    runs after every step node of the pass (they are its consumers) and produces the parameter
    gradient of ALL of them at once -
      * fused-step nodes (gcm_dense_step_bwd_slabs) accumulated per-graph slabs into `holder`:
        one slab sum instead of T slab sums and T engine-side adds;
    (The live-row steps do not pass through the gate: all of a chain's steps share one autograd node
    - RowsChainNode in csrc/torch_ext/step_ext.cpp - that consumes the packed vector directly.)"""

    @staticmethod
    def forward(ctx, packed, holder):
        ctx.holder = holder
        ctx.set_materialize_grads(False)
        return packed.view_as(packed)

    @staticmethod
    def backward(ctx, g):
        holder = ctx.holder
        total = g
        for B, slabs in holder.slabs.items():
            out = torch.empty(holder.P, device=slabs.device, dtype=_f32)
            _call("gcm_sum_slabs_acc", _hip.ptr(slabs), B, holder.P, _hip.ptr(total), _hip.ptr(out),
                  _hip.stream())
            slabs.zero_()
            total = out
        return total, None


def param_gate(packed, holder):
    return _ParamGate.apply(packed, holder)


# Time-parallel BPTT keeps T*B*(N*F + F + P) floats of scratch; above this many bytes the
# rollout backward runs step by step instead (2*B*N*F + B*P floats).  0 forces the sequential one.
ROLLOUT_BWD_BATCHED_MAX_BYTES = 16 << 30


class _FusedRollout(torch.autograd.Function):
    """T DenseGCM steps as ONE autograd node (gcm_dense_rollout_fwd/bwd)."""

    @staticmethod
    def forward(ctx, obs, nodes0, packed, adj0, num_nodes0, flags, cfg):
        obs = obs.contiguous()
        _hip.on_device(obs, nodes0, adj0, num_nodes0, flags)
        T, B, F = obs.shape
        N, H1, H2 = cfg.N, cfg.H1, cfg.H2
        dev = obs.device
        need_bwd = any(ctx.needs_input_grad)
        w = cfg.unpack_ptrs(packed)
        if not need_bwd:
            # inference: no history.  The persistent kernel keeps the state in LDS and writes the
            # final hidden state once (two-slot arrays); shapes / selectors it does not cover take
            # the general path below.
            nodes2 = torch.empty(2, B, N, F, device=dev, dtype=_f32)
            adj2 = torch.empty(2, B, N, N, device=dev, dtype=_f32)
            count2 = torch.empty(2, B, device=dev, dtype=torch.int64)
            nodes2[0].copy_(nodes0)
            adj2[0].copy_(adj0)
            count2[0].copy_(num_nodes0)
            mx_all = torch.empty(T, B, H2, device=dev, dtype=_f32)
            fn = _hip.lib().gcm_dense_rollout_persistent_fwd
            rc = fn(_hip.ptr(obs), _hip.ptr(nodes2), _hip.ptr(adj2), _hip.ptr(count2), None,
                    cfg.arr_ptr, cfg.n_desc, w[0], w[1], w[2], cfg.acts[0], w[3], w[4], w[5],
                    cfg.acts[1], _hip.ptr(mx_all), None, None, None, _hip.ptr(flags), 0, T, B, N, F,
                    H1, H2, _hip.stream())
            if rc == 0:
                adj_T, count_T = adj2[1], count2[1]
                ctx.mark_non_differentiable(adj_T, count_T)
                return mx_all, nodes2[1], adj_T, count_T
            if rc != _hip.GCM_EUNSUPPORTED:
                _hip.check(rc, "gcm_dense_rollout_persistent_fwd")
        nodes_all = torch.empty(T + 1, B, N, F, device=dev, dtype=_f32)
        adj_all = torch.empty(T + 1, B, N, N, device=dev, dtype=_f32)
        count_all = torch.empty(T + 1, B, device=dev, dtype=torch.int64)
        nodes_all[0].copy_(nodes0)
        adj_all[0].copy_(adj0)
        count_all[0].copy_(num_nodes0)
        cur_all = torch.empty(T, B, device=dev, dtype=torch.int64)
        mx_all = torch.empty(T, B, H2, device=dev, dtype=_f32)
        h1_all = torch.empty(T, B, N, H1, device=dev, dtype=_f32) if need_bwd else None
        agg1_all = torch.empty(T, B, N, F, device=dev, dtype=_f32) if need_bwd else None
        agg2_all = torch.empty(T, B, H1, device=dev, dtype=_f32) if need_bwd else None
        ws_ptr, ws_bytes = cfg.workspace(B)
        _call("gcm_dense_rollout_fwd", _hip.ptr(obs), _hip.ptr(nodes_all), _hip.ptr(adj_all),
              _hip.ptr(count_all), _hip.ptr(cur_all), cfg.arr_ptr, cfg.n_desc,
              w[0], w[1], w[2], cfg.acts[0], w[3], w[4], w[5], cfg.acts[1], _hip.ptr(mx_all),
              _hip.ptr(h1_all), _hip.ptr(agg1_all), _hip.ptr(agg2_all), _hip.ptr(flags), ws_ptr,
              ws_bytes, T, B, N, F, H1, H2, _hip.stream())
        ctx.save_for_backward(nodes_all, adj_all, count_all, cur_all, mx_all, h1_all, agg1_all,
                              agg2_all, packed)
        ctx.cfg, ctx.dims = cfg, (T, B)
        # clones: a view would pin the whole [T+1, ...] history for as long as the hidden lives
        nodes_T, adj_T, count_T = nodes_all[T].clone(), adj_all[T].clone(), count_all[T].clone()
        ctx.mark_non_differentiable(adj_T, count_T)
        return mx_all, nodes_T, adj_T, count_T

    @staticmethod
    def backward(ctx, g_mx_all, g_nodes_T, _g_adj, _g_count):
        (nodes_all, adj_all, count_all, cur_all, mx_all, h1_all, agg1_all, agg2_all,
         packed) = ctx.saved_tensors
        cfg = ctx.cfg
        T, B = ctx.dims
        N, F, H1, H2, P = cfg.N, cfg.F, cfg.H1, cfg.H2, cfg.P
        dev = nodes_all.device
        lib = _hip.lib()
        if g_mx_all is None:
            g_mx_all = torch.zeros(T, B, H2, device=dev)
        need = ctx.needs_input_grad
        if (not need[0] and not need[1] and g_mx_all.dtype == _f32
                and lib.gcm_dense_rows_supported(N, F, H1, H2)):
            # only the parameters need a gradient: every graph-step is independent - one launch over
            # the live rows of all T*B of them (csrc/rows_bptt.hip), no reverse scan, no Q array; an
            # expanded gradient (mean()) is read through its strides
            flat = torch.empty(P, device=dev, dtype=_f32)
            ws_bytes = lib.gcm_dense_rollout_bwd_params_workspace_bytes(T, B, F, H1, H2)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            st_t, st_b, st_h = g_mx_all.stride()
            _call("gcm_dense_rollout_bwd_params", _hip.ptr(g_mx_all), st_t, st_b, st_h, _hip.ptr(nodes_all),
                  _hip.ptr(adj_all), _hip.ptr(cur_all), packed.data_ptr(), cfg.acts[0], cfg.acts[1],
                  _hip.ptr(mx_all), _hip.ptr(h1_all), _hip.ptr(agg1_all), _hip.ptr(agg2_all), _hip.ptr(flat),
                  _hip.ptr(ws), ws_bytes, T, B, N, F, H1, H2, _hip.stream())
            return None, None, flat if need[2] else None, None, None, None, None
        g_mx_all = g_mx_all.contiguous()
        g_nodes_T = None if g_nodes_T is None else g_nodes_T.contiguous()
        g_obs = torch.empty(T, B, F, device=dev, dtype=_f32)
        g_nodes0 = torch.empty(B, N, F, device=dev, dtype=_f32)
        flat = torch.empty(P, device=dev, dtype=_f32)
        ws_bytes = lib.gcm_dense_rollout_bwd_batched_workspace_bytes(T, B, N, F, H1, H2)
        if ws_bytes > ROLLOUT_BWD_BATCHED_MAX_BYTES:
            ws_bytes = lib.gcm_dense_rollout_bwd_workspace_bytes(B, N, F, H1, H2)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        w = cfg.unpack_ptrs(packed)
        _call("gcm_dense_rollout_bwd", _hip.ptr(g_mx_all), _hip.ptr(g_nodes_T), _hip.ptr(nodes_all),
              _hip.ptr(adj_all), _hip.ptr(count_all), _hip.ptr(cur_all), w[0], w[1], w[2],
              cfg.acts[0], w[3], w[4], w[5], cfg.acts[1], _hip.ptr(mx_all), _hip.ptr(h1_all),
              _hip.ptr(agg1_all), _hip.ptr(agg2_all), _hip.ptr(g_obs), _hip.ptr(g_nodes0),
              _hip.ptr(flat), _hip.ptr(ws), ws_bytes, T, B, N, F, H1, H2, _hip.stream())
        need = ctx.needs_input_grad
        return (g_obs if need[0] else None, g_nodes0 if need[1] else None,
                flat if need[2] else None, None, None, None, None)


def fused_rollout(obs, nodes0, packed, adj0, num_nodes0, flags, cfg):
    return _FusedRollout.apply(obs, nodes0, packed, adj0, num_nodes0, flags, cfg)


def rows_linear(x2, weight, bias=None, transpose=False, ln=None, out=None, ldy=0):
    """csrc/rows_linear.hip on rows x2 [M, *]: x2 W^T + bias (transpose: x2 W).  ln = (gamma, beta, eps):
    -> (pre-activation, LayerNorm(relu(pre-activation))).  out/ldy: write into a wider matrix."""
    x2 = x2.contiguous()
    weight = weight.contiguous()
    _hip.on_device(x2, weight, bias)
    M = x2.shape[0]
    O, I = weight.shape
    n_out = I if transpose else O
    y = out if out is not None else torch.empty(M, n_out, device=x2.device, dtype=_f32)
    h = torch.empty(M, n_out, device=x2.device, dtype=_f32) if ln is not None else None
    _call("gcm_rows_linear", _hip.ptr(x2), _hip.ptr(weight), _hip.ptr(bias), _hip.ptr(y), M, I, O,
          int(transpose), ldy, _hip.ptr(ln[0]) if ln else None, _hip.ptr(ln[1]) if ln else None,
          float(ln[2]) if ln else 0.0, _hip.ptr(h), _hip.stream())
    return (y, h) if ln is not None else y


class _SkinnyLinear(torch.autograd.Function):
    """y = x W^T + b for many rows and narrow layers (<= 64 features: the LearnedEdge edge network, the
    PositionalEncoding re-projection): forward and dX are gcm_rows_linear (a row stream through the matrix
    cores), the weight gradient - a [O x M] x [M x I] product with M = B*N rows, which a library GEMM runs
    on one or two workgroups - is gcm_skinny_wgrad (rows split over the grid)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        y = rows_linear(x.reshape(-1, x.shape[-1]), weight, bias)
        return y.view(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad
        gx = None
        if need_x:
            gx = rows_linear(g.reshape(-1, weight.shape[0]), weight, transpose=True).view(x.shape)
        gw = gb = None
        if need_w or need_b:
            O, I = weight.shape
            g2 = g.reshape(-1, O).contiguous()
            x2 = x.reshape(-1, I).contiguous()
            M = g2.shape[0]
            lib = _hip.lib()
            ws_bytes = lib.gcm_skinny_wgrad_workspace_bytes(M, O, I)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g.device)
            out = torch.empty(O * I + O, device=g.device, dtype=_f32)
            _call("gcm_skinny_wgrad", _hip.ptr(g2), _hip.ptr(x2), _hip.ptr(out), _hip.ptr(ws), ws_bytes,
                  M, O, I, _hip.stream())
            gw = out[:O * I].view(O, I) if need_w else None
            gb = out[O * I:] if (need_b and ctx.has_bias) else None
        return gx, gw, gb


def skinny_linear(x, weight, bias):
    return _SkinnyLinear.apply(x, weight, bias)


class _ReluLayerNorm(torch.autograd.Function):
    """y = LayerNorm(relu(x)) over the last dim (gcm_relu_layernorm_fwd/bwd); x is saved, the row
    statistics are recomputed in the backward."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = x.contiguous()
        _hip.on_device(x, gamma, beta)
        F = x.shape[-1]
        M = x.numel() // F
        y = torch.empty_like(x)
        _call("gcm_relu_layernorm_fwd", _hip.ptr(x), _hip.ptr(gamma), _hip.ptr(beta), _hip.ptr(y), M, F,
              eps, _hip.stream())
        ctx.save_for_backward(x, gamma)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, g):
        x, gamma = ctx.saved_tensors
        F = x.shape[-1]
        M = x.numel() // F
        g = g.contiguous()
        dx = torch.empty_like(x)
        dgb = torch.empty(2 * F, device=x.device, dtype=_f32)
        lib = _hip.lib()
        ws_bytes = lib.gcm_relu_layernorm_bwd_workspace_bytes(M, F)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        _call("gcm_relu_layernorm_bwd", _hip.ptr(g), _hip.ptr(x), _hip.ptr(gamma), _hip.ptr(dx), _hip.ptr(dgb),
              _hip.ptr(ws), ws_bytes, M, F, ctx.eps, _hip.stream())
        return dx, dgb[:F], dgb[F:], None


def relu_layernorm(x, gamma, beta, eps):
    return _ReluLayerNorm.apply(x, gamma, beta, eps)


def default_edge_network(net):
    """The modules of `net` when it is the reference's default edge network (learned.py:38-51:
    Linear - ReLU - LayerNorm - Linear - ReLU - LayerNorm - Linear, features <= 64, affine norms,
    no hooks), else None: that architecture runs through skinny_linear / relu_layernorm, anything
    else is called as the torch module it is."""
    nn = torch.nn
    kinds = (nn.Linear, nn.ReLU, nn.LayerNorm, nn.Linear, nn.ReLU, nn.LayerNorm, nn.Linear)
    if not isinstance(net, nn.Sequential) or len(net) != 7:
        return None
    mods = list(net)
    if not all(isinstance(m, k) for m, k in zip(mods, kinds)):
        return None
    for m in mods + [net]:
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks:
            return None
    for ln, lin in ((mods[2], mods[0]), (mods[5], mods[3])):
        if (not ln.elementwise_affine or ln.bias is None or tuple(ln.normalized_shape) != (lin.out_features,)
                or lin.out_features > 64):
            return None
    if max(mods[0].in_features, mods[3].in_features, mods[6].in_features) > 64 or mods[6].out_features > 64:
        return None
    return mods


def _mlp_fwd(x2, w0, b0, g0, be0, w1, b1, g1, be1, w2, b2, eps0, eps1):
    """Linear - ReLU - LayerNorm - Linear - ReLU - LayerNorm - Linear on rows x2 [M, I];
    -> (out [M, O], tensors the backward needs)."""
    # three launches of gcm_rows_linear, the first two with the ReLU + LayerNorm epilogue; the
    # pre-activations are saved, the row statistics recomputed in the backward
    p0, h0 = rows_linear(x2, w0, b0, ln=(g0, be0, eps0))
    p1, h1 = rows_linear(h0, w1, b1, ln=(g1, be1, eps1))
    return rows_linear(h1, w2, b2), (x2, p0, h0, p1, h1, w0, g0, w1, g1, w2)


def _mlp_bwd(g2, saved, eps, has_bias, need_x):
    """adjoint of _mlp_fwd for g2 [M, O] -> (g_x2 | None, [dw0, db0, dg0, dbe0, dw1, db1, dg1, dbe1, dw2, db2])"""
    x2, p0, h0, p1, h1, w0, g0, w1, g1, w2 = saved
    lib = _hip.lib()
    st = _hip.stream()
    dev = x2.device
    M = x2.shape[0]

    def wgrad(gy, xin, O, I):
        ws_bytes = lib.gcm_skinny_wgrad_workspace_bytes(M, O, I)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(O * I + O, device=dev, dtype=_f32)
        _call("gcm_skinny_wgrad", _hip.ptr(gy), _hip.ptr(xin), _hip.ptr(out), _hip.ptr(ws), ws_bytes,
              M, O, I, st)
        return out[:O * I].view(O, I), out[O * I:]

    def ln_bwd(gy, pre, gamma, e):
        F = pre.shape[1]
        dx = torch.empty_like(pre)
        dgb = torch.empty(2 * F, device=dev, dtype=_f32)
        ws_bytes = lib.gcm_relu_layernorm_bwd_workspace_bytes(M, F)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _call("gcm_relu_layernorm_bwd", _hip.ptr(gy), _hip.ptr(pre), _hip.ptr(gamma), _hip.ptr(dx),
              _hip.ptr(dgb), _hip.ptr(ws), ws_bytes, M, F, e, st)
        return dx, dgb[:F], dgb[F:]

    dw2, db2 = wgrad(g2, h1, w2.shape[0], w2.shape[1])
    gp1, dg1, dbe1 = ln_bwd(rows_linear(g2, w2, transpose=True), p1, g1, eps[1])
    dw1, db1 = wgrad(gp1, h0, w1.shape[0], w1.shape[1])
    gp0, dg0, dbe0 = ln_bwd(rows_linear(gp1, w1, transpose=True), p0, g0, eps[0])
    dw0, db0 = wgrad(gp0, x2, w0.shape[0], w0.shape[1])
    gx = rows_linear(gp0, w0, transpose=True) if need_x else None
    hb = has_bias
    return gx, [dw0, db0 if hb[0] else None, dg0, dbe0, dw1, db1 if hb[1] else None, dg1, dbe1, dw2,
                db2 if hb[2] else None]


class _EdgeMLP(torch.autograd.Function):
    """The default edge network (learned.py:38-51) as ONE autograd node: Linear - ReLU - LayerNorm -
    Linear - ReLU - LayerNorm - Linear on M candidate rows.  Same kernels and library GEMMs as the
    module-by-module path (skinny_linear / relu_layernorm), chained by hand in both directions:
    five Python-level autograd nodes per step become one."""

    @staticmethod
    def forward(ctx, x, w0, b0, g0, be0, w1, b1, g1, be1, w2, b2, eps0, eps1):
        x2 = x.reshape(-1, x.shape[-1])
        out, saved = _mlp_fwd(x2, w0, b0, g0, be0, w1, b1, g1, be1, w2, b2, eps0, eps1)
        ctx.save_for_backward(*saved)
        ctx.eps = (eps0, eps1)
        ctx.has_bias = (b0 is not None, b1 is not None, b2 is not None)
        ctx.xshape = x.shape
        return out.view(*x.shape[:-1], out.shape[-1])

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        g2 = g.reshape(saved[0].shape[0], -1).contiguous()
        gx, pg = _mlp_bwd(g2, saved, ctx.eps, ctx.has_bias, ctx.needs_input_grad[0])
        return (gx.view(ctx.xshape) if gx is not None else None, *pg, None, None)


class _LearnedEdgeDefault(torch.autograd.Function):
    """Dense LearnedEdge with the default edge network as ONE autograd node (learned.py:53-113):
    candidate pairs, edge network, gumbel noise, gumbel-softmax + STE + adjacency-row write (in
    place on `adj`, which the caller owns).  `noise` None = draw it here with the device RNG the
    way torch.nn.functional.gumbel_softmax does.  `deterministic`: the hard sparsemax of the logits
    instead (learned.py:85-86) - `noise` and `cutoff` are not read, nothing is drawn or allocated for them."""

    @staticmethod
    def forward(ctx, nodes, adj, cur, noise, cutoff, deterministic, w0, b0, g0, be0, w1, b1, g1, be1, w2, b2,
                eps0, eps1):
        nodes = nodes.contiguous()
        _hip.on_device(nodes, adj, cur)
        B, N, F = nodes.shape
        st = _hip.stream()
        pairs = torch.empty(B * N, 2 * F, device=nodes.device, dtype=_f32)
        _call("gcm_learned_pairs_fwd", _hip.ptr(nodes), _hip.ptr(cur), _hip.ptr(pairs), B, N, F, st)
        logits, saved = _mlp_fwd(pairs, w0, b0, g0, be0, w1, b1, g1, be1, w2, b2, eps0, eps1)
        logits = logits.view(B, N)
        soft = torch.empty(B, N, device=adj.device, dtype=_f32)
        if deterministic:
            _call("gcm_learned_sparsemax_fwd", _hip.ptr(logits), _hip.ptr(cur), _hip.ptr(adj), _hip.ptr(soft),
                  B, N, st)
        else:
            if noise is None:
                noise = -torch.empty_like(logits).exponential_().log()
            noise = noise.contiguous()
            _call("gcm_learned_select_fwd", _hip.ptr(logits), _hip.ptr(noise), _hip.ptr(cur), float(cutoff),
                  _hip.ptr(adj), _hip.ptr(soft), B, N, st)
        ctx.mark_dirty(adj)
        ctx.deterministic = bool(deterministic)
        ctx.save_for_backward(soft, cur, *saved)
        ctx.eps = (eps0, eps1)
        ctx.has_bias = (b0 is not None, b1 is not None, b2 is not None)
        ctx.dims = (B, N, F)
        return adj

    @staticmethod
    def backward(ctx, g_adj):
        soft, cur, *saved = ctx.saved_tensors
        B, N, F = ctx.dims
        st = _hip.stream()
        g_adj = g_adj.contiguous()
        g_logits = torch.empty(B * N, 1, device=g_adj.device, dtype=_f32)
        _call("gcm_learned_sparsemax_bwd" if ctx.deterministic else "gcm_learned_select_bwd", _hip.ptr(g_adj),
              _hip.ptr(soft), _hip.ptr(cur), _hip.ptr(g_logits), B, N, st)
        g_pairs, pg = _mlp_bwd(g_logits, saved, ctx.eps, ctx.has_bias, ctx.needs_input_grad[0])
        g_nodes = None
        if g_pairs is not None:
            g_nodes = torch.empty(B, N, F, device=g_adj.device, dtype=_f32)
            _call("gcm_learned_pairs_bwd", _hip.ptr(g_pairs), _hip.ptr(cur), _hip.ptr(g_nodes), B, N, F, st)
        # both straight-through estimators are identities: the incoming adjacency receives g_adj
        # unchanged, also at the rewritten entries (learned.py:108-110 adds adj inside the STE)
        return (g_nodes, g_adj, None, None, None, None, *pg, None, None)


def learned_edge_default(net, nodes, adj, cur, noise, cutoff, deterministic=False):
    """The fused dense LearnedEdge when `net` is the default edge network on device tensors, else None."""
    mods = default_edge_network(net)
    if mods is None or not nodes.is_cuda or nodes.dtype != _f32:
        return None
    l0, _, n0, l1, _, n1, l2 = mods
    if l2.out_features != 1 or l0.in_features != 2 * nodes.shape[2]:
        return None
    return _LearnedEdgeDefault.apply(nodes, adj, cur, noise, cutoff, deterministic, l0.weight, l0.bias, n0.weight,
                                     n0.bias, l1.weight, l1.bias, n1.weight, n1.bias, l2.weight, l2.bias, n0.eps,
                                     n1.eps)


def edge_network_forward(net, x):
    """net(x) for the default architecture on device rows: one autograd node over the row-split
    kernels; anything else is called as the torch module it is."""
    mods = default_edge_network(net)
    if mods is None or not x.is_cuda or x.dtype != _f32 or x.numel() == 0:
        return net(x)
    l0, _, n0, l1, _, n1, l2 = mods
    return _EdgeMLP.apply(x, l0.weight, l0.bias, n0.weight, n0.bias, l1.weight, l1.bias, n1.weight, n1.bias,
                          l2.weight, l2.bias, n0.eps, n1.eps)


# ===========================================================================
# SURVEY 8(f) "next" rows: positional encoding, packed sparse hidden state
# ===========================================================================
class _PosEncAdd(torch.autograd.Function):
    """x[b, n] += pe[n] for n <= num_nodes[b], in place (gcm.py:120-131); backward = identity."""

    @staticmethod
    def forward(ctx, x, pe, num_nodes):
        _hip.on_device(x, pe, num_nodes)
        B, N, F = x.shape
        _call("gcm_posenc_add", _hip.ptr(x), _hip.ptr(pe), _hip.ptr(num_nodes), B, N, F, pe.shape[1],
              pe.shape[0], _hip.stream())
        ctx.mark_dirty(x)
        return x

    @staticmethod
    def backward(ctx, g):
        return g, None, None


class _PosEncCat(torch.autograd.Function):
    """PositionalEncoding(mode="cat") (gcm.py:133-140): rows i <= num_nodes[b] become
    [pe[i, :cat_dim] | reproject(x[b, i])], the rows beyond stay x - gcm_rows_linear writes the
    re-projection straight into the output's columns cat_dim.., one element-wise pass finishes it."""

    @staticmethod
    def forward(ctx, x, weight, bias, pe, num_nodes, cat_dim):
        x = x.contiguous()
        _hip.on_device(x, weight, bias, pe, num_nodes)
        B, N, F = x.shape
        out = torch.empty_like(x)
        rows_linear(x.view(B * N, F), weight, bias, out=out.view(B * N, F)[:, cat_dim:], ldy=F)
        _call("gcm_posenc_cat_finish", _hip.ptr(x), _hip.ptr(pe), pe.stride(0), _hip.ptr(num_nodes), _hip.ptr(out),
              B, N, F, cat_dim, _hip.stream())
        ctx.save_for_backward(x, weight, num_nodes)
        ctx.cat_dim = cat_dim
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, num_nodes = ctx.saved_tensors
        B, N, F = x.shape
        cat = ctx.cat_dim
        g = g.contiguous()
        g_x = torch.empty_like(x)
        g_proj = torch.empty(B * N, F - cat, device=x.device, dtype=_f32)
        _call("gcm_posenc_cat_bwd", _hip.ptr(g), _hip.ptr(num_nodes), _hip.ptr(g_x), _hip.ptr(g_proj), B, N, F, cat,
              _hip.stream())
        if ctx.needs_input_grad[0]:
            g_x = g_x + rows_linear(g_proj, weight, transpose=True).view(B, N, F)
        else:
            g_x = None
        gw = gb = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            O, I = weight.shape
            lib = _hip.lib()
            ws_bytes = lib.gcm_skinny_wgrad_workspace_bytes(B * N, O, I)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=g.device)
            out = torch.empty(O * I + O, device=g.device, dtype=_f32)
            _call("gcm_skinny_wgrad", _hip.ptr(g_proj), _hip.ptr(x), _hip.ptr(out), _hip.ptr(ws), ws_bytes,
                  B * N, O, I, _hip.stream())
            gw = out[:O * I].view(O, I)
            gb = out[O * I:] if ctx.has_bias else None
        return g_x, gw, gb, None, None, None


def posenc_cat(x, weight, bias, pe, num_nodes, cat_dim):
    return _PosEncCat.apply(x, weight, bias, pe, num_nodes, cat_dim)


def posenc_add_(x, pe, num_nodes):
    return _PosEncAdd.apply(x, pe, num_nodes)


def pack_hidden(coo, values, B, max_edges, edge_fill, weight_fill):
    """-> dense_edges [B,2,max_edges] i64, dense_weights [B,1,max_edges] f32 (util.py:323-351).
    One host readback (the per-graph counts, for the reference's assertion)."""
    coo, values = coo.contiguous(), values.contiguous()
    _hip.on_device(coo, values)
    E = coo.shape[1]
    dev = coo.device
    dense_edges = torch.full((B, 2, max_edges), edge_fill, dtype=_i64, device=dev)
    dense_weights = torch.full((B, 1, max_edges), weight_fill, dtype=_f32, device=dev)
    batch_ptr = ptr_from_sorted(coo[0], B)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    _call("gcm_pack_hidden", _hip.ptr(coo), _hip.ptr(values), _hip.ptr(batch_ptr),
          _hip.ptr(dense_edges), _hip.ptr(dense_weights), _hip.ptr(flags), E, B, max_edges,
          _hip.stream())
    counts = (batch_ptr[1:] - batch_ptr[:-1]).tolist()
    for n in counts:
        assert n < max_edges, f"Cannot pack {n} edges into {max_edges}, increase max edges"
    return dense_edges, dense_weights


# ===========================================================================
# sparse LearnedEdge (sparse_edge_selectors/learned.py:90-160)
# ===========================================================================
class CausalEdges:
    """Closed-form causal candidate edges of a batch (util.get_causal_edges util.py:242-282):
    indices [3, E] (batch, sink, source) in coalesced order + the sink-row segments."""

    def __init__(self, T, taus, window):
        _hip.on_device(T, taus)
        B = T.numel()
        dev = T.device
        self.T, self.taus, self.B = T, taus, B
        self.window = -1 if window is None else int(window)
        offs = torch.empty(2, B + 1, dtype=_i64, device=dev)
        self.edge_off, self.seg_off = offs[0], offs[1]
        _call("gcm_causal_count", _hip.ptr(T), _hip.ptr(taus), self.window, _hip.ptr(self.edge_off),
              _hip.ptr(self.seg_off), B, _hip.stream())
        self.E, self.S = (int(v) for v in offs[:, B].tolist())           # one readback
        self.indices = torch.empty(3, self.E, dtype=_i64, device=dev)
        self.seg_ptr = torch.empty(self.S + 1, dtype=_i64, device=dev)
        _call("gcm_causal_fill", _hip.ptr(T), _hip.ptr(taus), self.window, _hip.ptr(self.edge_off),
              _hip.ptr(self.seg_off), _hip.ptr(self.indices), _hip.ptr(self.seg_ptr), self.E,
              self.S, B, _hip.stream())


class _CausalPairs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, nodes, edges):
        nodes = nodes.contiguous()
        B, N, F = nodes.shape
        pairs = torch.empty(edges.E, 2 * F, device=nodes.device, dtype=_f32)
        _call("gcm_causal_pairs_fwd", _hip.ptr(nodes), _hip.ptr(edges.indices), _hip.ptr(pairs),
              edges.E, B, N, F, _hip.stream())
        ctx.edges, ctx.dims = edges, (B, N, F)
        return pairs

    @staticmethod
    def backward(ctx, g_pairs):
        e = ctx.edges
        B, N, F = ctx.dims
        g_pairs = g_pairs.contiguous()
        g_nodes = torch.empty(B, N, F, device=g_pairs.device, dtype=_f32)
        _call("gcm_causal_pairs_bwd", _hip.ptr(g_pairs), _hip.ptr(e.T), _hip.ptr(e.taus), e.window,
              _hip.ptr(e.edge_off), _hip.ptr(g_nodes), e.E, B, N, F, _hip.stream())
        return g_nodes, None


def causal_pairs(nodes, edges):
    return _CausalPairs.apply(nodes, edges)


class _SegmentSoftmax(torch.autograd.Function):
    """soft = softmax over each sink row of (logits + noise) / tau  (util.py:89-113, hard=False)."""

    @staticmethod
    def forward(ctx, logits, tau, noise, edges):
        logits, noise = logits.contiguous(), noise.contiguous()
        tau_d = tau.detach().to(device=logits.device, dtype=_f32).contiguous()
        soft = torch.empty_like(logits)
        _call("gcm_segment_softmax_fwd", _hip.ptr(logits), _hip.ptr(noise), _hip.ptr(tau_d),
              _hip.ptr(edges.seg_ptr), _hip.ptr(soft), edges.S, edges.E, _hip.stream())
        ctx.save_for_backward(soft, logits, noise, tau_d)
        ctx.edges, ctx.tau_shape = edges, tau.shape
        return soft

    @staticmethod
    def backward(ctx, g_soft):
        soft, logits, noise, tau_d = ctx.saved_tensors
        e = ctx.edges
        g_soft = g_soft.contiguous()
        g_logits = torch.empty_like(logits)
        g_tau_rows = torch.zeros(max(e.S, 1), device=logits.device, dtype=_f32)
        _call("gcm_segment_softmax_bwd", _hip.ptr(g_soft), _hip.ptr(soft), _hip.ptr(logits),
              _hip.ptr(noise), _hip.ptr(tau_d), _hip.ptr(e.seg_ptr), _hip.ptr(g_logits),
              _hip.ptr(g_tau_rows), e.S, e.E, _hip.stream())
        g_tau = g_tau_rows.sum().reshape(ctx.tau_shape) if ctx.needs_input_grad[1] else None
        return g_logits, g_tau, None, None


def segment_softmax(logits, tau, noise, edges):
    return _SegmentSoftmax.apply(logits, tau, noise, edges)


# ---------------------------------------------------------------------------
# sparse spatial selectors (src/gcm/sparse_edge_selectors/spatial.py)
# ---------------------------------------------------------------------------
def spatial_edges(nodes, T, taus, cols, mode, radius=0.0, k=0):
    """COO indices [3, E] (batch, sink, source) of SpatialRadiusEdge / SpatialKNNEdge in coalesced order, and the
    per-graph edge offsets [B+1].  cols: host list of position columns; mode: _hip.SPATIAL_*.  One readback (E and
    max(T + tau), the overflow check)."""
    if nodes.dtype != _f32:
        raise TypeError(f"spatial selector: the kernels read float32 node features, got {nodes.dtype}")
    nodes, T, taus = nodes.detach().contiguous(), T.to(_i64).contiguous(), taus.to(_i64).contiguous()
    _hip.on_device(nodes, T, taus)
    B, N, F = nodes.shape
    P = len(cols)
    if not _hip.lib().gcm_spatial_supported(mode, B, N, F, P):
        raise NotImplementedError(
            f"spatial selector: {P} position columns at graph size {N} are beyond the kernels' limits "
            f"(P <= {_hip.SPATIAL_MAX_COLS}, (P + 1) * N * 4 bytes of LDS <= 160 KB, N <= 4096 for kNN)")
    dev = nodes.device
    arr = (ctypes.c_int32 * max(P, 1))(*cols)
    row_off = torch.empty(B, N, dtype=torch.int32, device=dev)
    kth = torch.empty(B, N, dtype=_i64, device=dev) if mode == _hip.SPATIAL_KNN else None
    edge_off = torch.empty(B + 2, dtype=_i64, device=dev)
    _call("gcm_spatial_count", _hip.ptr(nodes), _hip.ptr(T), _hip.ptr(taus), ctypes.addressof(arr), P, mode,
          float(radius), int(k), _hip.ptr(row_off), _hip.ptr(kth), _hip.ptr(edge_off), B, N, F, _hip.stream())
    E, max_total = (int(v) for v in edge_off[B:].tolist())                # the one readback
    if max_total > N:
        raise IndexError(f"spatial selector: a graph holds {max_total} nodes, more than the node matrix's {N}")
    idx = torch.empty(3, E, dtype=_i64, device=dev)
    _call("gcm_spatial_fill", _hip.ptr(nodes), _hip.ptr(T), _hip.ptr(taus), ctypes.addressof(arr), P, mode,
          float(radius), _hip.ptr(row_off), _hip.ptr(kth), _hip.ptr(edge_off), _hip.ptr(idx) if E else None, E,
          B, N, F, _hip.stream())
    return idx, edge_off[:B + 1]
