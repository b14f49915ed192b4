"""DenseGCM - the dense graph memory step (reference: src/gcm/gcm.py:151-355).

Same constructor, call surface and hidden-state layout as the reference:

    belief, m_t = DenseGCM(gnn, edge_selectors=...)(obs, m_t)
    m_t = (nodes f32[B,N,F], adj f32[B,N,N], weights f32[B,N,N] | f32[0], num_nodes i64[B])

What differs is where the work runs: the node insert + overflow roll, the edge
selectors, DenseGraphConv and the belief-row extract are gfx950 kernels
(include/gcm_hip.h) launched on the current stream, and the step never blocks
on the device: the reference's two host syncs per step (gcm.py:263, 316-318)
are replaced by a device-side flag word that is polled without blocking
(`finite_check="deferred"`, default), checked every step (`"sync"`, the
reference's exact raise point) or not at all (`"off"`).
"""
import math
import os
from typing import Tuple, Union

import weakref

import torch

from . import _hip, _ops


_DTYPES = (torch.float32, torch.float32, torch.float32, torch.float32, torch.int64, 1)


class SparseToDense(torch.nn.Module):
    """Edge list back to a padded batch (reference: src/gcm/gcm.py:10-21; PyG's to_dense_batch / to_dense_adj with
    max_num_nodes=N).

        x [B,N,F], adj [B,N,N] float32 = SparseToDense()(x_sp [M,F], edge_index [2,E], batch_idx [M], B, N,
                                                         edge_weight=None)

    batch_idx is non-decreasing.  Node m lands at (batch_idx[m], m - first node of its graph); positions >= N are
    dropped and rows no node fills are 0.  adj[b, source, sink] += 1 per edge - += edge_weight[e] when given - so
    duplicate edges add; an edge with an end beyond N, or with its ends in two graphs, is dropped.  On a HIP device
    both are kernels (csrc/dense_sparse.hip): every sink sums its edges in the order of its CSR entries - the index
    attached to edge_index as `gcm_graph` when there is one, else one built here - so results are bitwise
    reproducible, without float atomics.  Gradients reach x_sp and edge_weight.

    Two deliberate differences from the reference: the batch size is the argument B (the reference reads
    batch_idx.max() + 1 back to the host), and adj is the whole [B,N,N] (the reference returns to_dense_adj(...)[0],
    the first graph's [N,N] only, which its test cannot tell apart because all its graphs are equal)."""

    def forward(self, x, edge_index, batch_idx, B, N, edge_weight=None):
        B, N = int(B), int(N)
        if x.dim() != 2 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise ValueError("SparseToDense takes x [M,F] and edge_index [2,E]")
        if edge_weight is not None and edge_weight.numel() != edge_index.shape[1]:
            raise ValueError("edge_weight must hold one value per edge")
        M, F = x.shape
        if not x.is_cuda or F == 0:
            return self._torch_forward(x, edge_index, batch_idx, B, N, edge_weight)
        with torch.cuda.device(x.device):
            graph = getattr(edge_index, "gcm_graph", None)
            if graph is None or graph.M != M or graph.mask is not None:
                graph = _ops.GraphIndex.from_edge_index(edge_index, M)
            if edge_weight is not None:
                edge_weight = edge_weight.to(torch.float32).view(-1)
            return _ops.sparse_to_dense(x.to(torch.float32), graph, batch_idx.to(torch.int64), B, N, edge_weight)

    @staticmethod
    def _torch_forward(x, edge_index, batch_idx, B, N, edge_weight):
        """The same function in torch ops (CPU tensors): index_put with accumulate, which a CPU runs in list order."""
        M = x.shape[0]
        batch_idx = batch_idx.to(torch.int64)
        first = torch.searchsorted(batch_idx, torch.arange(B, device=x.device))
        inside = (batch_idx >= 0) & (batch_idx < B)
        graph = batch_idx.clamp(0, max(B - 1, 0))
        pos = torch.arange(M, device=x.device) - first[graph]
        keep = inside & (pos >= 0) & (pos < N)
        dense = x.new_zeros(B, N, x.shape[1]).index_put((graph[keep], pos[keep]), x[keep])
        src, dst = edge_index[0], edge_index[1]
        ends = (src >= 0) & (src < M) & (dst >= 0) & (dst < M)
        src, dst = src.clamp(0, max(M - 1, 0)), dst.clamp(0, max(M - 1, 0))
        ok = ends & keep[src] & keep[dst] & (graph[src] == graph[dst])
        w = torch.ones(src.numel(), device=x.device) if edge_weight is None else edge_weight.to(torch.float32).view(-1)
        adj = torch.zeros(B, N, N, device=x.device).index_put((graph[src][ok], pos[src][ok], pos[dst][ok]), w[ok],
                                                              accumulate=True)
        return dense, adj


class DenseToSparse(torch.nn.Module):
    """Padded batch to an edge list (reference: src/gcm/gcm.py:24-53), so that sparse `edge_index` layers - the fused
    ones of gcm.nn and any gcm.nn.MessagePassing subclass - run inside DenseGCM behind its selectors.

        x_sp [B*N,F], edge_index [2,E] int64, batch_idx [B*N] int64 = DenseToSparse()(x [B,N,F], adj [B,N,N])
        ..., edge_weight [E] float32                                = DenseToSparse(edge_values=True)(x, adj)

    The edges are the entries adj[b,r,c] > 0 (strictly: a negative entry is no edge), in (b, r, c) order, which is
    torch.nonzero's.  x_sp is a view of x; mask must be None (the reference raises NotImplementedError too).

    ORIENTATION.  The reference emits (b*N + r, b*N + c): the ROW is the source.  The dense layers, and every
    selector of DenseGCM, read adj[b,i,j] as "i aggregates from j": the row is the sink.  Through the reference's
    bridge a sparse layer therefore works on the TRANSPOSED graph.  transpose=False (default) reproduces the
    reference; transpose=True emits (b*N + c, b*N + r) in the same list order, and a sparse layer then aggregates
    exactly as its dense twin does on the same adj.  Use transpose=True behind DenseGCM's selectors.

    edge_values=True also returns the values adj[b,r,c] of the edges, differentiable in adj (the gradient is scattered
    into a zero [B,N,N]): what the reference's docstring promises and its code does not do.

    On a HIP device with N <= 512 (GCM_BRIDGE_MAX_N: one thread per column of a graph) this is three kernels of
    csrc/dense_sparse.hip and ONE host read, of E.  float32 and int64 adj are read as they are, other dtypes are
    converted first.  The GraphIndex of the list (M = B*N; CSR by sink, the CSC view, batches) is attached as
    `edge_index.gcm_graph` - the arrays GraphIndex.from_edge_index and its csc() would compute, built by counting
    instead of two device-wide sorts - so the layers behind the bridge index nothing.  Inside a stream capture the host
    read is impossible and the call raises RuntimeError.  CPU tensors and larger N take torch ops (nonzero); on a
    device the index is then built by from_edge_index."""

    def __init__(self, transpose=False, edge_values=False):
        super().__init__()
        self.transpose, self.edge_values = bool(transpose), bool(edge_values)

    def extra_repr(self):
        return f"transpose={self.transpose}, edge_values={self.edge_values}"

    def forward(self, x, adj, mask=None):
        assert x.dim() == adj.dim() == 3
        if mask is not None:
            raise NotImplementedError("DenseToSparse: mask is not supported (nor is it in the reference)")
        B, N = x.shape[0], x.shape[1]
        assert adj.shape == (B, N, N), "adj must be [B,N,N] over the nodes of x"
        x_sp = x.view(B * N, x.shape[-1]) if x.is_contiguous() else x.reshape(B * N, x.shape[-1])
        if adj.is_cuda and 1 <= N <= _ops.BRIDGE_MAX_N and B >= 1:
            if adj.dtype not in (torch.float32, torch.int64):
                adj = adj.to(torch.float32)     # (autograd's own op: a gradient still reaches the caller's adj)
            with torch.cuda.device(adj.device):
                if self.edge_values:
                    edge_index, graph, values = _ops.dense_to_sparse_values(adj, self.transpose)
                else:
                    edge_index, graph, values = _ops.dense_to_sparse(adj, self.transpose, False)
                batch_idx = torch.arange(B * N, device=adj.device) // N
        else:
            b, r, c = torch.nonzero(adj > 0).t()
            rows, cols = b * N + r, b * N + c
            edge_index = torch.stack([cols, rows] if self.transpose else [rows, cols], dim=0).long()
            values = adj[b, r, c].to(torch.float32) if self.edge_values else None
            batch_idx = torch.arange(B, device=x.device).view(-1, 1).repeat(1, N).view(-1)
            graph = _ops.GraphIndex.from_edge_index(edge_index, B * N) if adj.is_cuda else None
        if graph is not None:
            edge_index.gcm_graph = graph
        if self.edge_values:
            return x_sp, edge_index, batch_idx, values
        return x_sp, edge_index, batch_idx


class PositionalEncoding(torch.nn.Module):
    """Embed a sin/cos positional encoding into the graph without touching future nodes
    (node index > num_nodes).  Reference: src/gcm/gcm.py:92-143 (same constructor, same lazily
    built `pe` buffer and `reproject` layer).  mode="add" is one in-place kernel
    (gcm_posenc_add); mode="cat" re-projects the features with gcm_rows_linear straight into the
    output's last columns and writes the first cat_dim columns from the table (gcm_posenc_cat_finish)."""

    def __init__(self, max_len: int = 5000, mode="add", cat_dim: int = 8):
        super().__init__()
        self.max_len = max_len
        self.mode = mode
        self.cat_dim = cat_dim
        assert mode in ["add", "cat"]

    def run_once(self, x: torch.Tensor) -> None:
        d_model = math.ceil(x.shape[-1] / 2) * 2          # gcm.py:103-112, table built on the host
        position = torch.arange(self.max_len).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(self.max_len, d_model)
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe", pe.to(x.device))
        if self.mode == "cat":
            self.reproject = torch.nn.Linear(x.shape[-1], x.shape[-1] - self.cat_dim,
                                             device=x.device)

    def forward(self, x: torch.Tensor, num_nodes: torch.Tensor) -> torch.Tensor:
        """x [B, N, F], num_nodes [B]: rows 0..num_nodes[b] (inclusive) are encoded."""
        if not hasattr(self, "pe"):
            self.run_once(x)
        if self.mode == "add":
            if x.is_leaf and x.requires_grad:
                x = x.clone()
            return _ops.posenc_add_(x.contiguous() if not x.is_contiguous() else x, self.pe,
                                    num_nodes)
        N, F = x.shape[1], x.shape[2]
        if x.is_cuda and x.dtype == torch.float32 and F <= 64 and 0 < self.cat_dim < F and x.dim() == 3 \
                and self.pe.shape[0] >= N:
            return _ops.posenc_cat(x, self.reproject.weight, self.reproject.bias, self.pe, num_nodes, self.cat_dim)
        # (wider features than the row kernel takes: torch ops)
        live = (torch.arange(N, device=x.device)[None, :] <= num_nodes[:, None]).unsqueeze(-1)
        pe = self.pe[:N, : self.cat_dim].unsqueeze(0).expand(x.shape[0], -1, -1)
        enc = torch.cat((pe, self.reproject(x)), dim=-1)
        return torch.where(live, enc, x)


class DenseGCM(torch.nn.Module):
    """Graph Associative Memory (dense adjacency)."""

    did_warn = False

    def __init__(
        self,
        gnn: torch.nn.Module,
        preprocessor: torch.nn.Module = None,
        edge_selectors: torch.nn.Module = None,
        aux_edge_selectors: torch.nn.Module = None,
        graph_size: int = 128,
        pooled: bool = False,
        positional_encoder: torch.nn.Module = None,
        edge_weights: bool = False,
        finite_check: str = "deferred",
        poll_interval: int = 16,
        mutate_num_nodes_on_overflow: bool = False,
        fused: bool = True,
        donate_state: bool = False,
    ):
        super().__init__()
        assert finite_check in ("deferred", "sync", "off")
        self.preprocessor = preprocessor
        self.gnn = gnn
        self.graph_size = graph_size
        self.edge_selectors = edge_selectors
        self.aux_edge_selectors = aux_edge_selectors
        self.pooled = pooled
        self.edge_weights = edge_weights
        self.positional_encoder = positional_encoder
        self.finite_check = finite_check
        self.poll_interval = poll_interval
        # gcm.py:354 decrements the CALLER's num_nodes in place when a graph wraps;
        # off by default (the returned values are identical either way)
        self.mutate_num_nodes_on_overflow = mutate_num_nodes_on_overflow
        # fused=True: when the GNN is the canonical two DenseGraphConv(+Tanh/ReLU) stack and the
        # selectors are native non-differentiable ones, a step runs as state-advance + selector
        # kernels + ONE fused GNN kernel under ONE autograd node (csrc/fused.hip)
        self.fused = fused
        # donate_state=True: the caller hands over the hidden state it passes in; the step advances
        # `nodes`, `adj` and `num_nodes` IN PLACE and returns the same tensors (no per-step clone of
        # the state, gcm.py:262,278,286).  Results are identical; a caller that keeps older hidden
        # states around (they would all alias the newest one) must leave this off.  Takes effect on
        # the live-row path (index-writing selectors, canonical GNN, no gradient w.r.t. obs / nodes);
        # every other case falls back to functional semantics.
        self.donate_state = donate_state
        self._plan_cache = None
        self._fold = None     # set by _structure(): what the live-row step absorbs besides the GNN
        self._noise_pool = None   # [exponential draws [noise_pool_steps, B, N], next index, drawn under capture] of the fused LearnedEdge step
        self._token = object()   # identifies hidden states produced by this module (_gcm_link)
        self._cfg_cache = {}
        self._cfg_last = None
        self._packed_cache = None
        self._flags = {}      # device -> uint32[1] flag word written by the kernels
        self._pending = []    # [(pinned host copy, event)] of flag words in flight
        self._pinned_pool = []
        self._ctr = [0]       # steps since the last poll (a list: nn.Module.__setattr__ is slow)
        self._fast = None     # (RowsFast, flag word) of the last live-row step: what __call__ tries first
        self._learned_chain = None   # (packed vector, LearnedChain, grad mode): the fused LearnedEdge steps' one autograd node
        # fused LearnedEdge steps: how many steps' gumbel draws one RNG launch makes (B x N x 4 bytes each)
        self.noise_pool_steps = 64
        # False: no cached steps (the first N steps of a LearnedEdge rollout from empty graphs on a donated state as
        # ONE launch each, the GNN behind the selection on per-chain caches) - A/B tests
        self.learned_cached_steps = True
        # ... a continuing LearnedEdge chain's steps run from DenseGCM.__call__ straight into the C++ host path
        # (LearnedFast in csrc/torch_ext/step_ext.cpp); False: every step through forward() - A/B tests
        self.learned_fast_path = True
        # False: no cached live-row steps (csrc/rows_cached.hip: the first N steps of a rollout from empty graphs on a
        # donated state, forward-only TemporalBackedge selectors: row cur alone over per-chain caches) - A/B
        self.rows_cached_steps = True
        # False: chains whose selectors also write COLUMN cur of the adjacency (DenseEdge; "backward" / "both" hops) stay
        # on the general live-row kernel instead of the column-write cached step (csrc/rows_colcache.hip: rank-1
        # updates of the chain's layer-1 aggregate, one matrix-core product of the live rows) - A/B tests
        self.rows_col_cache = os.environ.get("GCM_COL_CACHE", "1") == "1"
        # False: a cached EuclideanEdge chain as TWO launches per step (distance kernel, then the cached step) instead
        # of one (csrc/distance.hip: k_euclid_mfma2<.., TAIL>) - A/B tests; read when a chain is armed
        self.rows_one_launch_distance = True
        # True: the cached temporal-hops step (k_step_rows_cached_img4) reads the weight image in its interleaved form -
        # image2[layer][k][lane][rel | root], one 8-byte load per (W_rel[h][k], W_root[h][k]) pair straight into the
        # adjacent registers v_pk_fma_f32 wants: 64 load instructions instead of 128 and none of the 128 register moves
        # that paired the operands.  cfg2 on the same box, graph replay: 58.2 M against 55.2 M for the plain lane-major
        # image (False; env GCM_IMG_V4=0 for the A/B).  (Round 5's first use of this slot - four k per lane as 16-byte
        # loads - had measured slower: 4.85 against 4.63 us.)
        self.rows_weight_image_v4 = os.environ.get("GCM_IMG_V4", "1") == "1"
        # True (round 6): the cached temporal-hops step at F = H1 = 32 runs with a SECOND wave per graph that writes what
        # follows from `cur` alone (the observation into the node matrix / cache, the adjacency row, the count, the record's
        # live list) while wave 0 computes - ~120 instructions off a one-wave instruction stream.  False (env
        # GCM_ONE_WAVE=1): the one-wave kernel (A/B)
        self.rows_bookkeeping_wave = os.environ.get("GCM_ONE_WAVE", "0") != "1"
        # True: that two-wave step at tanh / tanh with at most four forward hops runs in its lean form
        # (csrc/rows_cached_lean.hip: the step resolved on the host, the arguments its loads need preloaded into SGPRs,
        # layer 2's weights in flight under layer 1).  False (env GCM_LEAN_STEP=0): k_step_rows_cached_img4b (A/B)
        self.rows_lean_step = os.environ.get("GCM_LEAN_STEP", "1") == "1"
        # True: the parameter backward of a chain of cached steps with forward temporal hops and host-known rows - the
        # donated per-step loop from hidden = None while it stays below N steps, and rollout() from empty graphs at
        # T <= N - runs in its GEMM form (csrc/rows_bptt_hops.hip: four small matrix products and one gather per graph,
        # the records' live lists not read).  False (env GCM_BPTT_HOPS=0): k_bptt_cached_graph, which every other chain
        # keeps (A/B); read when a chain is armed / a rollout starts
        self.rows_hops_bptt = os.environ.get("GCM_BPTT_HOPS", "1") == "1"
        # True: that GEMM form sums the D2 rows of a row's hop sources BEFORE the layer-2 product and multiplies once
        # (k_bptt_hops_graph_fold: no U image in LDS, the product's accumulator feeds dW1 from the registers).  False
        # (env GCM_BPTT_HOPS_FOLD=0): the kernel before, U through LDS and a gather (A/B); the gradients of the two
        # differ by re-ordered float32 sums
        self.rows_hops_fold = os.environ.get("GCM_BPTT_HOPS_FOLD", "1") == "1"
        # True: the head of a chain - the packed parameter vector, the cached step's weight image and, from hidden = None,
        # the zero state - is ONE launch (csrc/head_fused.hip) instead of a fill, a cat and the image kernel one behind the
        # other in front of step 0.  Taken when the six GNN tensors (and the edge network's) are all present, contiguous
        # fp32 on the current HIP device, and nothing is folded into the vector.  False (env GCM_FUSED_HEAD=0): the three
        # launches (A/B); the same bits either way
        self.rows_fused_head = os.environ.get("GCM_FUSED_HEAD", "1") == "1"
        # True: while a HIP graph is being captured, lean cached steps that follow one another directly - the stream's only
        # pending dependency is the node the previous step became, and the step continues that chain - are appended to
        # that node (csrc/rows_cached_run.hip: k_step_rows_cached_img4_lean_run makes them back to back in one launch)
        # instead of becoming ~1.6 us graph nodes of their own.  Eager steps are untouched.  False (env
        # GCM_MERGE_CAPTURED=0): one node per step (A/B); the same bits either way.  Read when a chain is armed
        self.rows_merge_captured = os.environ.get("GCM_MERGE_CAPTURED", "1") == "1"
        self.rows_merge_cap = None   # tests: steps per merged node (None: the library's cap)
        # True: in such a capture the head launch of forward(x, None) (rows_fused_head) that sits directly in front of
        # step 0 is absorbed into the merged node: the node is added on the head's dependencies, runs the kernel's
        # fresh-state form - which writes the packed vector, the weight image and the whole state itself - and the head's
        # node is destroyed ("the head absorbed"): one dependent launch less per replay.  False (env
        # GCM_ABSORB_HEAD=0): the head stays a node (A/B); the same bits either way.  Read when a chain is armed
        self.rows_absorb_head = os.environ.get("GCM_ABSORB_HEAD", "1") == "1"
        # True: the merged node runs the two layers of its steps on the fp32 matrix cores - one accumulator of
        # v_mfma_f32_16x16x4_f32 per chain of the per-step kernel's product, a wave per sixteen steps ("the
        # layers on the matrix cores").  False (env GCM_RUN_MFMA=0): the VALU form of the same kernel (A/B); the same
        # bits either way.  Read when a chain is armed
        self.rows_run_mfma = os.environ.get("GCM_RUN_MFMA", "1") == "1"
        self._head_ready = None   # (cfg, grad mode) of the packed vector forward(x, None) has just built with the state
        # False: rollout() from empty graphs with forward temporal hops runs the persistent per-graph kernel of round 1
        # instead of the two-launch time-parallel forward (csrc/rollout_tp.hip) - A/B tests
        self.rollout_time_parallel = True
        # Steps whose observations / nodes need a gradient run on the live-row kernels too.  True: the whole
        # chain's dL/dx in ONE launch by the chain's single autograd node (hardware float atomics: the order of
        # summation, i.e. the last bits, is not fixed; a policy that feeds belief t-1 into observation t switches
        # to "steps" by itself); "steps": one light node and launch per step, ordered sums (bit-reproducible);
        # False: the round-1 fused kernels (one kernel per step and direction, full state saved) - A/B tests
        self.rows_dx = True

    # -- state ---------------------------------------------------------------
    def get_initial_hidden_state(self, x):
        """gcm.py:194-211 - zero (nodes, adj, weights, num_nodes) for a dummy x [B, feats]."""
        assert x.dim() == 2
        B, feats = x.shape
        edges = torch.zeros(B, self.graph_size, self.graph_size, device=x.device)
        nodes = torch.zeros(B, self.graph_size, feats, device=x.device)
        if self.edge_weights:
            weights = torch.zeros(B, self.graph_size, self.graph_size, device=x.device)
        else:
            weights = torch.zeros(0, device=x.device)
        num_nodes = torch.zeros(B, dtype=torch.long, device=x.device)
        return nodes, edges, weights, num_nodes

    def _fresh_state(self, x):
        """The zero state forward(x, None) starts from, as ONE allocation and ONE fill launch: nodes | adj | num_nodes are
        carved from it as independent tensors (own version counters, no view relation - what the C++ host path does for
        the functional state it returns), 256-byte aligned.  get_initial_hidden_state() itself keeps returning separately
        allocated tensors.  Three launches less per rollout from hidden = None (cfg2: 8 us of 457)."""
        if not x.is_cuda or x.dim() != 2 or x.dtype != torch.float32 or self.edge_weights:
            return self.get_initial_hidden_state(x)
        B, feats = x.shape
        N = self.graph_size
        pad = lambda n: (n + 63) & ~63
        n_nodes, n_adj = pad(B * N * feats), pad(B * N * N)
        flat = torch.zeros(n_nodes + n_adj + 2 * B, device=x.device)
        st = flat.untyped_storage()
        nodes = torch.empty(0, device=x.device).set_(st, 0, (B, N, feats))
        edges = torch.empty(0, device=x.device).set_(st, n_nodes, (B, N, N))
        num_nodes = torch.empty(0, dtype=torch.long, device=x.device).set_(st, (n_nodes + n_adj) // 2, (B,))
        return nodes, edges, torch.zeros(0, device=x.device), num_nodes

    def rows_steps(self):
        """Number of steps this module has run on the live-row kernels (csrc/rows_step.hip) so far."""
        n = 0
        for cfg in self._cfg_cache.values():
            if cfg is not False and cfg._rows_fast is not None:
                n += cfg._rows_fast.steps()
        return n

    def merge_stats(self, head=False, form=False):
        """What became of this module's cached steps in the stream capture seen last: {"nodes": graph nodes they were
        launched as, "merged_steps": steps appended to an existing node instead (rows_merge_captured)}.  Both 0 after
        an eager step.  head=True: also "head_absorbed", the head launches of forward(x, None) whose node a merged node
        took the place of (rows_absorb_head).  form=True: also "run_mfma", whether the merged nodes run their layers on
        the matrix cores (rows_run_mfma, as the chains armed last took it)."""
        nodes = merged = absorbed = 0
        mfma = bool(self.rows_run_mfma)
        for cfg in self._cfg_cache.values():
            if cfg is not False and cfg._rows_fast is not None:
                a, b = cfg._rows_fast.merge_stats()
                nodes, merged = nodes + a, merged + b
                absorbed += cfg._rows_fast.head_absorbed()
                mfma = mfma and bool(cfg._rows_fast.run_mfma())
        out = {"nodes": nodes, "merged_steps": merged}
        if head:
            out["head_absorbed"] = absorbed
        if form:
            out["run_mfma"] = mfma
        return out

    def learned_fast_steps(self):
        """Number of LearnedEdge steps that went from __call__ straight into the C++ host path (LearnedFast)."""
        n = 0
        for cfg in self._cfg_cache.values():
            if cfg is not False and cfg._learned_fast is not None:
                n += cfg._learned_fast.steps()
        return n

    def learned_steady_steps_taken(self):
        """Steps of the current LearnedEdge chain that ran as the one-launch steady-state step (gcm_learned_step_steady:
        past graph_size steps of a chain from empty graphs on a donated state)."""
        lc = self._learned_chain
        return int(lc[1].steady_steps()) if lc is not None else 0

    def rows_cached_steps_taken(self):
        """... of which cached steps (csrc/rows_cached.hip) in the chains armed last."""
        n = 0
        for cfg in self._cfg_cache.values():
            if cfg is not False and cfg._rows_fast is not None:
                n += cfg._rows_fast.cached_steps()
        return n

    def rows_col_steps_taken(self):
        """... of which column-write cached steps (gcm_dense_rows_step_colcache: DenseEdge / backward hops)."""
        n = 0
        for cfg in self._cfg_cache.values():
            if cfg is not False and cfg._rows_fast is not None:
                n += cfg._rows_fast.col_steps()
        return n

    def rows_rolled_steps_taken(self):
        """... of which steady-state ones (gcm_dense_rows_step_cached_roll: past N steps, every step drops the oldest node)."""
        n = 0
        for cfg in self._cfg_cache.values():
            if cfg is not False and cfg._rows_fast is not None:
                n += cfg._rows_fast.rolled_steps()
        return n

    def rows_cached_launches_per_step(self, B):
        """Kernel launches one cached step of this module's last configuration makes at batch size B (0: no cached
        form; 1: forward temporal hops, or EuclideanEdge alone as the one-launch form; 2: distance kernel + step) -
        gcm_dense_rows_cached_launches, a pure function of the configuration."""
        cfg = self._cfg_last[3] if self._cfg_last else None
        if cfg is None or not cfg.cpp_handle():
            return 0
        return cfg._cpp.cached_launches(B)

    def _flag_users(self):
        users = self.__dict__.get("_flag_user_list")
        if users is None:
            users = [m for sel in (self.edge_selectors, self.aux_edge_selectors) if sel is not None
                     for m in sel.modules() if hasattr(m, "_gcm_flags")]
            self.__dict__["_flag_user_list"] = users
        return users

    # -- device flag word ------------------------------------------------------
    def _flag_word(self, device):
        f = self._flags.get(device)
        if f is None:
            f = torch.zeros(1, dtype=torch.int32, device=device)
            self._flags[device] = f
        return f

    def _raise_for(self, bits):
        if bits & _hip.FLAG_BAD_COUNT:
            raise AssertionError("num_nodes outside [0, graph_size]")
        if bits & _hip.FLAG_WRAPPED and not DenseGCM.did_warn:
            print("Overflow detected, wrapping around. Will not warn again")
            DenseGCM.did_warn = True
        if bits & _hip.FLAG_WINDOW:
            from .edge_selectors.temporal import WINDOW_ERROR
            raise RuntimeError(WINDOW_ERROR.format("see TemporalBackedge.learning_window"))
        if bits & _hip.FLAG_NONFINITE:
            raise AssertionError("Got NaN in returned memory, try using tanh activation")

    def check_flags(self, block=True):
        """Surface anything the kernels flagged so far.  block=False only looks at
        flag copies that have already landed on the host."""
        if block:
            bits = 0
            for host, ev in self._pending:     # copies in flight carry bits the device word
                ev.synchronize()               # no longer has (it was zeroed behind each copy)
                bits |= int(host.item())
            self._pending.clear()
            for dev, f in self._flags.items():
                b = int(f.item())
                if b:
                    f.zero_()
                bits |= b
            self._raise_for(bits)
            return
        while self._pending and self._pending[0][1].query():
            host, ev = self._pending.pop(0)
            bits = int(host.item())
            self._pinned_pool.append((host, ev))
            self._raise_for(bits)

    def _poll(self, flags):
        c = self._ctr
        c[0] += 1
        if self.finite_check == "deferred" and c[0] < self.poll_interval:
            return                        # the common step: nothing to look at
        self._poll_due(flags)

    def _poll_due(self, flags):
        self._ctr[0] = 0
        if torch.cuda.is_current_stream_capturing():
            return                        # inside a HIP-graph capture: the flag word is read later
        if self.finite_check == "sync":
            bits = int(flags.item())
            if bits:
                flags.zero_()
            self._raise_for(bits)
        elif self.finite_check == "deferred":
            self.check_flags(block=False)
            self._enqueue_flag_copy(flags)

    def _enqueue_flag_copy(self, flags):
        """async copy of the flag word to a pinned host word (recycled), zeroing it behind"""
        pool = self._pinned_pool
        host, ev = pool.pop() if pool else (torch.empty(1, dtype=torch.int32, pin_memory=True),
                                            torch.cuda.Event())
        host.copy_(flags, non_blocking=True)
        flags.zero_()
        ev.record()
        self._pending.append((host, ev))
        if len(self._pending) > 64:       # nobody is polling: fold the oldest back
            h, e = self._pending.pop(0)
            e.synchronize()
            self._raise_for(int(h.item()))

    # -- fused fast path -----------------------------------------------------------
    def _structure(self):
        """(convs, acts, selector modules) when the module tree qualifies for the fused
        kernels, else None.  Structure is analysed once (modules are assumed static)."""
        if self._plan_cache is not None:
            return self._plan_cache[0]
        from . import nn as G
        from .edge_selectors.temporal import TemporalBackedge
        from .edge_selectors.dense import DenseEdge
        from .edge_selectors.distance import Distance

        def foldable():
            """What sits between the selectors and the GNN (gcm.py:290-306), when the live-row step
            can absorb it: a Linear preprocessor (folded into the layer-1 weights, its bias through
            the row sums of the adjacency), index-writing aux selectors, and - as in the reference only
            when aux selectors exist - the PositionalEncoding ("add": a table added to the rows <= cur
            of the GNN's input; "cat": seen by the aux selectors only, which do not read it)."""
            pre = self.preprocessor
            if isinstance(pre, torch.nn.Sequential) and len(pre) == 1:
                pre = pre[0]
            if pre is not None and type(pre) is not torch.nn.Linear:
                return None
            aux = self.aux_edge_selectors
            if aux is not None and not (isinstance(aux, DenseEdge) or
                                        (isinstance(aux, TemporalBackedge) and not aux.learned)):
                return None
            pe = self.positional_encoder if aux is not None else None   # gcm.py:294-301
            if pe is not None and type(pe) is not PositionalEncoding:
                return None
            if pe is not None and pe.mode == "add" and pre is not None:
                return None
            return {"pre": pre, "aux": aux, "pe": pe}

        def analyse():
            if not self.fused or self.pooled:
                return None
            self._fold = None
            if (self.preprocessor is not None or self.positional_encoder is not None
                    or self.aux_edge_selectors is not None):
                self._fold = foldable()
                if self._fold is None:
                    return None
            g = self.gnn
            if not isinstance(g, G.Sequential) or len(g.arg_names) < 2:
                return None
            xn, an = g.arg_names[0], g.arg_names[1]
            convs, acts = [], []
            for mod, ins, outs in g.stages():
                if isinstance(mod, G.DenseGraphConv):
                    if mod.aggr != "add" or ins != [xn, an] or outs != [xn] or len(convs) == 2:
                        return None
                    convs.append(mod)
                    acts.append(_hip.ACT_NONE)
                elif type(mod) in G._FUSABLE and convs and ins == [xn] and outs == [xn] \
                        and acts[-1] == _hip.ACT_NONE:
                    acts[-1] = G._FUSABLE[type(mod)]
                else:
                    return None
            if len(convs) != 2 or convs[0].out_channels != convs[1].in_channels:
                return None
            native = (TemporalBackedge, DenseEdge, Distance)
            sel = self.edge_selectors
            from .edge_selectors.learned import LearnedEdge
            if isinstance(sel, LearnedEdge):
                # the fused learned step (csrc/learned_step.hip): default edge network only
                if (sel.deterministic or _ops.default_edge_network(sel.edge_network) is None
                        or self._fold is not None):
                    return None
                return convs, tuple(acts), [sel]
            if sel is None:
                mods = []
            elif isinstance(sel, native):
                mods = [sel]
            elif isinstance(sel, G.Sequential):
                mods = []
                names = sel.arg_names
                for mod, ins, outs in sel.stages():
                    if not isinstance(mod, native) or ins != names or outs != names[1:3]:
                        return None
                    mods.append(mod)
            else:
                return None
            if self._fold is not None:
                if any(isinstance(m, Distance) for m in mods):    # (they would need the dX path)
                    return None
                if self._fold["aux"] is not None:
                    mods = mods + [self._fold["aux"]]
            return convs, tuple(acts), mods

        self._plan_cache = (analyse(),)
        return self._plan_cache[0]

    def _fused_plan(self, nodes, adj, weights, F):
        """StepConfig for the fused kernels, or None when this call must take the layered path."""
        st = self._structure()
        if st is None or weights.numel() != 0 or adj.requires_grad or not nodes.is_cuda:
            return None
        last = self._cfg_last
        if last is not None and last[0] == nodes.shape[1] and last[1] == F and last[2] == nodes.device:
            return last[3]
        key = (nodes.shape[1], F, nodes.device)
        cached = self._cfg_cache.get(key)
        if cached is not None:
            return cached if cached is not False else None
        from .edge_selectors.distance import Distance
        from .edge_selectors.learned import LearnedEdge
        convs, acts, mods = st
        N, H1, H2 = nodes.shape[1], convs[0].out_channels, convs[1].out_channels
        cfg = False
        if mods and isinstance(mods[0], LearnedEdge):
            sel = mods[0]
            net = _ops.default_edge_network(sel.edge_network)
            # the kernels index the edge network with the fixed F-wide layout of learned.py:38-51
            # (2F -> F -> F -> 1, LayerNorms over F, every bias present): anything else - e.g. a hidden
            # width G != F, which default_edge_network accepts - takes the layered path
            if (convs[0].in_channels == F and net is not None and net[0].in_features == 2 * F
                    and net[0].out_features == F and net[3].in_features == F and net[3].out_features == F
                    and net[6].in_features == F and net[6].out_features == 1
                    and tuple(net[2].normalized_shape) == (F,) and tuple(net[5].normalized_shape) == (F,)
                    and all(net[i].bias is not None for i in (0, 3, 6))
                    and _hip.lib().gcm_learned_step_supported(N, F, H1, H2)):
                has_bias = (1 if convs[0].lin_rel.bias is not None else 0) | \
                           (2 if convs[1].lin_rel.bias is not None else 0)
                cfg = _ops.StepConfig([], acts, has_bias, N, F, H1, H2, nodes.device)
                cfg.convs = convs
                cfg.lins = (convs[0].lin_rel, convs[0].lin_root, convs[1].lin_rel, convs[1].lin_root)
                cfg.set_learned(sel, net)
        elif self._fold is not None:
            cfg = self._fold_config(convs, acts, mods, N, F, H1, H2, nodes.device)
        elif convs[0].in_channels == F and _ops.gnn2_supported(N, F, H1, H2):
            descs = [m.native_desc(F) if isinstance(m, Distance) else m.native_desc() for m in mods]
            if all(d is not None for d in descs):
                has_bias = (1 if convs[0].lin_rel.bias is not None else 0) | \
                           (2 if convs[1].lin_rel.bias is not None else 0)
                cfg = _ops.StepConfig(descs, acts, has_bias, N, F, H1, H2, nodes.device)
                cfg.convs = convs
                cfg.desc_sources = [m.pointer_source if isinstance(m, Distance) else None for m in mods]
                cfg.sharded = [m for m in mods if isinstance(m, Distance) and m.shard_group is not None]
                cfg.lins = (convs[0].lin_rel, convs[0].lin_root, convs[1].lin_rel, convs[1].lin_root)
        self._cfg_cache[key] = cfg
        if cfg is not False:
            self._cfg_last = (nodes.shape[1], F, nodes.device, cfg)
        return cfg if cfg is not False else None

    def _fold_config(self, convs, acts, mods, N, F, H1, H2, device):
        """StepConfig of a module with a folded preprocessor / positional encoding / aux selectors
        (live-row step only), or False."""
        fold = self._fold
        pre, pe = fold["pre"], fold["pe"]
        Fg = pre.out_features if pre is not None else F
        if (pre is not None and pre.in_features != F) or convs[0].in_channels != Fg:
            return False
        if pe is not None and not hasattr(pe, "pe"):      # the lazily built table / reproject layer
            pe.run_once(torch.empty(0, Fg, device=device))
        pe_add = pe is not None and pe.mode == "add"
        if pe_add and (pe.pe.shape[0] < N or pe.pe.shape[1] < F):
            return False
        descs = [m.native_desc() for m in mods]
        if any(d is None for d in descs):
            return False
        has_bias = (1 if convs[0].lin_rel.bias is not None else 0) | \
                   (2 if convs[1].lin_rel.bias is not None else 0)
        if pre is not None and pre.bias is not None:
            has_bias |= _hip.GNN_HAS_DEG_TERM
        if pe_add:
            has_bias |= _hip.GNN_HAS_PE_TABLE
        cfg = _ops.StepConfig(descs, acts, has_bias, N, F, H1, H2, device)
        if not cfg.rows_ok:
            return False
        cfg.convs = convs
        cfg.desc_sources = [None] * len(descs)
        cfg.lins = (convs[0].lin_rel, convs[0].lin_root, convs[1].lin_rel, convs[1].lin_root)
        cfg.fold = (pre, pe if pe_add else None)
        cfg.dx_ok = False      # (a gradient w.r.t. the observations through a folded transform: the layered path)
        return cfg

    def _fused_head(self, x):
        """forward(x, None) with rows_fused_head: the zero state _fresh_state(x) makes AND the packed vector (+ weight
        image) of this call's configuration out of one launch, or None when the call is not eligible (then _fresh_state
        and _packed_params run as they always did).  The vector lands in _packed_cache; the _packed_params(head=True)
        of this very call finds it there (_head_ready)."""
        if (not self.rows_fused_head or not x.is_cuda or x.dim() != 2 or x.dtype != torch.float32 or self.edge_weights
                or x.device.index != torch.cuda.current_device()):
            return None
        N, F = self.graph_size, x.shape[1]
        last = self._cfg_last
        if last is not None and last[0] == N and last[1] == F and last[2] == x.device:
            cfg = last[3]
        else:   # (what forward() asks below, of tensors that only carry the shape)
            shape = torch.empty(0, N, F, device=x.device)
            cfg = self._fused_plan(shape, shape, torch.empty(0, device=x.device), F)
            if cfg is None:
                return None
        state = []
        self._packed_params(cfg, head=True, fresh=(x.shape[0], N, F, state))
        self._head_ready = (cfg, torch.is_grad_enabled())
        if not state or state[0] is None:   # (no one-launch form, or an empty batch: the vector is kept for this call)
            return None
        nodes, adj, num_nodes = state
        return nodes, adj, torch.zeros(0, device=x.device), num_nodes

    def _packed_params(self, cfg, head=False, fresh=None):
        """The six GNN tensors as one flat vector (layout of include/gcm_hip.h "packed parameter
        vector"), so that a step returns ONE gradient tensor.  Rebuilt at the head of every chain
        of hidden states (`head`: hidden is None or not produced by this module - the reference
        reads live parameters, and writes through `.data` / `module.float()` bump no version
        counter), when a parameter changed, or after the previous vector took part in a backward
        pass; reused only inside a linked chain."""
        # current parameter tensors through the modules' own dicts (nn.Module.__getattr__ chains
        # cost ~0.5 us each and this runs every step)
        (rel0, root0, rel1, root1) = cfg.lins
        tensors = (rel0._parameters["weight"], root0._parameters["weight"], rel0._parameters["bias"],
                   rel1._parameters["weight"], root1._parameters["weight"], rel1._parameters["bias"])
        if cfg.learned_sel is not None:     # ... | edge network (layout of gcm_learned_* in gcm_hip.h)
            l0, _, n0, l1, _, n1, l2 = cfg.mlp_mods
            tensors = tensors + (l0.weight, l0.bias, n0.weight, n0.bias, l1.weight, l1.bias, n1.weight,
                                 n1.bias, l2.weight, l2.bias)
        fold = cfg.fold
        if fold is not None and fold[0] is not None:
            tensors = tensors + (fold[0]._parameters["weight"], fold[0]._parameters["bias"])
        cache = self._packed_cache
        ready, self._head_ready = self._head_ready, None
        if (ready is not None and head and cache is not None and ready[0] is cfg
                and ready[1] == torch.is_grad_enabled() == cache[0]):
            return cache[1]      # (this call's own head: _fused_head built it with the state a moment ago)
        if cache is not None and not head and not cache[2][0] and cache[0] == torch.is_grad_enabled():
            # valid while the very same tensor objects have not been written to (optimizer steps
            # bump _version; re-assigned Parameters are new objects)
            live = True
            for t, (t0, v0) in zip(tensors, cache[3]):
                if t is not t0 or (t is not None and t._version != v0):
                    live = False
                    break
            if live:
                return cache[1]
        # drop the previous vector FIRST: its graph keeps the parameters' AccumulateGrad nodes alive,
        # bound to the stream they were created on - a later HIP-graph capture of this module would
        # then be made to synchronise with that (possibly the default) stream and fail
        self._packed_cache = cache = None
        self._learned_chain = None
        if cfg._rows_fast is not None:
            cfg._rows_fast.forget()
        if cfg._learned_fast is not None:
            cfg._learned_fast.forget()
        key = torch.is_grad_enabled()
        sizes = (cfg.H1 * cfg.F, cfg.H1 * cfg.F, cfg.H1, cfg.H2 * cfg.H1, cfg.H2 * cfg.H1, cfg.H2)
        if cfg.learned_sel is not None:
            Fe = cfg.F
            sizes = sizes + (2 * Fe * Fe, Fe, Fe, Fe, Fe * Fe, Fe, Fe, Fe, Fe, 1)
        dev = tensors[0].device
        image = None
        if fold is None and all(t is not None for t in tensors):
            # (one autograd node: every parameter's gradient a view)
            if (head and self.rows_fused_head and len(tensors) <= 16 and dev.type == "cuda"
                    and dev.index == torch.cuda.current_device()
                    and all(t.dtype is torch.float32 and t.device == dev and t.is_contiguous() for t in tensors)):
                # ... and the weight image, and a fresh state, out of the same launch
                want_image = cfg.learned_sel is None and max(cfg.F, cfg.H1, cfg.H2) <= 64
                B, N, F = fresh[:3] if fresh is not None else (0, 0, 0)
                # (under a capture the chain's run object remembers the launch: its merged step node may absorb it)
                absorb = bool(fresh is not None and self.rows_absorb_head and self.rows_merge_captured
                              and self.rows_merge_cap != 1 and cfg.rows_ok and cfg.learned_sel is None)
                packed, image, *state = _ops._ext.module().pack_params_head(
                    list(tensors), cfg.F, cfg.H1, cfg.H2, want_image, B, N, F,
                    cfg.rows_fast(self) if absorb else cfg._rows_fast, absorb)
                if fresh is not None:
                    fresh[3].extend(state)
            else:
                packed = _ops._ext.module().pack_params(list(tensors))
        else:
            parts = [t.reshape(-1) if t is not None else torch.zeros(n, device=dev)
                     for t, n in zip(tensors, sizes)]
            if fold is not None:
                parts = self._folded_parts(cfg, tensors, parts)
            packed = torch.cat(parts)
        if cfg.learned_sel is not None:
            assert packed.numel() == cfg.P_total, "edge network does not have the fused kernels' layout"
        used = [False]
        if packed.requires_grad:
            packed.register_hook(lambda g: used.__setitem__(0, True))
        # (the gate of the per-step fused nodes - _gate() - is made when one of them first asks for it)
        gate = [None, None, cfg.P, dev]
        for d in cfg.descs:               # a re-assigned dist_param must not leave a stale pointer
            if d.kind == _hip.SEL_DISTANCE:
                cfg.refresh_pointers()
                break
        self._packed_cache = (key, packed, used,
                              [(t, t._version if t is not None else 0) for t in tensors], gate, image)
        return packed

    def _gate(self):
        """(gated packed vector, slab holder) of the current packed vector - what the per-step fused nodes consume
        the parameters through in grad mode (_ops._ParamGate: their parameter-gradient slabs summed once) - or
        (None, None) without gradients.  Made on first use: the live-row and rollout paths never ask."""
        pc = self._packed_cache
        g = pc[4]
        if g[0] is None and pc[1].requires_grad:
            g[1] = _ops.SlabHolder(g[2], g[3])
            g[0] = _ops.param_gate(pc[1], g[1])
        return g[0], g[1]

    @staticmethod
    def _folded_parts(cfg, tensors, parts):
        """Packed vector of a folded configuration (include/gcm_hip.h, "Folded node transforms"):
        layer 1 composed with the Linear preprocessor x' = W_p x + b_p -
            W_rel1 W_p | W_root1 W_p | b1 + W_root1 b_p | layer 2 | c1 = W_rel1 b_p | pe table
        built with torch ops, so autograd carries the kernel's gradient back to W_p, b_p and the
        original layer-1 tensors."""
        pre, pe = cfg.fold
        if pre is not None:
            w_rel, w_root, b1 = tensors[0], tensors[1], tensors[2]
            w_p, b_p = tensors[-2], tensors[-1]
            parts[0] = (w_rel @ w_p).reshape(-1)
            parts[1] = (w_root @ w_p).reshape(-1)
            if b_p is not None:
                parts[2] = parts[2] + w_root @ b_p
                parts.append(w_rel @ b_p)
        if pe is not None:
            parts.append(pe.pe[: cfg.N, : cfg.F].reshape(-1))
        return parts

    @staticmethod
    def _gather_sharded(cfg, x):
        """EuclideanEdge(shard_group=...): every rank's current nodes (= the observations going in) into
        the selector's persistent buffer, ahead of the kernels that read it (SURVEY 8e "Exception")."""
        for m in cfg.sharded:
            if m.gather_current(x):
                cfg.refresh_pointers()

    @staticmethod
    def _trains_gnn(cfg):
        """Does any of the six GNN tensors take a gradient?  The live-row chain hangs the observations' gradient on the
        node of the PARAMETER gradient (RowsChainNode / DxGateNode in csrc/torch_ext/step_ext.cpp, made only when the
        packed vector requires one): a frozen GNN behind a trainable encoder has no such node, and its beliefs would
        come back without a grad_fn.  Those calls take the fused per-step node, which differentiates w.r.t. whichever
        of (x, nodes, parameters) asks.  Looked at only when the observations need a gradient."""
        for lin in cfg.lins:
            for p in lin._parameters.values():
                if p is not None and p.requires_grad:
                    return True
        return False

    def _forward_rows(self, x, hidden, cfg, flags, link, need_dx=0):
        """The live-row step (csrc/rows_step.hip), checked entry: one kernel forward, no kernel and no
        autograd node per step backward (every step of a chain hangs its belief tensor on one node,
        whose backward is one time-parallel launch over every recorded step).  Taken when neither x
        nor the incoming node matrix needs a gradient.  A continuing chain does not come through
        here at all: DenseGCM.__call__ hands it to the C++ host path (RowsFast.step) directly."""
        nodes, adj, weights, num_nodes = hidden
        fast = cfg.rows_fast(self)
        if need_dx and fast.edited_dx_state(nodes, adj, weights, num_nodes):
            # The chain's dL/dx follows the rows of the node matrix back to the steps that inserted them BY POSITION;
            # a state the caller has edited in place (zeroed graphs of finished episodes ...) no longer has that form.
            if fast.donates():
                raise RuntimeError("donate_state=True with observation gradients: the hidden state was modified in "
                                   "place between two steps of a chain - use functional state (donate_state=False), "
                                   "or detach the chain (start it again from the edited state under a new call)")
            self._fast = None
            return self._forward_fused(x, nodes, adj, weights, num_nodes, cfg, flags, link)   # (full state saved)
        cont = fast.continues(nodes, adj, weights, num_nodes)
        root = self._packed_params(cfg, head=link is None and not cont)
        if not x.is_contiguous():
            x = x.contiguous()
        if not (nodes.is_contiguous() and adj.is_contiguous() and num_nodes.is_contiguous()):
            if self.donate_state:
                raise ValueError("donate_state=True needs contiguous hidden-state tensors")
            nodes, adj, num_nodes = nodes.contiguous(), adj.contiguous(), num_nodes.contiguous()
        # (a donated state with a gradient w.r.t. the observations: only in the one-node form, and the returned
        #  node matrix is then a plain tensor - RowsFast::want_donate decides and reports)
        fresh = getattr(nodes, "_gcm_fresh", False)
        if fresh:
            nodes._gcm_fresh = False          # (a donated state is this very tensor at every later step)
            if cfg.cpp_handle():
                cfg._cpp.set_cached_flags(
                    (0 if (self.rows_one_launch_distance or not cfg.has_distance) else _hip.STEP_TWO_LAUNCH)
                    | (_hip.STEP_IMG_V4 if self.rows_weight_image_v4 else 0)
                    | (0 if self.rows_bookkeeping_wave else _hip.STEP_ONE_WAVE)
                    | (0 if self.rows_lean_step else _hip.STEP_NOT_LEAN))
                cfg._cpp.set_col_cache(bool(self.rows_col_cache))
                cfg._cpp.set_hops_bptt(bool(self.rows_hops_bptt))
                cfg._cpp.set_hops_fold(bool(self.rows_hops_fold))
                cfg._cpp.set_merge_captured(bool(self.rows_merge_captured), int(self.rows_merge_cap or 0))
                cfg._cpp.set_absorb_head(bool(self.rows_absorb_head))
                cfg._cpp.set_run_mfma(bool(self.rows_run_mfma))
            image = self._packed_cache[5]
            if image is not None and self._packed_cache[1] is root:
                fast.set_head_image(root, image)   # (the first cached step takes it iff it is armed with this vector)
        mx, n2, a2, c2, donate = fast.run(x, nodes, adj, weights, num_nodes, root, flags, cfg.cpp_handle(),
                                          self.donate_state, need_dx, bool(fresh and self.rows_cached_steps))
        if donate:
            out = hidden
        else:
            if self.mutate_num_nodes_on_overflow:
                num_nodes.copy_(c2 - 1)
            out = (n2, a2, weights, c2)
        # the next call of this module tries the unchecked entry first (not with the compat flag that
        # writes into the caller's num_nodes: that needs the checked path every step)
        if self.mutate_num_nodes_on_overflow or cfg.sharded:   # (a collective ahead of every step)
            self._fast = None
        else:    # (bound C++ entry, flag word, steps between looks at it)
            every = {"deferred": self.poll_interval, "sync": 1, "off": float("inf")}[self.finite_check]
            self._fast = (fast.step, flags, every)
        if self.finite_check != "off":
            self._poll(flags)
        return mx, out

    def _forward_learned(self, x, hidden, cfg, flags, link):
        """DenseGCM + LearnedEdge as fused kernels (csrc/learned_step.hip), one time-parallel backward per chain.
        The returned adjacency carries no autograd history of its own: it carries the index of the step that
        wrote it (`_gcm_lin`), which the chain's backward follows."""
        nodes, adj, weights, num_nodes = hidden
        root = self._packed_params(cfg, head=link is None)
        B = x.shape[0]
        sel = cfg.learned_sel
        if sel.noise_fn is not None:      # injected gumbel draws (parity tests); values of the argument unspecified
            noise, is_exp = sel.noise_fn(torch.empty(B, cfg.N, device=x.device)), 0
        else:                             # torch.nn.functional.gumbel_softmax draws -log(Exp(1)) the same way
            # (noise_pool_steps steps' worth per draw: one RNG launch instead of one per step - and a refill is a
            #  step on the interpreter's path: 64 since round 6, the RNG launches were 36 of a cfg5 rollout's 550 us)
            # A pool drawn outside a HIP-graph capture is not used inside one (and vice versa): the
            # captured kernels would keep reading its address after it has been replaced.
            pool, cap = self._noise_pool, torch.cuda.is_current_stream_capturing()
            if (pool is None or pool[1] >= pool[0].shape[0] or pool[2] != cap or pool[0].shape[1] != B
                    or pool[0].device != x.device):
                pool = self._noise_pool = [torch.empty(max(1, int(self.noise_pool_steps)), B, cfg.N,
                                                       device=x.device).exponential_(), 0, cap]
            noise, is_exp = pool[0][pool[1]], 1
            pool[1] += 1
        ext = _ops._ext.module()
        # every step of a chain of hidden states hangs its belief tensor on ONE autograd node
        # (LearnedChainNode in csrc/torch_ext/step_ext.cpp); the adjacency carries the index of the step
        # that wrote it, so that the time-parallel backward can follow the chain (or tree) of states
        lc = self._learned_chain
        # (a chain that starts from the empty graphs of hidden = None runs its first N steps as cached steps,
        #  LearnedChain in step_ext.cpp: its caches belong to ONE such rollout)
        fresh = getattr(nodes, "_gcm_fresh", False)
        if fresh:
            nodes._gcm_fresh = False      # (a donated state is this very tensor at every later step)
        fresh = fresh and self.learned_cached_steps
        if (lc is None or lc[0] is not root or lc[1].executed() or lc[2] != torch.is_grad_enabled()
                or (fresh and lc[1].total_steps() > 0)):
            lc = self._learned_chain = (root, ext.LearnedChain(cfg.learned_cpp_handle(), root,
                                                               bool(self.donate_state)),
                                        torch.is_grad_enabled())
        lin = getattr(adj, "_gcm_lin", None)
        parent = lin[1] if (lin is not None and lin[0] is lc[1]) else -1
        mx, n2, a2, cur, c2, idx = ext.learned_step2(lc[1], x, nodes, adj, num_nodes, noise, is_exp, flags, parent,
                                                     bool(fresh))
        if idx >= 0:
            a2._gcm_lin = (lc[1], idx)
        # the next call of this chain may skip the interpreter: DenseGCM.__call__ -> LearnedFast.step (C++)
        if sel.noise_fn is None and not self.mutate_num_nodes_on_overflow and self.learned_fast_path:
            lf = cfg.learned_fast(self)
            lf.arm(lc[1], self._noise_pool, self._token, weakref.ref(cfg), flags, root, weights, idx, B, x.shape[1],
                   cfg.N)
            every = {"deferred": self.poll_interval, "sync": 1, "off": float("inf")}[self.finite_check]
            self._fast = (lf.step, flags, every)
        if lc[1].donates():      # the state was advanced in place: the caller's own tuple
            n2._gcm_link = (self._token, a2, cfg, flags, None, root, x.shape, weights, c2)
            if self.mutate_num_nodes_on_overflow:
                raise NotImplementedError("mutate_num_nodes_on_overflow with donate_state")
            if self.finite_check != "off":
                self._poll(flags)
            return mx, hidden
        n2._gcm_link = (self._token, a2, cfg, flags, None, root, x.shape, weights, c2)
        if self.mutate_num_nodes_on_overflow:
            num_nodes.copy_(cur)
        if self.finite_check != "off":
            self._poll(flags)
        return mx, (n2, a2, weights, c2)

    def _forward_fused(self, x, nodes, adj, weights, num_nodes, cfg, flags, link=None):
        root = self._packed_params(cfg, head=link is None)
        gated, holder = self._gate()
        # In grad mode the steps consume the parameter vector through a gate node and accumulate
        # their parameter-gradient slabs into ONE array of the module (summed once by the gate,
        # _ops._ParamGate) instead of returning T gradients for the engine to add.
        # `_gcm_link` on the returned node matrix lets the next call skip re-validating a hidden
        # state this module produced itself, and tells whether it continues the same chain.
        if gated is not None:
            is_head = link is None or link[5] is not root
            packed, slab_acc = gated, holder.get(x.shape[0])
        else:
            is_head, packed, slab_acc = True, root, None
        fast = cfg.cpp_call()     # (function, handle, device index) of the C++ node: no wrapper layers
        mx, nodes_out, adj_out, cur, num_nodes_next = fast[0](
            x, nodes, packed, adj, num_nodes, flags, fast[1], torch._C._cuda_getCurrentRawStream(fast[2]),
            slab_acc, is_head)
        nodes_out._gcm_link = (self._token, adj_out, cfg, flags, None, root, x.shape, weights,
                               num_nodes_next)
        if self.mutate_num_nodes_on_overflow:
            num_nodes.copy_(cur)
        if self.finite_check != "off":
            self._poll(flags)
        return mx, (nodes_out, adj_out, weights, num_nodes_next)

    def _has_learned_edge(self):
        from .edge_selectors.learned import LearnedEdge
        return any(isinstance(m, LearnedEdge) for sel in (self.edge_selectors, self.aux_edge_selectors)
                   if sel is not None for m in sel.modules())

    def _check_reset(self, reset, T, B, what):
        """Argument checks of a reset mask, before anything is launched."""
        if not isinstance(reset, torch.Tensor) or reset.dtype != torch.bool:
            raise TypeError(f"{what} must be a torch.bool tensor, got "
                            f"{reset.dtype if isinstance(reset, torch.Tensor) else type(reset).__name__}")
        want = (B,) if T is None else (T, B)
        if tuple(reset.shape) != want:
            raise ValueError(f"{what} must have shape {list(want)}, got {list(reset.shape)}")
        if self._has_learned_edge():
            # its adjacency carries the chain's gradient by step index (_gcm_lin): clearing some graphs of that tensor
            # needs a design of its own
            raise NotImplementedError("episode resets with a dense LearnedEdge selector are not implemented yet "
                                      "(follow-up: per-graph resets of the LearnedEdge chain, whose adjacency carries "
                                      "the gradient by step index); reset such a memory by starting a new rollout")

    def reset_hidden(self, hidden, mask):
        """The hidden state with the graphs of `mask` (bool [B], on the device or the CPU) emptied: node rows, adjacency,
        weights if present, num_nodes = 0 - what an RL loop does to the memories of finished episodes, as one launch
        (gcm_state_reset) and one autograd function (the gradient w.r.t. a cleared graph's incoming state is zero, the
        others' the identity).  Functional by default: new tensors, the inputs untouched.  With donate_state=True the
        given tensors are cleared in place and returned, and the running chain of cached steps ends (the next step
        reads the state itself)."""
        self._check_reset(mask, None, hidden[0].shape[0], "mask")
        return self._apply_reset(hidden, mask)

    def _apply_reset(self, hidden, mask):
        nodes, adj, weights, num_nodes = hidden
        if nodes.is_cuda and nodes.device.index != torch.cuda.current_device():
            with torch.cuda.device(nodes.device):
                return self._apply_reset(hidden, mask)
        if mask.device != nodes.device:
            mask = mask.to(nodes.device)
        mask = mask.contiguous()
        if self.donate_state:
            if not (nodes.is_contiguous() and adj.is_contiguous() and num_nodes.is_contiguous()
                    and weights.is_contiguous()):
                raise ValueError("donate_state=True needs contiguous hidden-state tensors")
            _ops.state_reset(nodes, adj, weights, num_nodes, mask, True)
            # the cached-step chains read per-chain caches and the host's step count, not the state: the version
            # counters moved (RowsFast::state_untouched), and the unchecked entries are dropped outright
            self._fast = None
            self._learned_chain = None
            return hidden
        n2, a2, w2, c2 = _ops.state_reset(nodes, adj, weights, num_nodes, mask, False)
        return n2, a2, (w2 if weights.numel() else weights), c2

    def _reset_plan(self, reset, device):
        """(reset on the device [T, B], list of T bools: does step t clear a graph) - learned with ONE host read per
        call (`reset.any(1)`), none at all when `reset` lives on the CPU."""
        if reset.is_cuda:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DenseGCM.rollout(reset=...) on the per-step path reads which steps have a reset on "
                                   "the host: inside a stream capture pass `reset` as a CPU tensor")
            return reset.contiguous(), reset.any(1).tolist()
        steps = reset.any(1).tolist()
        return reset.contiguous().to(device), steps

    def rollout(self, obs, hidden=None, batch_first=False, truncate=True, reset=None):
        """T memory steps at once: obs [T, B, feat] -> (beliefs [T, B, H], hidden after the
        last step); batch_first=True: obs [B, T, feat] -> beliefs [B, T, H] - the shape RLlib's wrapper holds
        (ray_gcm.py:186-209: `flat` [B, T, F] in, the stacked beliefs [B*T, H] out).  The VALUES (beliefs, hidden
        state) are those of T calls of forward(), and so is every gradient that flows inside the call.  Index-writing
        selectors on the canonical GNN: the whole rollout is enqueued by one C call and is one autograd node;
        EuclideanEdge alone and LearnedEdge from empty graphs: time-parallel forwards (csrc/euclid_tp.hip,
        gcm_learned_rollout_fwd); every other configuration runs the per-step kernels in a loop - on a state this
        call owns, so the steps advance it IN PLACE whatever `donate_state` says (the caller never sees the
        intermediate states; the incoming state is copied once).

        truncate (LearnedEdge only - the one selector whose ADJACENCY carries a gradient, learned.py:89-113): True
        (default) - the hidden state going in and the one coming out are plain tensors: truncated BPTT at the call
        boundary, which is what RLlib's state passing does (ray_gcm.py:186-209 hands states over as detached
        batches).  A later call's loss then does not reach this call's edge selections through the returned
        adjacency, as it would across T forward() calls.  False: the chain of hidden states is kept across the call
        boundary exactly as T forward() calls keep it (functional state, per-step kernels; slower).

        reset (bool [T, B]; [B, T] with batch_first; on the device or the CPU): reset[t, b] empties graph b (node rows,
        adjacency, weights, num_nodes = 0) BEFORE obs[t, b] is inserted - episodes that end inside the batch.  Values,
        final hidden state and gradients are those of T forward() calls with reset_hidden() between them.  From
        hidden = None with forward temporal hops the forward stays time-parallel (csrc/rollout_reset.hip: the validity
        of a hop decided per graph, no host read); every other configuration runs the per-step loop with one masked
        clear (gcm_state_reset) ahead of each step that has a reset.  None: no resets, the launches of before."""
        assert obs.dim() == 3 and obs.dtype == torch.float32
        if batch_first:
            if isinstance(reset, torch.Tensor) and reset.dim() == 2:
                reset = reset.transpose(0, 1)
            out, hidden = self.rollout(obs.transpose(0, 1), hidden, truncate=truncate, reset=reset)
            return out.transpose(0, 1), hidden
        if reset is not None:
            self._check_reset(reset, obs.shape[0], obs.shape[1], "reset")
        if obs.is_cuda and obs.device.index != torch.cuda.current_device():
            with torch.cuda.device(obs.device):
                return self.rollout(obs, hidden, truncate=truncate, reset=reset)
        if not truncate and torch.is_grad_enabled():
            from .edge_selectors.learned import LearnedEdge
            if any(isinstance(m, LearnedEdge) for sel in (self.edge_selectors, self.aux_edge_selectors)
                   if sel is not None for m in sel.modules()):
                outs = []
                for t in range(obs.shape[0]):        # T forward() calls: the chain (_gcm_lin / adj.grad_fn) survives
                    mx, hidden = self(obs[t], hidden)
                    outs.append(mx)
                if not outs:
                    return self.rollout(obs, hidden)
                return torch.stack(outs), hidden
        if obs.shape[0] == 0:
            if hidden is None:
                hidden = self.get_initial_hidden_state(obs[0] if obs.shape[0] else obs.new_zeros(obs.shape[1:]))
            return obs.new_zeros(0, obs.shape[1], 0), hidden
        fresh = hidden is None
        if fresh and not self.edge_weights:
            # (the plan looks at shapes and devices only: the 21 MB empty state is materialised by whoever needs it)
            z = obs.new_empty(0, self.graph_size, obs.shape[-1])
            cfg = self._fused_plan(z, obs.new_empty(0, self.graph_size, self.graph_size), obs.new_zeros(0), obs.shape[-1])
            # (T <= N: the adjacency entries a step writes are read by later steps' layer 1 - their gradient reaches
            #  the selection through ONE chain's records, so a rollout is not split at the overflow)
            if (cfg is not None and cfg.learned_sel is not None and self.learned_cached_steps
                    and obs.shape[0] <= self.graph_size and not (torch.is_grad_enabled() and obs.requires_grad)):
                return self._rollout_learned(obs, cfg)
            # forward temporal hops only, from empty graphs, observations without gradient: no recurrence at all - the
            # whole forward as two launches over every (step, graph) (csrc/rollout_tp.hip), one autograd node
            if (cfg is not None and cfg.learned_sel is None and cfg.fold is None and cfg.rows_ok
                    and self.rollout_time_parallel
                    and not (torch.is_grad_enabled() and obs.requires_grad)):
                if cfg.cpp_handle():
                    flags = self._flag_word(obs.device)
                    cfg._cpp.set_hops_bptt(bool(self.rows_hops_bptt))
                    cfg._cpp.set_hops_fold(bool(self.rows_hops_fold))
                    if reset is None:
                        r = _ops._ext.module().rows_rollout_tp(cfg.cpp_handle(), self._packed_params(cfg, head=True),
                                                               obs, flags)
                    else:      # (copied to the device once if it came from the CPU: this path reads nothing back)
                        r = _ops._ext.module().rows_rollout_tp(
                            cfg.cpp_handle(), self._packed_params(cfg, head=True), obs, flags,
                            reset.contiguous() if reset.is_cuda else reset.contiguous().to(obs.device))
                    if r is not None:
                        mx, nodes, adj, count = r
                        if self.finite_check == "sync":
                            self.check_flags()
                        elif self.finite_check == "deferred" and not torch.cuda.is_current_stream_capturing():
                            self.check_flags(block=False)
                            self._enqueue_flag_copy(flags)
                        # (with resets the kernel raises it: whether an episode outgrows the graph is not known here)
                        if reset is None and obs.shape[0] > self.graph_size and self.finite_check != "off":
                            flags.bitwise_or_(_hip.FLAG_WRAPPED)     # gcm.py:264-266: the one-time overflow notice
                        return mx, (nodes, adj, torch.zeros(0, device=obs.device), count)
        if fresh:
            hidden = self.get_initial_hidden_state(obs[0])
        nodes, adj, weights, num_nodes = hidden
        if reset is not None:             # the per-step kernels, a masked clear ahead of every step that has a reset
            return self._rollout_loop(obs, hidden, fresh, self._reset_plan(reset, obs.device))
        cfg = self._fused_plan(nodes, adj, weights, obs.shape[-1])
        if cfg is not None and (cfg.learned_sel is not None or cfg.fold is not None):
            cfg = None                    # LearnedEdge / folded transforms: the per-step kernels, in a loop
        elif (cfg is not None and cfg.has_distance and cfg.rows_ok
              and not (torch.is_grad_enabled() and (obs.requires_grad or nodes.requires_grad))):
            cfg = None                    # distance selectors: selector kernel + live-row step per step
        if cfg is None:
            return self._rollout_loop(obs, hidden, fresh)
        B, N = obs.shape[1], nodes.shape[1]
        assert (nodes.shape[0], adj.shape, num_nodes.shape[0], nodes.shape[2]) == \
            (B, (B, N, N), B, obs.shape[2]), "hidden state and observation shapes disagree"
        flags = self._flag_word(obs.device)
        mx_all, nodes_T, adj_T, count_T = _ops.fused_rollout(
            obs, nodes, self._packed_params(cfg, head=True), adj, num_nodes, flags, cfg)
        if self.finite_check == "sync":
            self.check_flags()
        elif self.finite_check == "deferred" and not torch.cuda.is_current_stream_capturing():
            self.check_flags(block=False)      # gcm.py:316-318 for rollout-only loops
            self._enqueue_flag_copy(flags)
        return mx_all, (nodes_T, adj_T, weights, count_T)

    def _rollout_learned(self, obs, cfg):
        """rollout() with LearnedEdge from hidden = None, T <= graph_size steps, observations without gradient: TWO
        launches (gcm_learned_rollout_fwd: the selection of a step depends on raw observations and its gumbel draws
        only, so every (graph, step) is a workgroup of one launch; the beliefs follow in a second one) and one
        autograd node whose backward is the chain's time-parallel one.  The hidden state it returns is a plain
        tensor tuple: like every rollout() it ends its gradient chain (a later call's gradient does not reach this
        rollout's selections - truncated BPTT at the call boundary, which is what RLlib's state passing does)."""
        T, B = obs.shape[0], obs.shape[1]
        N = cfg.N
        # (gcm_learned_rollout_fwd: GCM_EUNSUPPORTED above 65535 graphs - ADVICE r4)
        if (N & 3) or (cfg.F & 3) or B > 65535:
            return self._rollout_loop(obs, self.get_initial_hidden_state(obs[0]), True)
        root = self._packed_params(cfg, head=True)
        sel = cfg.learned_sel
        if sel.noise_fn is not None:      # injected gumbel draws (parity tests): one call per step, in step order
            noise = torch.stack([sel.noise_fn(torch.empty(B, N, device=obs.device)) for _ in range(T)])
            is_exp = 0
        else:                             # torch.nn.functional.gumbel_softmax draws -log(Exp(1)) the same way
            noise, is_exp = torch.empty(T, B, N, device=obs.device).exponential_(), 1
        flags = self._flag_word(obs.device)
        mx, nodes, adj, count = _ops._ext.module().learned_rollout(cfg.learned_cpp_handle(), root, obs, noise, is_exp,
                                                                   flags)
        if self.finite_check == "sync":
            self.check_flags()
        elif self.finite_check == "deferred" and not torch.cuda.is_current_stream_capturing():
            self.check_flags(block=False)
            self._enqueue_flag_copy(flags)
        return mx, (nodes, adj, torch.zeros(0, device=obs.device), count)

    def _rollout_loop(self, obs, hidden, fresh, reset_plan=None):
        """rollout() as the loop of per-step calls.  The intermediate hidden states never leave this function, so -
        when no gradient flows through the state itself - the steps run on a state this call owns and advance it in
        place (the live-row / LearnedEdge kernels' donated form: no per-step copy of the 21 MB state), whatever the
        module's `donate_state`; a chain from hidden = None also gets the cached steps."""
        nodes = hidden[0]
        own = (not self.donate_state and self.fused and nodes.is_cuda and hidden[2].numel() == 0
               and not (torch.is_grad_enabled() and (obs.requires_grad or nodes.requires_grad or hidden[1].requires_grad)))
        if own:
            if fresh:
                hidden = None             # (the module's own empty graphs: the cached steps' precondition)
            else:
                hidden = (nodes.clone(), hidden[1].clone(), hidden[2], hidden[3].clone())
            self.donate_state = True
        try:
            outs = []
            for t in range(obs.shape[0]):
                # (a state this call owns is cleared in place, like the steps advance it; hidden = None: empty graphs)
                if reset_plan is not None and reset_plan[1][t] and hidden is not None:
                    hidden = self._apply_reset(hidden, reset_plan[0][t])
                mx, hidden = self(obs[t], hidden)
                outs.append(mx)
        finally:
            if own:
                self.donate_state = False
                self._fast = None         # (the C++ entry and the LearnedEdge chain were armed for a donated state)
                self._learned_chain = None
        return torch.stack(outs), hidden

    # -- the step --------------------------------------------------------------
    def __call__(self, *args, **kwargs):
        """`belief, m = gcm(obs, m)`.  A step that continues the chain of the previous call on the
        live-row kernels is ONE call into the C++ host path (RowsFast.step validates exactly that:
        same hidden-state tensors as returned last, same observation shape, parameters untouched, grad
        mode unchanged, no module / global hooks registered); everything else goes through
        torch.nn.Module.__call__ and forward() below."""
        fast = self._fast
        if fast is not None and not kwargs and len(args) == 2:
            r = fast[0](args[0], args[1])
            if r is not None:
                c = self._ctr           # gcm.py:316-318, deferred: look at the flag word now and then
                c[0] += 1
                if c[0] >= fast[2]:
                    self._poll_due(fast[1])
                return r
        return torch.nn.Module.__call__(self, *args, **kwargs)

    def __getstate__(self):
        """copy.deepcopy / pickle of a module that has already run: the per-shape plans, the packed
        parameter vector and the C++ host path are runtime caches (rebuilt on the first call)."""
        d = dict(self.__dict__)
        d.update(_plan_cache=None, _fold=None, _noise_pool=None, _token=object(), _cfg_cache={}, _cfg_last=None,
                 _packed_cache=None, _head_ready=None, _flags={}, _pending=[], _pinned_pool=[], _ctr=[0], _fast=None,
                 _learned_chain=None, _flag_user_list=None)
        return d

    def forward(
        self,
        x,
        hidden: Union[None, Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]],
    ) -> Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]:
        """x [B, feat]; hidden = (nodes [B,N,feat], adj [B,N,N], weights [B,N,N] | [0],
        num_nodes [B]) or None.  Returns (belief [B, H], new hidden)."""
        if hidden is None:
            hidden = self._fused_head(x) or self._fresh_state(x)
            hidden[0]._gcm_fresh = True     # empty graphs: what the cached LearnedEdge steps may rely on
            try:
                return self._forward(x, hidden)
            finally:
                self._head_ready = None     # (a head vector no path of this call asked for is not the next call's)
        return self._forward(x, hidden)

    def _forward(self, x, hidden):
        """forward() on a hidden state that exists."""
        nodes, adj, weights, num_nodes = hidden

        # the kernels are launched on the CURRENT device's stream: tensors on another GPU get a
        # device guard for the call (PyTorch ops in the reference guard implicitly)
        if x.is_cuda and x.device.index != torch.cuda.current_device():
            with torch.cuda.device(x.device):
                return self._forward(x, hidden)

        # A hidden state this module returned itself (same node / adjacency tensors, same input
        # shape): everything checked below held for it by construction.
        link = getattr(nodes, "_gcm_link", None)
        if (link is not None and link[0] is self._token and link[1] is adj and link[7] is weights
                and link[8] is num_nodes and x.shape == link[6] and x.dtype is torch.float32):
            cfg = link[2]
            no_dx = not (torch.is_grad_enabled() and (x.requires_grad or nodes.requires_grad))
            if cfg.sharded:
                self._gather_sharded(cfg, x)
            if cfg.rows_ok and (no_dx or (cfg.dx_ok and self.rows_dx and self._trains_gnn(cfg))):
                return self._forward_rows(x, hidden, cfg, link[3], link, 0 if no_dx else (2 if self.rows_dx == "steps" else 1))
            if cfg.learned_sel is None and cfg.fold is None:
                return self._forward_fused(x, nodes, adj, weights, num_nodes, cfg, link[3], link)
            if no_dx:
                return self._forward_learned(x, hidden, cfg, link[3], link)
            # (observations with gradient: the layered path below)

        # gcm.py:246-260, as one comparison
        if (x.dtype, nodes.dtype, adj.dtype, weights.dtype, num_nodes.dtype, num_nodes.dim()) != _DTYPES:
            assert x.dtype == torch.float32
            assert nodes.dtype == torch.float
            assert adj.dtype == torch.float, "adj must be float32"
            assert weights.dtype == torch.float
            assert num_nodes.dtype == torch.long
            assert num_nodes.dim() == 1
        N = nodes.shape[1]
        B = x.shape[0]
        assert N == adj.shape[1] == adj.shape[2], "N must be equal for adj mat and node mat"

        flags = self._flag_word(x.device)
        plan = self._fused_plan(nodes, adj, weights, x.shape[-1])
        if plan is not None:
            # raw pointers from here on: the shapes must agree (the reference raises an indexing
            # error on a mismatched hidden state)
            assert (nodes.shape[0], adj.shape[0], num_nodes.shape[0], nodes.shape[2]) == \
                (B, B, B, x.shape[1]), "hidden state and observation shapes disagree"
            no_dx = not (torch.is_grad_enabled() and (x.requires_grad or nodes.requires_grad))
            if plan.sharded:
                self._gather_sharded(plan, x)
            if plan.rows_ok and (no_dx or (plan.dx_ok and self.rows_dx and self._trains_gnn(plan))):
                return self._forward_rows(x, hidden, plan, flags, None, 0 if no_dx else (2 if self.rows_dx == "steps" else 1))
            if plan.learned_sel is None and plan.fold is None:
                return self._forward_fused(x, nodes, adj, weights, num_nodes, plan, flags)
            if no_dx:
                return self._forward_learned(x, hidden, plan, flags, None)
        # insert x at row num_nodes (after the overflow roll); fresh nodes/adj/weights buffers
        nodes, adj, weights, cur, num_nodes_next = _ops.state_advance(
            nodes, adj, weights, num_nodes, x, flags)
        if self.mutate_num_nodes_on_overflow:
            num_nodes.copy_(cur)          # == num_nodes unless the graph wrapped (gcm.py:354)

        # The returned `nodes` must stay clean (gcm.py:275-278): hand user modules a copy
        # because they may write in place; native selectors/GNN layers never mutate nodes.
        user_code = self.preprocessor is not None or self.positional_encoder is not None
        dirty_nodes = nodes.clone() if user_code else nodes

        for m in self._flag_users():      # selectors whose kernels raise flags write this module's word
            m._gcm_flags = flags
        if self.edge_selectors:
            adj, weights = self.edge_selectors(dirty_nodes, adj, weights, cur, B)
        if self.preprocessor:
            dirty_nodes = self.preprocessor(dirty_nodes)
        if self.aux_edge_selectors:
            seen = dirty_nodes
            if self.positional_encoder:
                seen = self.positional_encoder(dirty_nodes, cur)
            adj, weights = self.aux_edge_selectors(seen, adj, weights, cur, B)

        node_feats = self.gnn(dirty_nodes, adj, weights, B, N)
        if self.pooled:
            mx = node_feats
            if self.finite_check != "off":   # gcm.py:316-318 on the pooled output
                flags.bitwise_or_((~torch.isfinite(mx)).any().to(torch.int32) * _hip.FLAG_NONFINITE)
        else:
            mx = _ops.gather_rows(node_feats, cur, flags)
        if self.finite_check != "off":
            self._poll(flags)
        return mx, (nodes, adj, weights, num_nodes_next)

    def wrap_overflow(self, nodes, adj, weights, num_nodes):
        """gcm.py:323-355 as a standalone call: returns rolled copies (inputs untouched,
        unless mutate_num_nodes_on_overflow)."""
        B, N, F = nodes.shape
        full = num_nodes + 1 > N
        x = torch.zeros(B, F, device=nodes.device)
        flags = self._flag_word(nodes.device)
        n2, a2, w2, cur, _ = _ops.state_advance(nodes, adj, weights, num_nodes, x, flags)
        # undo the insert of the dummy x for graphs that did not wrap
        keep = (~full).view(B, 1, 1)
        n2 = torch.where(keep, nodes, n2)
        if self.mutate_num_nodes_on_overflow:
            num_nodes.copy_(cur)
        return n2, a2, w2, cur
