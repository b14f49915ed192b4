"""gcm.nn.MessagePassing: torch_geometric.nn.MessagePassing's contract, in the subset real layers use, on the
project's device index (GraphIndex) and the HIP gather / segment kernels of csrc/message_passing.hip.  A layer written
by subclassing PyG's base class runs by changing its import; the hand-fused layers of gcm.nn stay the
fast path - this one materialises [E, C] messages, as PyG does."""
import inspect

import torch

from . import _hip, _ops
from .graph_utils import scatter

_AGGRS = ("add", "sum", "mean", "max", "min")
_SPECIAL = ("edge_index", "edge_index_i", "edge_index_j", "index", "ptr", "size", "size_i", "size_j", "dim_size")


def _signature(fn, skip_first):
    """The parameters `propagate` fills of message / aggregate / update: name -> inspect.Parameter."""
    params = [p for p in inspect.signature(fn).parameters.values()
              if p.kind in (p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY)]
    return {p.name: p for p in (params[1:] if skip_first else params)}


class MessagePassing(torch.nn.Module):
    """out = update(aggregate(message(...))) over the edges of `edge_index` [2, E] int64 (source, sink).

    aggr: "add" / "sum", "mean", "max", "min", or None (the subclass overrides `aggregate`).  A node without an
    in-edge aggregates 0; "mean" divides by max(count, 1); duplicate edges are separate terms and a loop is an ordinary
    edge.  The gradient of "max" / "min" goes to ONE edge, the earliest of its sink in the caller's order on a tie.
    node_dim: -2 (every gathered tensor is [M, C]) or 0 (any rank >= 1, gathered along dim 0: the [M, H, C] form).

    `propagate` collects the arguments of message, aggregate and update from their signatures by PyG's rules: `name_j`
    / `name_i` is kwargs[name] gathered by source / sink (a (src, dst) pair gives element 0 to _j and 1 to _i);
    edge_index, edge_index_i, edge_index_j, index (the sink of each edge), ptr (None), size, size_i, size_j and
    dim_size are provided; every other name is kwargs[name] as given, in the caller's edge order.  float32 tensors are
    gathered by the kernels and carry gradients; other dtypes by plain indexing, without one.

    Not implemented: flow="target_to_source", bipartite sizes, SparseTensor inputs, aggregation modules and lists,
    message_and_aggregate, edge_updater, hooks, explain, decomposed_layers, jittable."""

    def __init__(self, aggr="add", *, flow="source_to_target", node_dim=-2, **kwargs):
        super().__init__()
        if kwargs:                              # aggr_kwargs, decomposed_layers, ...
            raise NotImplementedError(f"MessagePassing({next(iter(kwargs))}=...) is not implemented")
        if aggr is not None and (not isinstance(aggr, str) or aggr not in _AGGRS):
            raise NotImplementedError(f"aggr={aggr!r} is not implemented: one of {_AGGRS} or None (aggregation "
                                      "modules and lists of aggregations are not)")
        if flow != "source_to_target":
            raise NotImplementedError(f"flow='{flow}' is not implemented: 'source_to_target' only")
        if node_dim not in (0, -2):
            raise NotImplementedError(f"node_dim={node_dim} is not implemented: 0 or -2")
        self.aggr, self.flow, self.node_dim = aggr, flow, node_dim
        self._mp_params = (_signature(self.message, False), _signature(self.aggregate, True),
                           _signature(self.update, True))

    def reset_parameters(self):
        pass

    # ---- the three stages a subclass overrides -----------------------------------------------------
    def message(self, x_j):
        return x_j

    def aggregate(self, inputs, index, ptr=None, dim_size=None):
        if self.aggr is None:
            raise NotImplementedError("aggr=None: the subclass overrides aggregate()")
        return scatter(inputs, index, dim=0, dim_size=dim_size, reduce=self.aggr)

    def update(self, inputs):
        return inputs

    def edge_updater(self, edge_index, size=None, **kwargs):
        raise NotImplementedError("edge_updater / edge_update are not implemented")

    # ---- propagate -----------------------------------------------------------------------------
    def _check_rows(self, t, M):
        if self.node_dim == -2 and t.dim() != 2:
            raise ValueError(f"node_dim=-2 gathers [M, C] tensors; got {list(t.shape)} (use node_dim=0)")
        if t.dim() < 1:
            raise ValueError("a gathered tensor needs at least one dimension")
        if M is not None and t.shape[0] != M:
            raise ValueError(f"encountered a tensor with {t.shape[0]} rows along the node dimension, expected {M}")
        return t.shape[0]

    def _graph(self, edge_index, M):
        """The index SparseGCM attached (`edge_index.gcm_graph`) when it fits, else one built here on the device."""
        graph = getattr(edge_index, "gcm_graph", None)
        if graph is None or graph.M != M or graph.E != edge_index.shape[1]:
            _hip.on_device(edge_index)
            graph = _ops.GraphIndex.from_edge_index(edge_index, M)
        if graph.mask is not None:
            raise ValueError(f"{self.__class__.__name__} does not take a masked GraphIndex (k-hop subgraphs reach it "
                             "relabelled)")
        return graph

    def propagate(self, edge_index, size=None, **kwargs):
        if not isinstance(edge_index, torch.Tensor) or edge_index.layout != torch.strided:
            raise NotImplementedError("propagate takes edge_index as a [2, E] int64 tensor (SparseTensor / sparse "
                                      "adjacency inputs are not implemented)")
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise ValueError(f"edge_index must be [2, E] int64; got {list(edge_index.shape)} {edge_index.dtype}")
        M = None
        if size is not None:
            if len(size) != 2:
                raise ValueError("size must be None or (M, M)")
            if size[0] is not None and size[1] is not None and size[0] != size[1]:
                raise NotImplementedError(f"bipartite propagation (size={tuple(size)}) is not implemented")
            M = size[0] if size[0] is not None else size[1]
        wanted = {name: p for params in self._mp_params for name, p in params.items()}

        # what is gathered, by which row of edge_index: name -> (tensor, 0 source | 1 sink)
        gathers = {}
        for name in wanted:
            if name in _SPECIAL or name[-2:] not in ("_i", "_j") or name[:-2] not in kwargs:
                continue
            side = 0 if name.endswith("_j") else 1
            data = kwargs[name[:-2]]
            if isinstance(data, (tuple, list)):
                if len(data) != 2:
                    raise ValueError(f"{name[:-2]}: a (src, dst) pair has two elements")
                if data[1] is not None and isinstance(data[0], torch.Tensor) and isinstance(data[1], torch.Tensor) \
                        and data[0].shape[0] != data[1].shape[0]:
                    raise NotImplementedError(f"{name[:-2]}: bipartite (src, dst) pairs are not implemented")
                data = data[side]
            if isinstance(data, torch.Tensor):
                M = self._check_rows(data, M)
            gathers[name] = (data, side)
        if M is None:
            raise ValueError("propagate needs size=(M, M) when no tensor is gathered")

        device_call = edge_index.is_cuda
        for data, _ in gathers.values():
            if isinstance(data, torch.Tensor) and data.dtype == torch.float32:
                _hip.on_device(data.contiguous())       # a CPU tensor fails here, before the index is built
                device_call = True
        graph = self._graph(edge_index, M) if device_call else None

        index = edge_index[1]
        if graph is not None:
            index.gcm_graph = graph         # how softmax / scatter find the CSR without a sort (graph_utils.py)
        coll = {"edge_index": edge_index, "edge_index_i": index, "edge_index_j": edge_index[0], "index": index,
                "ptr": None, "size": (M, M), "size_i": M, "size_j": M, "dim_size": M}
        for name, (data, side) in gathers.items():
            if isinstance(data, torch.Tensor):
                if data.dtype == torch.float32:
                    seg = _ops.Segments.by_sink(graph) if side else _ops.Segments.by_source(graph)
                    data = _ops.mp_gather(data, seg)
                else:
                    data = data.detach().index_select(0, edge_index[side])
            coll[name] = data
        for name in wanted:
            if name not in coll and name in kwargs:
                coll[name] = kwargs[name]

        def args_of(params):
            out = {}
            for name, p in params.items():
                if name in coll:
                    out[name] = coll[name]
                elif p.default is inspect.Parameter.empty:
                    raise TypeError(f"{self.__class__.__name__}.propagate: required argument '{name}' is missing "
                                    f"(pass {name[:-2] if name[-2:] in ('_i', '_j') else name}=...)")
            return out

        msg_params, aggr_params, update_params = self._mp_params
        out = self.message(**args_of(msg_params))
        out = self.aggregate(out, **args_of(aggr_params))
        return self.update(out, **args_of(update_params))

    def __repr__(self):
        if hasattr(self, "in_channels") and hasattr(self, "out_channels"):
            return f"{self.__class__.__name__}({self.in_channels}, {self.out_channels})"
        return f"{self.__class__.__name__}()"
