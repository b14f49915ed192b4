"""The setups of tests/test_typed_edge_gpu.py, built on the CPU from a seed: the planes the TypedEdge selector is run
on alone, the typed memory end to end, and the memory with a LearnedEdge child.  tests/test_rgcn_cpu.py asserts the
preconditions (every relation used, two-bit entries, one-relation-empty rows, threshold and selection margins)."""
import copy
import functools

import torch

from _learned_det_restate import LearnedEdgeDet
from _reset_restate import reset_rollout
from _rgcn_restate import RGCNRef, TypedEdge
from oracle import dense as od

# ---- (a) the selector alone ------------------------------------------------------------------------------------
SPATIAL_R, COSINE_T = 0.9, 0.8
PLANES = {8: [5, 7, 2], 70: [69, 30, 3]}      # N -> the graphs' current rows (B = 3)
PLANE_F = 5


def oracle_children():
    return [od.TemporalBackedge([1, 3], "both"), od.SpatialEdge(SPATIAL_R, slice(0, 2)), od.CosineEdge(COSINE_T)]


def device_children():
    from gcm.edge_selectors.distance import CosineEdge, SpatialEdge
    from gcm.edge_selectors.temporal import TemporalBackedge
    return [TemporalBackedge([1, 3], "both"), SpatialEdge(SPATIAL_R, slice(0, 2)), CosineEdge(COSINE_T)]


def plane(N):
    """-> dict(nodes [3,N,F], adj, rel [3,N,N], cur [3]): a state with edges and codes already in it, bits above the
    selector's relations among them (they must come through untouched)."""
    torch.manual_seed(40 + N)
    cur = torch.tensor(PLANES[N])
    nodes = torch.randn(3, N, PLANE_F)
    nodes[..., :2] = torch.rand(3, N, 2) * 2.0
    adj = (torch.rand(3, N, N) < 0.2).float()
    rel = adj * torch.randint(1, 64, (3, N, N)).float()       # codes 1..63: relations 0-2 and the bits 3-5 above
    return {"nodes": nodes, "adj": adj, "rel": rel, "cur": cur}


def threshold_margin(nodes, cur):
    """The smallest distance of a candidate (j < n_b) of the spatial and the cosine child from its threshold."""
    _, spatial, cosine = oracle_children()
    live = torch.arange(nodes.shape[1])[None, :] < cur[:, None]
    out = []
    for sel in (spatial, cosine):
        d = sel.distances(nodes.double(), cur)
        out.append(float((d - sel.max_distance).abs()[live].min()) if bool(live.any()) else float("inf"))
    return min(out)


# ---- (b) the memory end to end ---------------------------------------------------------------------------------
B, N, F, H, T, R = 3, 8, 5, 6, 13, 3          # past the overflow roll of both planes
SEED = 7
RESET_AT = (6, 1)                             # the reset run: graph 1 is emptied before step 6


def memory_nets(seed=SEED):
    """-> (observations [T,B,F], the two layers' restatements), fp32 on the CPU."""
    torch.manual_seed(seed)
    obs = torch.rand(T, B, F)
    obs[..., :2] = torch.rand(T, B, 2) * 2.0
    layers = [RGCNRef(F, H, R), RGCNRef(H, H, R)]
    with torch.no_grad():
        for layer in layers:
            layer.weight.copy_(torch.randn_like(layer.weight) * 0.4)
            layer.root.copy_(torch.randn_like(layer.root) * 0.4)
            layer.bias.copy_(torch.randn_like(layer.bias) * 0.1)
    return obs, layers


def memory_children_oracle():
    return [od.TemporalBackedge([1, 3]), od.SpatialEdge(SPATIAL_R, slice(0, 2)), od.DenseEdge()]


def memory_children_device():
    from gcm.edge_selectors.dense import DenseEdge
    from gcm.edge_selectors.distance import SpatialEdge
    from gcm.edge_selectors.temporal import TemporalBackedge
    return [TemporalBackedge([1, 3]), SpatialEdge(SPATIAL_R, slice(0, 2)), DenseEdge()]


def _gnn_of(layers):
    def gnn(x, adj, w, B_, N_):
        return torch.tanh(layers[1](torch.tanh(layers[0](x, adj, w)), adj, w))
    return gnn


def _rollout(obs, layers, sel, dtype, reset):
    layers = [copy.deepcopy(layer).to(dtype) for layer in layers]
    obs = obs.to(dtype).requires_grad_(True)
    kw = dict(graph_size=N, edge_selectors=sel, edge_weights=True)
    if reset:
        mask = torch.zeros(T, B, dtype=torch.bool)
        mask[RESET_AT] = True
        out, hid = reset_rollout(obs, mask, None, _gnn_of(layers), **kw)
    else:
        out, hid = od.dense_rollout(obs, None, _gnn_of(layers), **kw)
    out.square().sum().backward()
    grads = {f"{i}.{k}": p.grad for i, layer in enumerate(layers) for k, p in layer.named_parameters()}
    grads["obs"] = obs.grad
    return out.detach(), tuple(h.detach() for h in hid), grads


@functools.lru_cache(maxsize=None)
def memory_reference(reset=False):
    """The restated typed memory in float64 and float32: (beliefs, final hidden, gradients) each; computed once and
    shared, never modified."""
    obs, layers = memory_nets()
    return tuple(_rollout(obs, layers, TypedEdge(memory_children_oracle()), dt, reset)
                 for dt in (torch.float64, torch.float32))


def memory_margin():
    """The smallest distance of a spatial candidate from the threshold over the float64 trajectory."""
    obs, _ = memory_nets()
    spatial = od.SpatialEdge(SPATIAL_R, slice(0, 2))
    margins = []

    class Watch:
        def __call__(self, nodes, adj, weights, num_nodes, B_):
            live = torch.arange(N)[None, :] < num_nodes[:, None]
            if bool(live.any()):
                margins.append(float((spatial.distances(nodes, num_nodes) - SPATIAL_R).abs()[live].min()))
            return adj, weights

    od.dense_rollout(obs.double(), None, lambda x, a, w, B_, N_: x, graph_size=N, edge_selectors=Watch(),
                     edge_weights=True)
    return min(margins)


# ---- (c) a LearnedEdge child: the adjacency's gradient -----------------------------------------------------------
LEARNED_SEED = 3
LOGIT_SCALE = 4.0                             # tests/test_learned_det_gpu.py: spreads the logits so the supports vary
LEARNED_R = 2


def learned_nets(seed=LEARNED_SEED):
    torch.manual_seed(seed)
    obs = torch.rand(T, B, F)
    layers = [RGCNRef(F, H, LEARNED_R), RGCNRef(H, H, LEARNED_R)]
    with torch.no_grad():
        for layer in layers:
            for p in layer.parameters():
                p.copy_(torch.randn_like(p) * 0.4)
    net = od.build_edge_network(F)
    with torch.no_grad():
        net[-1].weight.mul_(LOGIT_SCALE)
    return obs, layers, net


def _learned_rollout(dtype):
    obs, layers, net = learned_nets()
    layers = [copy.deepcopy(layer).to(dtype) for layer in layers]
    net = copy.deepcopy(net).to(dtype)
    obs = obs.to(dtype).requires_grad_(True)
    learned = LearnedEdgeDet(net)
    sel = TypedEdge([od.TemporalBackedge([1]), learned])
    out, hid = od.dense_rollout(obs, None, _gnn_of(layers), graph_size=N, edge_selectors=sel, edge_weights=True)
    out.square().sum().backward()
    grads = {f"{i}.{k}": p.grad for i, layer in enumerate(layers) for k, p in layer.named_parameters()}
    grads.update({"edge." + k: p.grad for k, p in net.named_parameters()})
    grads["obs"] = obs.grad
    return out.detach(), tuple(h.detach() for h in hid), grads, learned.margin


@functools.lru_cache(maxsize=None)
def learned_reference():
    return _learned_rollout(torch.float64), _learned_rollout(torch.float32)
