"""CPU restatement of KNNEdge (gcm/edge_selectors/knn.py, include/gcm_hip_knn.h) in torch.
TEST INFRASTRUCTURE ONLY.

Candidates of graph b: the stored rows j < cur_b of the same graph.  Distance: per-graph L2 over the pose slices,
or 1 - cosine similarity (each side normalised by max(norm, 1e-8)).  Rank by (distance, j) ascending - equal
distances to the lower index, NaN behind everything and never selected - take the first min(k, cur), and of those
the ones with distance < max_distance when a cap is given (None: no cap)."""
import math

import torch


def distances(nodes, cur_rows, metric="l2", a=None, b=None, dtype=torch.float64):
    """[B, N] distance of every stored row to its graph's current row, evaluated in `dtype` (float64: the
    yardstick; float32: the restatement's own fp32 evaluation, for the error bound)."""
    x = nodes.to(dtype)
    c = cur_rows.to(dtype)
    if metric == "l2":
        a = slice(None) if a is None else a
        b = a if b is None else b
        diff = c[:, None, a] - x[:, :, b]
        return (diff * diff).sum(-1).sqrt()
    assert metric == "cosine" and a is None and b is None
    cn = c / c.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    xn = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-8)
    return 1.0 - (cn[:, None, :] * xn).sum(-1)


def topk_rows(dist, cur, k, max_distance=None):
    """[B, N] 0 / 1 selection of a [B, N] distance matrix: per graph the first min(k, cur_b) of the candidates j < cur_b
    in (distance, j) order by a STABLE sort (ties keep index order), NaN never, then the cap."""
    B, N = dist.shape
    out = torch.zeros(B, N)
    cap = math.inf if max_distance is None else float(max_distance)
    for g in range(B):
        n = int(cur[g])
        if n == 0:
            continue
        d = dist[g, :n].clone()
        nan = torch.isnan(d)
        d[nan] = math.inf                      # behind every number ...
        order = torch.sort(d, stable=True).indices.tolist()
        order = [j for j in order if not bool(nan[j])]   # ... and never selected
        for j in order[:k]:
            if math.isinf(cap) or float(dist[g, j]) < cap:
                out[g, j] = 1.0
    return out


class KNNSelector:
    """The restated selector with the dense plug-in signature (nodes, adj, weights, num_nodes, B) -> (adj, weights):
    drives the oracle's DenseGCM (oracle.dense.dense_step: nodes are the advanced state, num_nodes[b] the row of the
    current node).  Distances in float64 whatever the state's dtype."""

    def __init__(self, k, a_pose_slice=None, b_pose_slice=None, max_distance=None, metric="l2", bidirectional=False):
        self.k, self.a, self.b = k, a_pose_slice, b_pose_slice
        self.max_distance, self.metric, self.bidirectional = max_distance, metric, bidirectional

    def distances(self, nodes, num_nodes, dtype=torch.float64):
        B = nodes.shape[0]
        return distances(nodes, nodes[torch.arange(B), num_nodes], self.metric, self.a, self.b, dtype)

    def select(self, nodes, num_nodes):
        return topk_rows(self.distances(nodes, num_nodes), num_nodes, self.k, self.max_distance)

    def __call__(self, nodes, adj, weights, num_nodes, B):
        adj = adj.clone()
        sel = self.select(nodes.detach(), num_nodes)
        b_idx, j_idx = torch.nonzero(sel, as_tuple=True)
        adj[b_idx, num_nodes[b_idx], j_idx] = 1
        if self.bidirectional:
            adj[b_idx, j_idx, num_nodes[b_idx]] = 1
        return adj, weights
