"""k-nearest edge selector of the dense memory (not in the reference; its navigation model builds its graphs
with knn_graph / radius_graph(max_num_neighbors=k), models/nav_gcm.py).

The threshold selectors of distance.py connect the new node to EVERY stored node closer than a radius: the radius
is tuned per environment and the in-degree grows with the memory's fill level.  KNNEdge connects it to the k
nearest stored nodes of its own graph instead - a fixed in-degree (csrc/knn.hip: distances, ranks and the
adjacency row in one kernel)."""
import math

from .. import _hip
from .distance import Distance

_METRICS = {"l2": _hip.DIST_L2_PERGRAPH, "cosine": _hip.DIST_COSINE_SIM}


class KNNEdge(Distance):
    """Edge (n_b <- j) for the k nearest stored nodes j < n_b of the same graph (past graph_size: of the rows
    left after the overflow roll).

    metric "l2":     SpatialEdge's distance, || nodes[b, n_b, a_pose_slice] - nodes[b, j, b_pose_slice] ||; without
                     slices over all features, i.e. Euclidean kNN in feature space.
    metric "cosine": 1 - cosine similarity (CosineEdge's similarity: each side normalised by max(norm, 1e-8)), over
                     all features; pose slices are not accepted.

    The candidates are ranked by (distance, j): equal distances go to the LOWER index (the older node), a NaN
    distance is never selected.  The first min(k, n_b) are taken, and of those only the ones with distance <
    max_distance when a cap is given (None: no cap) - the in-degree is min(k, n_b) without a cap and never more
    with one.  distances() returns the ranked values; the selection is exactly their top-k.  bidirectional adds the
    reverse edges (j <- n_b).  A learned scale is not offered: scaling does not change a ranking.  1 <= k <= 255.

    Relation to the sparse twin: sparse_edge_selectors.SpatialKNNEdge(k) counts the new node itself among its k
    (at distance 0), so stepwise (tau = 1) it selects what the dense KNNEdge(k - 1) selects whenever fewer than k
    earlier nodes sit at distance 0 from the new one.

    A Distance: alone or in a selector Sequential with TemporalBackedge / DenseEdge it runs on the fused per-step
    kernels wherever SpatialEdge with the same arguments does (k travels in the descriptor's `mode`, see
    include/gcm_hip_knn.h)."""

    def __init__(self, k, a_pose_slice=None, b_pose_slice=None, max_distance=None, metric="l2", bidirectional=False):
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _hip.DIST_KNN_MAX:
            raise ValueError(f"KNNEdge: k must be an integer in 1..{_hip.DIST_KNN_MAX}, got {k!r}")
        if metric not in _METRICS:
            raise ValueError(f"KNNEdge: metric must be one of {sorted(_METRICS)}, got {metric!r}")
        if metric == "cosine" and (a_pose_slice is not None or b_pose_slice is not None):
            raise ValueError("KNNEdge: metric='cosine' runs over all features - pose slices are not accepted")
        if max_distance is not None and math.isnan(float(max_distance)):
            raise ValueError("KNNEdge: max_distance is NaN")
        super().__init__(math.inf if max_distance is None else float(max_distance), bidirectional=bidirectional)
        self.k = k
        self.metric = metric
        self.a_pose_slice = a_pose_slice
        self.b_pose_slice = b_pose_slice if b_pose_slice is not None else a_pose_slice

    @property
    def mode(self):
        """the metric in the low byte, k above it (include/gcm_hip_knn.h)"""
        return _METRICS[self.metric] | self.k << _hip.DIST_KNN_SHIFT

    def _slices(self, F):
        def rng(s):
            if s is None:
                return 0, F
            start, stop, step = s.indices(F)
            if step != 1:
                raise NotImplementedError("pose slices must be contiguous")
            return start, stop
        return rng(self.a_pose_slice), rng(self.b_pose_slice)

    def extra_repr(self):
        cap = "" if math.isinf(self.max_distance) else f", max_distance={self.max_distance}"
        return f"k={self.k}, metric={self.metric!r}{cap}, bidirectional={self.bidirectional}"
