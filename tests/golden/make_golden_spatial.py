#!/usr/bin/env python3
"""Generate tests/golden/g17_sparse_spatial_*.npz by running the REFERENCE's sparse spatial selectors
(src/gcm/sparse_edge_selectors/spatial.py) and its SparseGCM with them.

Run:  python tests/golden/make_golden_spatial.py            (needs the reference source, like make_golden.py)

Placeholders as in make_golden.py (install_placeholders), plus the two names spatial.py needs:
  torch_geometric.transforms.delaunay.Delaunay   imported at spatial.py:8, never called (an empty class)
  torch_geometric.nn.knn(x, y, k)                 plain torch: for every row of y the k rows of x with the smallest
                                                  squared distance, ties to the lower index, as [y_idx; x_idx].
                                                  Like the other PyG stand-ins this boundary is "parity unpinned":
                                                  the fixtures use continuous random positions, so no pair is a
                                                  tie (checked below) and any exact kNN ranks them alike.
Positions are also kept at least 1e-5 away from every radius (checked below), so the fixtures do not depend on
how a distance is rounded.  kNN fixtures are one-shot only (T = 0): at T > 0 the reference's local sink index
is the bug DESIGN.md §3.13 describes.
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_placeholders, params_of, save  # noqa: E402


def knn(x, y, k, batch_x=None, batch_y=None, **kw):
    """torch_geometric.nn.knn stand-in -> [2, len(y) * min(k, len(x))] = [y_idx; x_idx]."""
    if x.shape[0] == 0 or y.shape[0] == 0:
        return torch.zeros(2, 0, dtype=torch.long)
    d = ((y[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    kk = min(int(k), x.shape[0])
    nbr = torch.sort(d, dim=1, stable=True).indices[:, :kk]
    y_idx = torch.arange(y.shape[0]).repeat_interleave(kk)
    return torch.stack([y_idx, nbr.reshape(-1)])


def install_spatial_placeholders():
    install_placeholders()
    tg = sys.modules["torch_geometric"]
    tg.nn.knn = knn
    tr = types.ModuleType("torch_geometric.transforms")
    dl = types.ModuleType("torch_geometric.transforms.delaunay")
    dl.Delaunay = type("Delaunay", (), {})
    tr.delaunay = dl
    tg.transforms = tr
    sys.modules["torch_geometric.transforms"] = tr
    sys.modules["torch_geometric.transforms.delaunay"] = dl


def spec_of(position_slice):
    """json form of a position slice (the tests rebuild it)"""
    if isinstance(position_slice, slice):
        return {"slice": [position_slice.start, position_slice.stop, position_slice.step]}
    return {"cols": list(position_slice)}


def graph_pairs_ok(nodes, n_of, cols, radius=None):
    """no two squared distances of a sink row within 1e-6 relative of each other (kNN ties) and no distance within
    1e-5 of the radius, over every pair of every graph (float64)"""
    for b, n in enumerate(n_of):
        pos = nodes[b, :n][:, cols].double()
        if n < 2:
            continue
        d2 = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1)
        off = ~torch.eye(n, dtype=torch.bool)
        if radius is not None and ((d2.sqrt() - radius).abs()[off] < 1e-5).any():
            return False
        for i in range(n):
            v = torch.sort(d2[i][off[i]]).values
            if v.numel() > 1 and ((v[1:] - v[:-1]) <= 1e-6 * v[1:].clamp_min(1e-12)).any():
                return False
    return True


def draw_positions(gen, B, N, F, n_of, cols, radius=None):
    for _ in range(100):
        nodes = torch.rand(B, N, F, generator=gen)
        if graph_pairs_ok(nodes, n_of, cols, radius):
            return nodes
    raise RuntimeError("no tie-free draw")


def main():
    assert os.path.isdir(REF), "golden vectors can only be generated where the reference source exists"
    install_spatial_placeholders()
    from oracle import sparse as osp
    from gcm.sparse_gcm import SparseGCM
    from gcm.sparse_edge_selectors.spatial import SpatialKNNEdge, SpatialRadiusEdge
    from gcm.sparse_edge_selectors.temporal import TemporalEdge

    def run_selector(name, sel, nodes, T, taus, meta):
        B = nodes.shape[0]
        adj = sel(nodes.clone(), T, taus, B).coalesce()
        save(name, meta, nodes=nodes, T=T, taus=taus, indices=adj.indices(), values=adj.values(),
             size=torch.tensor(list(adj.shape)))

    # ---- selector outputs at T = 0: ragged taus with 0 and 1 -------------------------------------------------
    gen = torch.Generator().manual_seed(17)
    B, N, F = 5, 12, 6
    T0 = torch.zeros(B, dtype=torch.long)
    taus = torch.tensor([5, 0, 1, 12, 7])
    n_of = (T0 + taus).tolist()
    radius = 0.45
    nodes = draw_positions(gen, B, N, F, n_of, list(range(F)), None)
    for ps in (slice(0, 2), slice(1, 4), slice(0, 6, 2), slice(-5, None, 2), [4, 1]):
        cols = list(range(F))[ps] if isinstance(ps, slice) else ps
        assert graph_pairs_ok(nodes, n_of, cols, radius), ps
    cases = [("knn_p2_k1", SpatialKNNEdge(slice(0, 2), 1), slice(0, 2), dict(k=1)),
             ("knn_p2_k3", SpatialKNNEdge(slice(0, 2), 3), slice(0, 2), dict(k=3)),
             ("knn_p2_k20", SpatialKNNEdge(slice(0, 2), 20), slice(0, 2), dict(k=20)),
             ("knn_p3_k3", SpatialKNNEdge(slice(1, 4), 3), slice(1, 4), dict(k=3)),
             ("knn_strided_k3", SpatialKNNEdge(slice(0, 6, 2), 3), slice(0, 6, 2), dict(k=3)),
             ("radius_p2", SpatialRadiusEdge(slice(0, 2), radius), slice(0, 2), dict(radius=radius, causal=True)),
             ("radius_p3", SpatialRadiusEdge(slice(1, 4), radius), slice(1, 4), dict(radius=radius, causal=True)),
             ("radius_strided", SpatialRadiusEdge(slice(-5, None, 2), radius), slice(-5, None, 2),
              dict(radius=radius, causal=True)),
             ("radius_cols", SpatialRadiusEdge([4, 1], radius), [4, 1], dict(radius=radius, causal=True)),
             ("radius_noncausal", SpatialRadiusEdge(slice(0, 2), radius, causal=False), slice(0, 2),
              dict(radius=radius, causal=False))]
    for tag, sel, ps, extra in cases:
        kind = "knn" if tag.startswith("knn") else "radius"
        run_selector("g17_sparse_spatial_" + tag, sel, nodes, T0, taus,
                     dict(kind=kind, pos=spec_of(ps), **extra))

    # ---- radius at T > 0 (the reference is right there), graphs with tau = 0 and T + tau <= 1 ----------------
    T1 = torch.tensor([3, 0, 5, 1, 4, 0])
    taus1 = torch.tensor([4, 2, 0, 0, 8, 1])
    n_of = (T1 + taus1).tolist()
    nodes = draw_positions(gen, 6, N, F, n_of, [0, 1], radius)
    for causal in (True, False):
        tag = "radius_t_causal" if causal else "radius_t_noncausal"
        run_selector("g17_sparse_spatial_" + tag, SpatialRadiusEdge(slice(0, 2), radius, causal=causal), nodes, T1,
                     taus1, dict(kind="radius", pos=spec_of(slice(0, 2)), radius=radius, causal=causal))

    # ---- SparseGCM end to end (run_sparse of make_golden.py with spatial selectors) ----------------------------
    def run_sparse(name, B, N, F, H, obs, tau_plan, main, aux, meta):
        torch.manual_seed(0)
        gnn = osp.canonical_gnn(F, H, act=torch.nn.Tanh)
        m = SparseGCM(gnn, edge_selectors=main, aux_edge_selectors=aux, graph_size=N)
        obs = obs.clone().requires_grad_(True)
        hidden, outs, pos = None, [], torch.zeros(B, dtype=torch.long)
        for taus in tau_plan:
            t = int(taus.max())
            x = torch.zeros(B, t, F)
            for b in range(B):
                x[b, : taus[b]] = obs[b, pos[b]: pos[b] + taus[b]]
            out, hidden = m(x, taus, hidden)
            outs.append(out)
            pos = pos + taus
        loss = sum(o.sum() for o in outs) / sum(o.numel() for o in outs)
        loss.backward()
        arrays = dict(obs=obs.detach(), grad_obs=obs.grad, taus=torch.stack(tau_plan),
                      hT_nodes=hidden[0], hT_adj_indices=hidden[1].coalesce().indices(),
                      hT_adj_values=hidden[1].coalesce().values().detach(), hT_T=hidden[2])
        for i, o in enumerate(outs):
            arrays[f"out{i}"] = o
        arrays.update(params_of(gnn))
        for k, p in gnn.named_parameters():
            arrays["grad:" + k] = p.grad.clone()
        save(name, dict(B=B, N=N, F=F, H=H, **meta), **arrays)

    B, N, F, H, ts = 4, 16, 4, 8, 12
    r = 0.35
    tlen = torch.tensor([12, 7, 1, 10])
    obs = draw_positions(gen, B, ts, F, tlen.tolist(), [0, 1], r)
    ps = slice(0, 2)
    run_sparse("g17_sparse_spatial_gcm_knn", B, N, F, H, obs, [tlen], SpatialKNNEdge(ps, 3), TemporalEdge([1]),
               dict(main=dict(kind="knn", k=3, pos=spec_of(ps)), aux=dict(kind="temporal", hops=[1])))
    run_sparse("g17_sparse_spatial_gcm_radius", B, N, F, H, obs, [tlen], SpatialRadiusEdge(ps, r),
               TemporalEdge([1]),
               dict(main=dict(kind="radius", radius=r, causal=True, pos=spec_of(ps)),
                    aux=dict(kind="temporal", hops=[1])))
    full = torch.full((B,), ts, dtype=torch.long)
    obs_s = draw_positions(gen, B, ts, F, full.tolist(), [0, 1], r)
    run_sparse("g17_sparse_spatial_gcm_radius_stepwise", B, N, F, H, obs_s, [torch.ones(B, dtype=torch.long)] * ts,
               SpatialRadiusEdge(ps, r), TemporalEdge([1]),
               dict(main=dict(kind="radius", radius=r, causal=True, pos=spec_of(ps)),
                    aux=dict(kind="temporal", hops=[1])))
    # the other way round: TemporalEdge as the main selector, the spatial one as aux (ragged calls, T > 0)
    plan = [torch.tensor([3, 1, 4, 2]), torch.tensor([5, 5, 1, 3]), torch.tensor([4, 2, 7, 1])]
    run_sparse("g17_sparse_spatial_gcm_aux_radius", B, N, F, H, obs_s, plan, TemporalEdge([1]),
               SpatialRadiusEdge(ps, r),
               dict(main=dict(kind="temporal", hops=[1]),
                    aux=dict(kind="radius", radius=r, causal=True, pos=spec_of(ps))))


if __name__ == "__main__":
    main()
