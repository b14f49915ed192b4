"""gcm.edge_selectors.typed.TypedEdge: alone against its restatement (exact), inside DenseGCM(edge_weights=True) with
two DenseRGCNConv layers against oracle.dense.dense_rollout over the restated selector and layers, and with a
LearnedEdge child, whose edge network is reached only through the layer's adjacency gradient.  The setups and their
preconditions are tests/_typed_cases.py's (asserted in tests/test_rgcn_cpu.py).  Needs an MI355X."""
import pytest
import torch

import _typed_cases as C
from _gcn_restate import assert_bounded
from _rgcn_restate import TypedEdge as TypedEdgeRef

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_FLOOR = 5e-7


def _typed(children, relations=None):
    from gcm.edge_selectors.typed import TypedEdge
    return TypedEdge(children, relations).to(DEV)


# ---- (a) the selector alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("relations", [None, [0, 0, 1]], ids=["own", "shared"])
@pytest.mark.parametrize("N", sorted(C.PLANES))
def test_selector_is_exact(N, relations):
    p = C.plane(N)
    adj_ref, rel_ref = TypedEdgeRef(C.oracle_children(), relations)(p["nodes"], p["adj"], p["rel"], p["cur"], 3)
    sel = _typed(C.device_children(), relations)
    assert sel.num_relations == (3 if relations is None else 2)
    adj_in, rel_in = p["adj"].to(DEV), p["rel"].to(DEV)
    adj, rel = sel(p["nodes"].to(DEV), adj_in, rel_in, p["cur"].to(DEV), 3)
    assert torch.equal(adj.cpu(), adj_ref) and torch.equal(rel.cpu(), rel_ref)
    assert torch.equal(adj_in.cpu(), p["adj"]) and torch.equal(rel_in.cpu(), p["rel"])      # the inputs are untouched
    keep = ~((1 << sel.num_relations) - 1)                                                  # the rest of the codes
    assert torch.equal(rel.cpu().long() & keep, p["rel"].long() & keep)
    assert bool(((rel.cpu().long() & ~keep) != (p["rel"].long() & ~keep)).any())            # and something was added


def test_selector_under_autograd_takes_the_torch_merge():
    """An adjacency that requires a gradient: adj_out is util.diff_or - same values, and the gradient of diff_or."""
    p = C.plane(8)
    sel = _typed(C.device_children())
    adj_in = p["adj"].to(DEV).requires_grad_()
    adj, rel = sel(p["nodes"].to(DEV), adj_in, p["rel"].to(DEV), p["cur"].to(DEV), 3)
    adj_ref, rel_ref = TypedEdgeRef(C.oracle_children())(p["nodes"], p["adj"].clone().requires_grad_(), p["rel"],
                                                         p["cur"], 3)
    assert torch.equal(adj.detach().cpu(), adj_ref.detach()) and torch.equal(rel.cpu(), rel_ref)
    assert adj.requires_grad and not rel.requires_grad
    adj.sum().backward()
    picked = sum(s(p["nodes"], torch.zeros_like(p["adj"]), torch.zeros(0), p["cur"], 3)[0] for s in C.oracle_children())
    assert torch.equal(adj_in.grad.cpu(), (picked == 0).float())    # d diff_or / d adj = prod (1 - a_k)


def test_selector_refuses_a_wrong_weights_shape():
    p = C.plane(8)
    sel = _typed(C.device_children())
    with pytest.raises(ValueError, match="edge_weights=True"):
        sel(p["nodes"].to(DEV), p["adj"].to(DEV), torch.zeros(0, device=DEV), p["cur"].to(DEV), 3)


# ---- (b) the memory end to end ---------------------------------------------------------------------------------
def _device_memory(children, layers_ref):
    from gcm import nn as G
    from gcm.gcm import DenseGCM
    sel = _typed(children)
    Fi, Hh = layers_ref[0].weight.shape[1], layers_ref[0].weight.shape[2]
    convs = [G.DenseRGCNConv(Fi, Hh, sel.num_relations), G.DenseRGCNConv(Hh, Hh, sel.num_relations)]
    for conv, ref in zip(convs, layers_ref):
        conv.load_state_dict(ref.state_dict())
    gnn = G.Sequential("x, adj, weights, B, N", [
        (convs[0], "x, adj, weights -> x"), torch.nn.Tanh(),
        (convs[1], "x, adj, weights -> x"), torch.nn.Tanh()]).to(DEV)
    return DenseGCM(gnn, edge_selectors=sel, graph_size=C.N, edge_weights=True), convs, sel


def _steps(mem, obs, reset=None):
    hidden, outs = None, []
    for t in range(obs.shape[0]):
        if reset is not None and t == reset[0]:
            mask = torch.zeros(obs.shape[1], dtype=torch.bool)
            mask[reset[1]] = True
            hidden = mem.reset_hidden(hidden, mask)
        mx, hidden = mem(obs[t], hidden)
        outs.append(mx)
    return torch.stack(outs), hidden


# Sparsemax does not change when every logit moves by the same amount, so the gradients of the two parameters that
# only shift the logits - the last LayerNorm's bias and the last Linear's bias of the default edge network - are
# exactly zero; float64 gives 1e-16 for them, rounding noise whose own magnitude is no scale.  They are held to 5e-7 of
# the largest gradient of the edge network instead (the same floor, on the scale of the sums they are the residue of).
SHIFT_ONLY = ("edge.5.bias", "edge.6.bias")


def _check_memory(out, hid, got, ref64, ref32):
    (o64, h64, g64), (o32, h32, g32) = ref64[:3], ref32[:3]
    g64, g32, got = dict(g64), dict(g32), dict(got)
    if SHIFT_ONLY[0] in g64:
        edge_scale = max(float(v.abs().max()) for k, v in g64.items() if k.startswith("edge."))
        for k in SHIFT_ONLY:
            assert float(g64.pop(k).abs().max()) <= 1e-12
            g32.pop(k)
            assert float(got.pop(k).abs().max()) <= GRAD_FLOOR * edge_scale, k
    assert_bounded(out, o64, o32, "beliefs")
    assert_bounded(hid[0], h64[0], h32[0], "nodes")
    assert torch.equal(hid[1].detach().cpu().double(), h64[1]), "adjacency must be exact"
    assert torch.equal(hid[2].detach().cpu().double(), h64[2]), "relation plane must be exact"
    assert torch.equal(hid[3].cpu(), h64[3])
    assert set(got) == set(g64)
    for k in g64:
        assert got[k] is not None, k
        assert_bounded(got[k], g64[k], g32[k], "grad " + k, floor=GRAD_FLOOR, relative=True)


@pytest.mark.parametrize("how", ["steps", "rollout", "steps_reset"])
def test_typed_memory_matches_the_oracle(how):
    reset = how == "steps_reset"
    ref64, ref32 = C.memory_reference(reset)
    obs, layers = C.memory_nets()
    mem, convs, _ = _device_memory(C.memory_children_device(), layers)
    obs = obs.to(DEV).requires_grad_(True)
    if how == "rollout":
        out, hid = mem.rollout(obs)
    else:
        out, hid = _steps(mem, obs, C.RESET_AT if reset else None)
    out.square().sum().backward()
    mem.check_flags()
    got = {f"{i}.{k}": p.grad for i, conv in enumerate(convs) for k, p in conv.named_parameters()}
    got["obs"] = obs.grad
    _check_memory(out, hid, got, ref64, ref32)


# ---- (c) a LearnedEdge child -----------------------------------------------------------------------------------
def test_learned_child_trains_through_the_layers_adjacency_gradient():
    from gcm.edge_selectors.learned import LearnedEdge
    from gcm.edge_selectors.temporal import TemporalBackedge
    ref64, ref32 = C.learned_reference()
    obs, layers, net = C.learned_nets()
    learned = LearnedEdge(C.F, deterministic=True)
    learned.edge_network.load_state_dict(net.state_dict())
    mem, convs, sel = _device_memory([TemporalBackedge([1]), learned], layers)
    obs = obs.to(DEV).requires_grad_(True)
    out, hid = _steps(mem, obs)
    out.square().sum().backward()
    mem.check_flags()
    assert hid[1].requires_grad and not hid[2].requires_grad
    got = {f"{i}.{k}": p.grad for i, conv in enumerate(convs) for k, p in conv.named_parameters()}
    got.update({"edge." + k: p.grad for k, p in learned.edge_network.named_parameters()})
    got["obs"] = obs.grad
    _check_memory(out, hid, got, ref64, ref32)
