"""The table and the operand forms of tests/test_contract_cpu.py and tests/test_contract_gpu.py: HOW a conv layer of
gcm.nn is called - dtypes, shapes, devices, layouts - where every other test of these layers passes fresh, contiguous,
float32 / int64 tensors on the device.

The table: every entry of tests/_freeze.py's CASES (24 layer classes on two shapes each) through `Z.spec`, and one
small case each of RGCNConv, GENConv and EdgeConv, dense and sparse, built from their own case files.  Those three stay
in this file's table (`_OWN`): tests/_freeze.py's `_BUILDERS` decides what test_freeze_* runs.

A case is a namespace: id, layer (the class name), dense, product() -> a fresh CPU module, ops (the CPU operands by the
name of the forward's argument: x, adj | edge_index, rel, edge_weight, edge_type), grad (the operands that get a
gradient), g (the output's gradient) and z (the key of Z.spec / Z.reference, or None).

The forms: every awkward operand is `select(leaf)`, a view of a contiguous leaf that holds the canonical values inside
the view and zeros outside (`embed_*` -> (base, select)); `expected_grad` states the leaf's gradient: the canonical
gradient inside the view, exactly zero outside."""
import copy
import types

import torch

import _edgeconv_cases as EC
import _freeze as Z
import _gen_cases as GEC
import _rgcn_cases as RC

GRAD_NAMES = ("x", "adj", "edge_weight")

# (layer id, form) pairs held to the float64 bound of the restatement instead of bitwise equality with the canonical
# run, with the reason: {layer id: {form: reason}}.  The one rule for an entry: two CANONICAL runs of the layer differ
# from each other.  None does.  (GINConv, GENConv and a PNAConv with post_layers > 1 end in torch modules; the layers
# hand those the output's gradient contiguous - gcm/nn.py's _ready_grad - or a transposed / zero-stride g would take
# another path through torch's GEMMs and change the last bits of every gradient.)
FLOAT64_BOUND = {}


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
def _case(**kw):
    return types.SimpleNamespace(**kw)


def _z_case(family, dense, i):
    s = Z.spec(family, dense, i)
    return _case(id=Z.layer_id(family, dense, i), layer=Z.layer_id(family, dense), dense=dense, product=s.product,
                 ops={**s.inputs, **s.const}, grad=tuple(k for k in GRAD_NAMES if k in s.inputs), g=s.g,
                 z=(family, dense, i))


def _fixed(module):
    return lambda: copy.deepcopy(module)


def _rgcn(dense):
    """tests/_rgcn_cases.py: the weighted dense case (adj values of both signs, with a gradient) and the plain sparse
    one; parameters N(0, 0.5) as tests/test_rgcn_gpu.py sets them."""
    from gcm import nn as G
    gen = torch.Generator().manual_seed(9001 + dense)
    if dense:
        case = (2, 12, 4, 5, 3, {"weighted": True})
        B, N, Fi, Fo, R, opts = case
        o = RC.dense_operands(case)
        conv = G.DenseRGCNConv(Fi, Fo, R, **RC.layer_kwargs(opts))
        ops, grad = {"x": o["x"], "adj": o["adj"], "rel": o["rel"]}, ("x", "adj")
    else:
        case = (20, 60, 3, {})
        o = RC.sparse_operands(case)
        conv = G.RGCNConv(6, 5, case[2])
        ops, grad = {"x": o["x"], "edge_index": o["edge_index"], "edge_type": o["ids"]}, ("x",)
    with torch.no_grad():
        for p in conv.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.5)
    name = "DenseRGCNConv" if dense else "RGCNConv"
    return _case(id=name + "-0", layer=name, dense=dense, product=_fixed(conv), ops=ops, grad=grad, g=o["g"], z=None)


def _gen(dense):
    """tests/_gen_cases.py: in_channels != out_channels (lin_src and lin_dst exist), a learnt t, norm=None."""
    from gcm import nn as G
    if dense:
        c = GEC.dense_case(2, 40, 16, {"cin": 10})
        ops = {"x": c["x"], "adj": c["adj"]}
    else:
        c = GEC.csr_case(40, 90, 8, {"cin": 5})
        ops = {"x": c["x"], "edge_index": c["ei"]}
    ref = c["ref"]
    name = "DenseGENConv" if dense else "GENConv"
    conv = getattr(G, name)(ref.in_channels, ref.out_channels, t=ref.initial_t, learn_t=True, norm=None, bias=True)
    conv.load_state_dict(ref.state_dict())
    return _case(id=name + "-0", layer=name, dense=dense, product=_fixed(conv), ops=ops, grad=("x",), g=c["g"], z=None)


def _edge(dense):
    """tests/_edgeconv_cases.py: D1 (an empty row, a diagonal entry), S7 (duplicate and self edges, isolated nodes)."""
    from gcm import nn as G
    if dense:
        c = EC.dense_case("D1")
        ops = {"x": c["x"], "adj": c["adj"]}
    else:
        c = EC.csr_case(EC.CSR_EXTRA)
        ops = {"x": c["x"], "edge_index": c["ei"]}
    name = "DenseEdgeConv" if dense else "EdgeConv"
    conv = getattr(G, name)(copy.deepcopy(c["nn"]))
    return _case(id=name + "-0", layer=name, dense=dense, product=_fixed(conv), ops=ops, grad=("x",), g=c["g"], z=None)


_OWN = {"RGCNConv": _rgcn, "GENConv": _gen, "EdgeConv": _edge}

# (layer id, [case keys]): one parametrised test per layer class
LAYERS = [(Z.layer_id(f, d), [("z", f, d, 0), ("z", f, d, 1)]) for f, d in Z.LAYERS]
LAYERS += [(("Dense" if d else "") + f, [("own", f, d, 0)]) for f in _OWN for d in (True, False)]
LAYER_IDS = [lid for lid, _ in LAYERS]

_cases = {}


def case(key):
    if key not in _cases:
        kind, family, dense, i = key
        _cases[key] = _z_case(family, dense, i) if kind == "z" else _OWN[family](dense)
    return _cases[key]


def smallest(layer_id):
    """The smallest case of a layer class (the CPU tests run on it)."""
    return case(dict(LAYERS)[layer_id][0])


def mask_of(c):
    """A bool mask [B,N] for a dense case: about a third of the nodes off."""
    B, N = c.ops["x"].shape[:2]
    return torch.rand(B, N, generator=torch.Generator().manual_seed(4242 + B + N)) < 0.7


def call(mod, ops):
    """The forward with the operands by name, as the layers' own tests call it."""
    if "adj" in ops:
        args = [ops["x"], ops["adj"]] + ([ops["rel"]] if "rel" in ops else [])
        return mod(*args, mask=ops["mask"]) if ops.get("mask") is not None else mod(*args)
    return mod(ops["x"], ops["edge_index"], *[ops[k] for k in ("edge_weight", "edge_type") if k in ops])


# ---------------------------------------------------------------------------
# awkward views: (base, select) with select(base) equal to the value
# ---------------------------------------------------------------------------
def embed_columns(v):
    """v as wide[..., 2:2+F] of a buffer five columns wider."""
    F = v.shape[-1]
    base = torch.zeros(*v.shape[:-1], F + 5, dtype=v.dtype, device=v.device)
    base[..., 2:2 + F] = v

    def select(t):
        return t[..., 2:2 + F]
    return base, select


def embed_transposed(v):
    """v as vt.transpose(-1, -2)."""
    return v.transpose(-1, -2).contiguous(), lambda t: t.transpose(-1, -2)


def embed_offset(v):
    """v as flat[1:1+n].view(shape): contiguous, one element off the allocation (4-byte aligned for float32)."""
    n, shape = v.numel(), v.shape
    base = torch.zeros(n + 1, dtype=v.dtype, device=v.device)
    base[1:] = v.reshape(-1)
    return base, lambda t: t[1:1 + n].view(shape)


def embed_every_other(v):
    """v [E] as w2[::2]."""
    base = torch.zeros(2 * v.numel(), dtype=v.dtype, device=v.device)
    base[::2] = v
    return base, lambda t: t[::2]


def embed_pairs(ei):
    """edge_index as pairs.t() of an [E,2] list."""
    return ei.t().contiguous(), lambda t: t.t()


def embed_wide_index(ei):
    """edge_index as buf[:, 3:3+E] of a buffer seven edges wider."""
    E = ei.shape[1]
    base = torch.zeros(2, E + 7, dtype=ei.dtype, device=ei.device)
    base[:, 3:3 + E] = ei
    return base, lambda t: t[:, 3:3 + E]


def embed_expanded(v):
    """v [B,...] with equal batch entries as v[:1].expand(B, ...)."""
    B = v.shape[0]
    return v[:1].clone(), lambda t: t.expand(B, *t.shape[1:])


def expected_grad(base, select, canonical):
    """The gradient of the leaf `base`: the canonical gradient inside the view, zero outside (an expanded view: the
    sum over what it repeats, which is how autograd folds it)."""
    if select(base).shape != base.shape and select(base).numel() > base.numel():
        return canonical.reshape(select(base).shape).sum(0, keepdim=True)
    want = torch.zeros_like(base)
    select(want).copy_(canonical.reshape(select(base).shape))
    return want


def is_kernel_ready(t):
    return t.is_contiguous() and t.data_ptr() % 16 == 0
