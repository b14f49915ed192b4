"""The calling contract of the conv layers of gcm.nn on the device: ACCEPTED operands only (every rejection - a wrong
dtype, a wrong shape, a host tensor - is tested in tests/test_contract_cpu.py, on the CPU, because on a device those
are the calls that fault it).  One parametrised test per layer class of tests/_contract.py's table.

Canonical run: the layer as its own tests call it - fresh, contiguous operands - forward and backward with the case's
g.  For the cases of tests/_freeze.py the output and every gradient are held to the float64 restatement exactly as
tests/test_freeze_conv_gpu.py holds them (3x the restatement's own float32 distance, floors 2e-6 / 5e-7); for RGCN,
GEN and EdgeConv the canonical run is the comparand only (their own tests hold the float64 bound).  Two canonical runs
must agree bitwise.

Awkward forms: the same values again as
  dense:  x as a column slice of a wider buffer; x and adj as transposes; adj[:1].expand(B, ..) (canonical: the same
          adjacency repeated); 2-D x and adj (canonical: the batch of one); a bool mask as maskT.t() (canonical: the
          mask contiguous); x one element off its allocation (contiguous, 4-byte aligned);
  sparse: edge_index as pairs.t() of an [E,2] list and as a slice of a wider buffer; x as a column slice; edge_weight
          as w2[::2]; x and edge_weight one element off their allocation;
  both:   backward with g transposed in memory, and with g = ones(1).expand_as(out), the strides of
          out.sum().backward() (canonical: contiguous ones).
The output, every parameter's gradient and every operand's gradient must be torch.equal to the canonical run's: the
host code copies the operand and launches the same kernels on the same numbers, and the conv kernels hold no floating
atomics, so the tolerance is zero by construction, not by measurement.  Every awkward operand is a view of a contiguous
leaf: the leaf's gradient is the canonical one inside the view and exactly zero outside.  tests/_contract.py's
FLOAT64_BOUND lists the (layer, form) pairs held to the float64 bound instead, with the reason.  Needs an MI355X."""
import pytest
import torch

import _contract as C
import _freeze as Z
from _gcn_restate import assert_bounded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _identity(v):
    """The 2-D operand of a dense layer for a batch of one: the leaf itself (what is awkward is its rank)."""
    return v[0].clone(), lambda t: t


def _run(conv, ops, leaves, g_of):
    """Forward and backward -> (out, {operand: the leaf's gradient}, {parameter: gradient})."""
    conv.zero_grad(set_to_none=True)
    out = C.call(conv, ops)
    out.backward(g_of(out))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return out.detach(), {k: t.grad for k, t in leaves.items()}, {k: p.grad for k, p in conv.named_parameters()}


def _canonical(conv, c, values, g):
    ops = {k: (v.clone().requires_grad_() if k in c.grad else v) for k, v in values.items()}
    return _run(conv, ops, {k: ops[k] for k in c.grad}, lambda out: g.view_as(out))


def _variants(c, values, g):
    """The canonical comparands: {key: (operand values, g)}."""
    out = {"plain": (values, g), "ones": (values, torch.ones_like(g))}
    if c.dense:
        B = values["x"].shape[0]
        planes = [k for k in ("adj", "rel") if k in values]
        out["mask"] = ({**values, "mask": C.mask_of(c).to(DEV)}, g)
        out["bcast"] = ({**values, **{k: values[k][:1].repeat(B, 1, 1) for k in planes}}, g)
        out["b1"] = ({k: v[:1].clone() for k, v in values.items()}, g[:1].clone())
    return out


def _forms(c):
    """(name, canonical variant, {operand: embed}, how g is laid out)."""
    if c.dense:
        planes = [k for k in ("adj", "rel") if k in c.ops]
        forms = [("x-columns", "plain", {"x": C.embed_columns}, None),
                 ("x-transposed", "plain", {"x": C.embed_transposed}, None),
                 ("adj-transposed", "plain", {"adj": C.embed_transposed}, None),
                 ("adj-expanded", "bcast", {k: C.embed_expanded for k in planes}, None),
                 ("2d", "b1", {k: _identity for k in ["x"] + planes}, None),
                 ("mask-transposed", "mask", {"mask": C.embed_transposed}, None),
                 ("x-offset", "plain", {"x": C.embed_offset}, None)]
    else:
        forms = [("edge_index-pairs", "plain", {"edge_index": C.embed_pairs}, None),
                 ("edge_index-wide", "plain", {"edge_index": C.embed_wide_index}, None),
                 ("x-columns", "plain", {"x": C.embed_columns}, None),
                 ("x-offset", "plain", {"x": C.embed_offset}, None)]
        if "edge_weight" in c.ops:
            forms += [("edge_weight-every-other", "plain", {"edge_weight": C.embed_every_other}, None),
                      ("edge_weight-offset", "plain", {"edge_weight": C.embed_offset}, None)]
    return forms + [("g-transposed", "plain", {}, "transposed"), ("g-ones-expanded", "ones", {}, "expanded")]


def _awkward(conv, c, values, g, embeds, g_layout):
    ops, leaves, views = {}, {}, {}
    for k, v in values.items():
        if k in embeds:
            base, select = embeds[k](v)
            if k in c.grad:
                base.requires_grad_()
            ops[k] = select(base)
            assert torch.equal(ops[k].detach().reshape(v.shape), v), "the form changed the values"
            assert embeds[k] is _identity or not C.is_kernel_ready(ops[k]), "the form is not awkward"
            if embeds[k] is C.embed_offset:
                assert ops[k].is_contiguous() and ops[k].data_ptr() % 16 == 4
            views[k] = (base, select)
        else:
            ops[k] = v.clone().requires_grad_() if k in c.grad else v
        if k in c.grad:
            leaves[k] = base if k in embeds else ops[k]

    def g_of(out):
        gv = g.view_as(out)
        if g_layout == "transposed":
            base, select = C.embed_transposed(gv)
            gv = select(base)
            assert not gv.is_contiguous()
        elif g_layout == "expanded":
            gv = torch.ones(1, device=out.device).expand_as(out)
            assert set(gv.stride()) == {0}
        return gv
    out, grads, pgrads = _run(conv, ops, leaves, g_of)
    return out, grads, pgrads, views


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a.reshape(b.shape), b))


def _compare(tag, c, got, want, views, failures):
    """An awkward run against its canonical comparand, bitwise."""
    out, grads, pgrads = got
    w_out, w_grads, w_pgrads = want
    if not _same(out, w_out):
        failures.append("%s: the output differs (max %.3e)"
                        % (tag, float((out.reshape(w_out.shape) - w_out).abs().max())))
    for k, wg in w_pgrads.items():
        if not _same(pgrads[k], wg):
            failures.append("%s: the gradient of parameter %s differs" % (tag, k))
    for k, wg in w_grads.items():
        gg = grads[k]
        if k in views and wg is not None:
            base, select = views[k]
            wg = C.expected_grad(base.detach(), select, wg)
        if not _same(gg, wg):
            failures.append("%s: the gradient of %s differs from the canonical one inside its view, or is not zero "
                            "outside" % (tag, k))


def _hold_to_float64(tag, c, run):
    """A run on the operands of a tests/_freeze.py case against the float64 restatement, as test_freeze_conv_gpu.py."""
    s = Z.spec(*c.z)
    ref = Z.reference(*c.z, tuple(s.names))
    (o64, g64), (o32, g32) = ref[torch.float64], ref[torch.float32]
    out, grads, pgrads = run
    assert out.shape == o64.shape, tag
    assert_bounded(out, o64, o32, tag + " out")
    got = {**grads, **pgrads}
    for name in g64:
        assert got[name] is not None, tag + ": %s got no gradient" % name
        assert bool(torch.isfinite(got[name]).all()), tag + " " + name
        assert_bounded(got[name].reshape(g64[name].shape), g64[name], g32[name], tag + " " + name, floor=Z.GRAD_FLOOR,
                       relative=True)


@pytest.mark.parametrize("lid,keys", C.LAYERS, ids=C.LAYER_IDS)
def test_every_accepted_form_is_the_canonical_run(lid, keys):
    failures, ran = [], []
    for key in keys:
        c = C.case(key)
        conv = c.product().to(DEV)
        values = {k: v.to(DEV) for k, v in c.ops.items()}
        g = c.g.to(DEV)
        variants = _variants(c, values, g)
        canon = {}
        for name, variant, embeds, g_layout in _forms(c):
            tag = "%s [%s]" % (c.id, name)
            v_values, v_g = variants[variant]
            if variant not in canon:
                canon[variant] = _canonical(conv, c, v_values, v_g)
                if variant == "plain":
                    again = _canonical(conv, c, v_values, v_g)
                    _compare(c.id + " [a second canonical run]", c, again, canon[variant], {}, failures)
                    if c.z is not None:
                        _hold_to_float64(c.id, c, canon[variant])
            *got, views = _awkward(conv, c, v_values, v_g, embeds, g_layout)
            if name in C.FLOAT64_BOUND.get(lid, {}):
                assert c.z is not None and variant == "plain", "the float64 bound needs the restatement's own operands"
                folded = {k: (views[k][1](t) if k in views and t is not None else t) for k, t in got[1].items()}
                _hold_to_float64(tag, c, (got[0], folded, got[2]))
            else:
                _compare(tag, c, got, canon[variant], views, failures)
            ran.append(tag)
    print("\nCONTRACT %s: %d awkward runs, %d differ from their canonical run" % (lid, len(ran), len(failures)))
    assert not failures, "\n".join(failures)


def test_an_awkward_g_reaches_the_aggregations_of_gin_and_gen():
    """GINConv and GENConv end in a torch.nn.Linear, so in the test above the awkward g meets torch (and the layer's
    _ready_grad) before it meets a conv Function: what the Functions get there is a fresh tensor.  Here the aggregation
    ops of the four layers get the awkward g themselves: transposed in memory and as ones(1).expand_as(out), every
    gradient bitwise that of the contiguous g."""
    from gcm import _ops
    gen = torch.Generator().manual_seed(77)
    B, N, M, E, F = 2, 33, 40, 90, 8
    x3, adj = torch.randn(B, N, F, generator=gen).to(DEV), (torch.rand(B, N, N, generator=gen) < 0.3).float().to(DEV)
    x2 = torch.randn(M, F, generator=gen).to(DEV)
    graph = _ops.GraphIndex.from_edge_index(torch.randint(0, M, (2, E), generator=gen).to(DEV), M)
    ops = {"dense_gin_aggregate": (x3, lambda x, p: _ops.dense_gin_aggregate(x, adj, p, True)),
           "csr_gin_aggregate": (x2, lambda x, p: _ops.csr_gin_aggregate(x, p, graph)),
           "dense_genagg": (x3, lambda x, p: _ops.dense_genagg(x, adj, p, 1e-7)),
           "csr_genagg": (x2, lambda x, p: _ops.csr_genagg(x, p, graph, 1e-7))}
    for name, (x, op) in ops.items():
        g = torch.randn(x.shape, generator=gen).to(DEV)
        gt, select = C.embed_transposed(g)
        ones = torch.ones(1, device=DEV).expand_as(g)
        assert not select(gt).is_contiguous() and set(ones.stride()) == {0}
        runs = []
        for gv in (g, select(gt), torch.ones_like(g), ones):
            xl, p = x.clone().requires_grad_(), torch.full((1,), 0.3, device=DEV, requires_grad=True)   # eps / t
            op(xl, p).backward(gv)
            torch.cuda.synchronize()
            assert float(xl.grad.abs().max()) > 0 and float(p.grad.abs()) > 0, name
            runs.append((xl.grad, p.grad))
        for a, b, what in ((runs[1], runs[0], "transposed"), (runs[3], runs[2], "expanded")):
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "%s: a g %s differs" % (name, what)
