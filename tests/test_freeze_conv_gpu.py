"""Every conv layer of gcm.nn under frozen parameters and partial gradient requests.  The backward of each layer
allocates only the gradients that `ctx.needs_input_grad` asks for and hands the C ABI null pointers for the rest, where
they select code (early returns, workspace slices, shared intermediates); the forward passes a null store target for
what only a backward would read.  Each layer class runs on two shapes (tests/_freeze.py) under every subset of its
differentiable tensors (x, adj / edge_weight where the layer defines that gradient, every parameter), set as
requires_grad flags before the forward on the layer and on its restatement alike.  For every subset S:

  * the output is BITWISE that of the run that asks for everything (the host code launches the same forward kernel for
    every S, with or without the store target of the backward's intermediates - FORWARD_KERNEL_DIFFERS lists the layers
    where it does not: none);
  * S empty, grad mode on: the output does not require a gradient and nothing raises;
  * every tensor in S has a gradient within the family's bound (tests/_gcn_restate.assert_bounded: 3x the restatement's
    own float32 distance from its float64 evaluation, floor 5e-7 of the gradient's scale) of the float64 restatement
    evaluated under the SAME flags;
  * every tensor outside S has .grad None.

tests/test_freeze_cpu.py states what makes this sensitive: every one of these gradients is >= 100x its atol in size, so
a buffer left at zero cannot pass.  With -s: per layer the largest deviation of a subset's gradient from the full
run's, in units of the tensor's atol (a report: the kernels may legitimately sum in another order).  Needs an MI355X."""
import pytest
import torch

import _freeze as Z
from _gcn_restate import assert_bounded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# layer ids whose host code picks ANOTHER forward kernel for some subset: their outputs are held to the float64 bound
# of the restatement instead of bitwise equality with the full run
FORWARD_KERNEL_DIFFERS = frozenset()


@pytest.mark.parametrize("family,dense", Z.LAYERS, ids=[Z.layer_id(f, d) for f, d in Z.LAYERS])
def test_every_subset_of_gradients(family, dense):
    lid = Z.layer_id(family, dense)
    report = (0.0, "every subset gradient is bitwise the full run's")
    for i in (0, 1):
        s = Z.spec(family, dense, i)
        conv = s.product().to(DEV)
        assert Z.tensor_names(s.inputs, conv) == s.names, "the layer and its restatement name their tensors differently"
        picks = Z.subsets(s.names)
        full = None
        for subset in picks:
            tag = "%s-%d [%s]" % (lid, i, Z.subset_id(subset, s.names))
            ref = Z.reference(family, dense, i, subset)
            o64, g64 = ref[torch.float64]
            o32, g32 = ref[torch.float32]
            out, grads, req = Z.run(conv, s, subset, device=DEV)
            torch.cuda.synchronize()
            assert req == bool(subset), tag + ": out.requires_grad"
            assert out.shape == o64.shape and bool(torch.isfinite(out).all()), tag
            if full is None:
                full = (out, grads)
                assert_bounded(out, o64, o32, tag + " out")
            elif lid in FORWARD_KERNEL_DIFFERS:
                assert_bounded(out, o64, o32, tag + " out")
            else:
                assert torch.equal(out, full[0]), tag + ": the output differs from the full run's"
            for name in s.names:
                if name not in subset:
                    assert grads[name] is None, tag + ": %s is frozen and got a gradient" % name
                    continue
                assert grads[name] is not None, tag + ": %s got no gradient" % name
                got = grads[name].reshape(g64[name].shape)
                assert bool(torch.isfinite(got).all()), tag + " " + name
                assert_bounded(got, g64[name], g32[name], tag + " " + name, floor=Z.GRAD_FLOOR, relative=True)
                dev = float((got - full[1][name].reshape(got.shape)).abs().max()) / Z.bound(g64[name], g32[name])
                if dev > report[0]:
                    report = (dev, tag + " " + name)
    print("\nFREEZE %s: largest |subset gradient - full run's| = %.3f atol (%s)" % (lid, report[0], report[1]))
