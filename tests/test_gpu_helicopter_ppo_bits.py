"""GPU: HelicopterPolicy.ppo_grad computes what it computed before its kernels were generalised over the head layout.
tests/golden/helicopter_ppo_bits.npz holds the uint32 bits of the five gradients and of `stats` for the helicopter's
_ppo_ref.SHAPES [1] and [5] with _ppo_ref.minibatch(c, 333), recorded on an MI355X at the commit before the generalisation (e66b18c). The
head layout is a template parameter and the helicopter's instantiation runs the same operations in the same order, so
the bits must be the same; a difference means the helicopter path was changed."""
import numpy as np
import pytest

import _ppo_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("si", [1, 5])
def test_helicopter_ppo_grad_bits_are_the_parents(device, golden, si):
    import torch

    from gymca_amd.forest_fire.helicopter import HelicopterPolicy

    want = golden("helicopter_ppo_bits")
    c = R.case(R.HELI, R.SHAPES[R.HELI][si])
    d = c["d"]
    pol = HelicopterPolicy((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device=device).load(c["w"])
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    grads, stats = pol.ppo_grad({k: t(v) for k, v in c["rec"].items()}, t(c["adv"]), t(c["ret"]), t(R.minibatch(c, 333)))
    for k in R.GRADS:
        got = grads[k].cpu().numpy().view(np.uint32)
        assert got.shape == want[f"s{si}_{k}"].shape and np.array_equal(got, want[f"s{si}_{k}"]), k
    assert np.array_equal(stats.cpu().numpy().view(np.uint32), want[f"s{si}_stats"])
