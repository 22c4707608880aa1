"""GPU: gca_adam_step and gca_permutation on the device (csrc/gca_opt.hip) through forest_fire.ppo. The cases of
tests/test_adam_host.py run on the device and equal the host build bit for bit (weights, both moments, the state block
and the info rows; 16-B and 4-B aligned tensors; clipping on, off and on zero gradients; annealing; a total above 2^21
elements, where the chunk grows); a captured step replayed three times equals three eager steps; state_dict round
trips; the permutation for every small T."""
import numpy as np
import pytest

import _adam_ref as A

pytestmark = pytest.mark.gpu


def _assert_same(dev, host, where):
    (od, pd, idv), (oh, ph, ih) = dev, host
    for n in pd:
        assert np.array_equal(A.bits(pd[n]), A.bits(ph[n])), (where, "w", n)
        assert np.array_equal(A.bits(od.m[n]), A.bits(oh.m[n])), (where, "m", n)
        assert np.array_equal(A.bits(od.v[n]), A.bits(oh.v[n])), (where, "v", n)
    assert np.array_equal(od.state.cpu().numpy()[:5], oh.state.numpy()[:5]), where
    assert np.array_equal(A.bits(idv), A.bits(ih)), where


@pytest.mark.parametrize("offset", [0, 1])
def test_adam_equals_the_host_build(device, offset):
    ws, gs = A.tensors(), A.gradients()
    dev = A.run_steps(device, ws, gs, offset=offset, **A.HYPER)
    assert all(p.storage_offset() == offset and p.data_ptr() % 16 == 4 * offset for p in dev[1].values())
    host = A.run_steps("cpu", ws, gs, offset=offset, **A.HYPER)
    _assert_same(dev, host, f"offset {offset}")
    # info holds the pre-clip norm and the learning rate: the float64 norm of the gradients, above and below 0.5
    want = [np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in step)) for step in gs]
    assert np.allclose(dev[2][:, 0], want, rtol=1e-6, atol=0) and max(want) > 0.5 > min(want)
    assert (A.bits(dev[2][:, 1]) == A.bits(np.float32(2.5e-4))).all()
    assert A.opt_state(dev[0])[0] == len(gs)


def test_adam_clipping_annealing_and_large_totals(device):
    ws = A.tensors()
    cases = [("below", A.gradients(steps=3, scale=0.1), A.HYPER),
             ("no clip", A.gradients(steps=3, scale=4.0), dict(A.HYPER, max_grad_norm=0.0)),
             ("above", A.gradients(steps=3, scale=4.0), A.HYPER),
             ("zeros", [[np.zeros_like(w) for w in ws]] + A.gradients(steps=1) + [[np.zeros_like(w) for w in ws]],
              A.HYPER)]
    for where, gs, hyper in cases:
        dev = A.run_steps(device, ws, gs, **hyper)
        _assert_same(dev, A.run_steps("cpu", ws, gs, **hyper), where)
        assert np.isfinite(dev[2]).all() and all(np.isfinite(p.cpu().numpy()).all() for p in dev[1].values())
    lengths = (5, 1025)
    hyper = dict(A.HYPER, anneal=(2, 3))
    gs = A.gradients(lengths, steps=9)
    dev = A.run_steps(device, A.tensors(lengths), gs, **hyper)
    _assert_same(dev, A.run_steps("cpu", A.tensors(lengths), gs, **hyper), "anneal")
    assert (dev[2][6:, 1] == 0).all() and (dev[2][:6, 1] > 0).all()
    # more than 2^21 elements: chunks of 2048, more than 256 partials, one tensor on the scalar path
    lengths = (2 ** 21 + 4099, 5, 1023)
    gs = A.gradients(lengths, steps=2, scale=2.0)
    for offset in (0, 1):
        dev = A.run_steps(device, A.tensors(lengths), gs, offset=offset, **A.HYPER)
        _assert_same(dev, A.run_steps("cpu", A.tensors(lengths), gs, offset=offset, **A.HYPER), f"large {offset}")


def test_adam_captured_step_and_state_dict(device):
    import torch

    ws, gs = A.tensors(), A.gradients(steps=6)
    eager, pe, ie = A.run_steps(device, ws, gs, **A.HYPER)
    opt, ps = A.make_opt(ws, device=device, **A.HYPER)
    for g in gs[:3]:
        opt.step(A.grads_on(g, device=device))
    sd = opt.state_dict()
    w3 = [ps[f"p{i}"].cpu().numpy() for i in range(len(ws))]
    # a step captured once and replayed three times is three steps: the count lives on the device
    static = A.grads_on(gs[3], device=device)
    info = torch.full((2,), float("nan"), device=device)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(static, info_out=info)
    assert A.opt_state(opt)[0] == 3  # capturing ran nothing
    for s in (3, 4, 5):
        for i, g in enumerate(gs[s]):
            static[f"p{i}"].copy_(torch.from_numpy(g))
        graph.replay()
        torch.cuda.synchronize(device)
        assert np.array_equal(A.bits(info), A.bits(ie[s]))
    assert A.opt_state(opt) == A.opt_state(eager) and A.opt_state(opt)[0] == 6
    for n in ps:
        assert np.array_equal(A.bits(ps[n]), A.bits(pe[n])) and np.array_equal(A.bits(opt.v[n]), A.bits(eager.v[n]))
    # state_dict / load_state_dict: a fresh optimizer on the weights of step 3 resumes with equal bits
    fresh, pn = A.make_opt(w3, device=device, **A.HYPER)
    fresh.load_state_dict(sd)
    for g in gs[3:]:
        fresh.step(A.grads_on(g, device=device))
    assert A.opt_state(fresh) == A.opt_state(eager)
    for n in pn:
        assert np.array_equal(A.bits(pn[n]), A.bits(pe[n])) and np.array_equal(A.bits(fresh.m[n]), A.bits(eager.m[n]))


def test_permutation_equals_the_host_build(device):
    import torch

    from gymca_amd.forest_fire import ppo

    for T in A.PERM_SIZES:
        out = torch.full((3, T), -1, dtype=torch.int32, device=device)
        got = ppo.permutation(T, 3, seed=7, epoch0=2, out=out)
        assert got is out
        want = ppo.permutation(T, 3, seed=7, epoch0=2, device="cpu")
        assert torch.equal(out.cpu(), want), T
    assert (np.sort(out.cpu().numpy(), axis=1) == np.arange(T)).all()
    # counter shifts the rows exactly as epoch0 does, read on the device at run time
    counter = torch.tensor([2, 99], dtype=torch.int32, device=device)
    base = ppo.permutation(1000, 6, seed=3, epoch0=10, device=device)
    assert base.device == device and base.dtype == torch.int32
    assert torch.equal(ppo.permutation(1000, 3, seed=3, epoch0=9, counter=counter), base[1:4])
    assert torch.equal(base.cpu(), ppo.permutation(1000, 6, seed=3, epoch0=10, device="cpu"))
    counter[0] = 3
    assert torch.equal(ppo.permutation(1000, 3, seed=3, epoch0=9, counter=counter), base[2:5])
