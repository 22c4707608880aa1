"""GPU: HelicopterPolicy.ppo_update, the whole PPO update on the device (one permutation launch, then per epoch and
minibatch ppo_grad and Adam.step), on the records of _ppo_ref's smallest shape (T = 1200) at 2 epochs x 2 minibatches:
equal to the hand-written loop bit for bit, capturable as one graph whose replays draw new shuffles, its argument
errors, and twenty full-batch steps that lower the loss as the float64 yardstick says they must."""
import numpy as np
import pytest

import _adam_ref as A
import _ppo_ref as R

pytestmark = pytest.mark.gpu

SHAPE = R.SHAPES[R.HELI][0]
EPOCHS, MINIBATCHES = 2, 2


def _setup(device, lr=2.5e-4):
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.helicopter import HelicopterPolicy
    from gymca_amd.forest_fire.helicopter.policy import WEIGHTS

    c = R.case(R.HELI, SHAPE)
    d = c["d"]
    pol = HelicopterPolicy((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device=device).load(c["w"])
    opt = ppo.Adam({n: getattr(pol, n) for n in WEIGHTS}, lr=lr)
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    return c, pol, opt, {k: t(v) for k, v in c["rec"].items()}, t(c["adv"]), t(c["ret"])


def _weights(pol):
    return {n: t.clone() for n, t in pol.state_dict().items()}


def _same(a, b):
    return all(np.array_equal(A.bits(a[n]), A.bits(b[n])) for n in a)


def test_ppo_update_equals_the_hand_written_loop(device):
    import torch

    from gymca_amd.forest_fire import ppo

    c, pol, opt, rec, adv, ret = _setup(device)
    T = c["T"]
    N = T // MINIBATCHES
    perm_out = torch.full((EPOCHS, T), -1, dtype=torch.int32, device=device)
    stats, info = pol.ppo_update(opt, rec, adv, ret, epochs=EPOCHS, minibatches=MINIBATCHES, seed=5, perm_out=perm_out)
    assert stats.shape == (4, 8) and info.shape == (4, 2) and torch.isfinite(stats).all()
    assert (np.sort(perm_out.cpu().numpy(), axis=1) == np.arange(T)).all()
    assert A.opt_state(opt)[0] == 4
    # by hand: the shuffles are keyed by the optimizer's count on entry
    _, pol2, opt2, _, _, _ = _setup(device)
    want_s, want_i = [], []
    perm = ppo.permutation(T, EPOCHS, seed=5, counter=opt2.count)
    assert torch.equal(perm, perm_out)
    for e in range(EPOCHS):
        for mb in range(MINIBATCHES):
            grads, s = pol2.ppo_grad(rec, adv, ret, perm[e, mb * N:(mb + 1) * N])
            want_s.append(s)
            want_i.append(opt2.step(grads))
    assert np.array_equal(A.bits(stats), A.bits(torch.stack(want_s)))
    assert np.array_equal(A.bits(info), A.bits(torch.stack(want_i)))
    assert _same(_weights(pol), _weights(pol2))
    assert not _same(_weights(pol), {k: torch.from_numpy(np.array(v)) for k, v in c["w"].items()})
    assert (info[:, 0] > 0).all() and (A.bits(info[:, 1]) == A.bits(np.float32(2.5e-4))).all()


def test_ppo_update_as_one_graph(device):
    import torch

    c, pol, opt, rec, adv, ret = _setup(device)
    _, pol2, opt2, _, _, _ = _setup(device)
    T = c["T"]
    steps = EPOCHS * MINIBATCHES
    eager = [pol2.ppo_update(opt2, rec, adv, ret, epochs=EPOCHS, minibatches=MINIBATCHES, seed=5) for _ in range(2)]
    # every buffer given: nothing is allocated and nothing syncs, so the call is one graph
    stats = torch.full((steps, 8), float("nan"), device=device)
    info = torch.full((steps, 2), float("nan"), device=device)
    perm = torch.full((EPOCHS, T), -1, dtype=torch.int32, device=device)
    grads = {n: torch.empty(s, device=device) for n, s in pol.weight_shapes().items()}
    ws = torch.empty(pol._ppo_workspace(T // MINIBATCHES, None).numel(), dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pol.ppo_update(opt, rec, adv, ret, epochs=EPOCHS, minibatches=MINIBATCHES, seed=5, stats_out=stats,
                             info_out=info, perm_out=perm, grads_out=grads, workspace=ws)
    assert out[0] is stats and out[1] is info
    perms = []
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize(device)
        assert np.array_equal(A.bits(stats), A.bits(eager[k][0])) and np.array_equal(A.bits(info), A.bits(eager[k][1]))
        perms.append(perm.clone())
    assert not torch.equal(perms[0], perms[1])  # the count moved, so the second replay shuffled anew
    assert A.opt_state(opt) == A.opt_state(opt2) and A.opt_state(opt)[0] == 2 * steps
    assert _same(_weights(pol), _weights(pol2))


def test_ppo_update_argument_errors(device):
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.helicopter.policy import WEIGHTS

    c, pol, opt, rec, adv, ret = _setup(device)
    with pytest.raises(ValueError, match="do not divide into 7 minibatches"):
        pol.ppo_update(opt, rec, adv, ret, epochs=1, minibatches=7)
    with pytest.raises(ValueError, match="stats_out"):
        pol.ppo_update(opt, rec, adv, ret, epochs=2, minibatches=2, stats_out=torch.zeros((3, 8), device=device))
    with pytest.raises(ValueError, match="forest_fire.ppo.Adam"):
        pol.ppo_update(ppo.Adam({"b1": pol.b1}), rec, adv, ret)
    pol.b2 = pol.b2.clone()  # a reassigned tensor: the optimizer would update the old one
    with pytest.raises(ValueError, match=r"opt.params\['b2'\] is not policy.b2"):
        pol.ppo_update(opt, rec, adv, ret, epochs=2, minibatches=2)
    assert A.opt_state(opt)[0] == 0  # nothing ran
    opt = ppo.Adam({n: getattr(pol, n) for n in WEIGHTS})
    pol.ppo_update(opt, rec, adv, ret, epochs=1, minibatches=2)
    assert A.opt_state(opt)[0] == 2


def test_twenty_full_batch_steps_lower_the_loss(device):
    """lr = 1e-3, the other hyper-parameters the defaults (clip 0.5, b1 0.9, b2 0.999, eps 1e-5), 20 epochs of one
    minibatch of all T = 1200 rows. The float64 yardstick (autograd of _ppo_ref.loss_and_grad, optax restated in
    _adam_ref.OptaxRef) takes the loss from 1.8104 to 0.4666, a factor 0.258; the host build gives 1.8104 -> 0.4666
    too. The assertion asks for less than half of the first loss."""
    from gymca_amd.forest_fire.helicopter.policy import WEIGHTS

    c, pol, opt, rec, adv, ret = _setup(device, lr=1e-3)
    gold = A.OptaxRef([np.asarray(c["w"][k], np.float64) for k in WEIGHTS], lr=1e-3)
    losses = []
    for _ in range(20):
        cur = {k: gold.w[i] for i, k in enumerate(WEIGHTS)}
        g, st, _, _ = R.loss_and_grad(cur, c["d"], c["rec"], c["adv"], c["ret"], np.arange(c["T"]), R.HELI.heads)
        losses.append(st[0])
        gold.step([g[k] for k in WEIGHTS])
    assert losses[-1] < 0.3 * losses[0], (losses[0], losses[-1])  # the yardstick's own margin
    stats, info = pol.ppo_update(opt, rec, adv, ret, epochs=20, minibatches=1, seed=3)
    s = stats[:, 0].cpu().numpy()
    print(f"loss: yardstick {losses[0]:.6f} -> {losses[-1]:.6f}, device {s[0]:.6f} -> {s[-1]:.6f}")
    assert s[-1] < 0.5 * s[0]
    assert abs(s[0] - losses[0]) < 1e-4 * losses[0]  # the same loss before the first step
    assert (info[:, 0] > 0.5).cpu().numpy().any()  # the clip was active
