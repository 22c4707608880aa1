"""GPU: what only the bulldozer's PPO update on the device has (ppo_grad against the yardstick, its reproducibility,
capture and tile paths are in test_gpu_ppo.py, with the helicopter's): BulldozerPolicy.ppo_update against the
hand-written loop, as one graph, its argument errors and twenty steps that lower the loss, on synthetic records of
T = 1200 rows; and the loop end to end on an env's records with truncations inside the window."""
import numpy as np
import pytest

import _adam_ref as A
import _bulldozer_policy_ref as bref
import _ppo_ref as R

pytestmark = pytest.mark.gpu

BDZ = R.BDZ
EPOCHS, MINIBATCHES = 2, 2


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, device):
    import torch

    return None if a is None else torch.from_numpy(np.array(a)).to(device)


def _policy(device, c):
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    d = c["d"]
    return BulldozerPolicy((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device=device).load(c["w"])


def _records(device, c):
    return ({k: _dev(v, device) for k, v in c["rec"].items()}, _dev(c["adv"], device), _dev(c["ret"], device))


# ------------------------------------------------------------------ ppo_update
def _setup(device, lr=2.5e-4):
    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    c = R.case(BDZ, R.SHAPES[BDZ][0])
    pol = _policy(device, c)
    opt = ppo.Adam({n: getattr(pol, n) for n in WEIGHTS}, lr=lr)
    return (c, pol, opt) + _records(device, c)


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
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    c, pol, opt, rec, adv, ret = _setup(device)
    with pytest.raises(ValueError, match="T = 1200 samples do not divide into 7 minibatches"):
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
    """lr = 1e-3, the other hyper-parameters the defaults, 20 epochs of one minibatch of all T = 1200 rows of the
    smallest shape. The float64 yardstick (autograd of _ppo_ref.loss_and_grad, optax restated in
    _adam_ref.OptaxRef) takes the loss from 2.7400 to 0.3469, a factor 0.127; the host build gives 2.7400 -> 0.3469
    too. The assertion asks for less than half of the first loss."""
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    c, pol, opt, rec, adv, ret = _setup(device, lr=1e-3)
    gold = A.OptaxRef([np.asarray(c["w"][k], np.float64) for k in WEIGHTS], lr=1e-3)
    losses = []
    for _ in range(20):
        cur = {k: gold.w[i] for i, k in enumerate(WEIGHTS)}
        g, st, _, _ = R.loss_and_grad(cur, c["d"], c["rec"], c["adv"], c["ret"], np.arange(c["T"]), BDZ.heads)
        losses.append(st[0])
        gold.step([g[k] for k in WEIGHTS])
    assert losses[-1] < 0.3 * losses[0], (losses[0], losses[-1])  # the yardstick's own margin
    stats, info = pol.ppo_update(opt, rec, adv, ret, epochs=20, minibatches=1, seed=3)
    s = stats[:, 0].cpu().numpy()
    print(f"loss: yardstick {losses[0]:.6f} -> {losses[-1]:.6f}, device {s[0]:.6f} -> {s[-1]:.6f}")
    assert s[-1] < 0.5 * s[0]
    assert abs(s[0] - losses[0]) < 1e-4 * losses[0]  # the same loss before the first step
    assert (info[:, 0] > 0.5).cpu().numpy().any()  # the clip was active


# ------------------------------------------------------------------ end to end
def test_rollout_gae_ppo_grad_end_to_end(device):
    """The smallest env the fused rollout takes: E = 4 of 32 x 256, K = 6 with autoreset and max_episode_steps = 3, so
    `truncated` is set inside the window and the terminal flags matter to the advantages."""
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv, BulldozerPolicy

    r, Bk, Hd, H, W = shape = R.SHAPES[BDZ][0]
    d = bref.dims(*shape)
    E, K = 4, 6
    env = BatchedForestFireBulldozerEnv(E, H, W, device=device, seed=17, materialize_obs=False, t_move=0.3, t_shoot=0.25,
                                        autoreset=True, max_episode_steps=3)
    env.reset(seed=5)
    w = bref.make_weights(d, seed=3, head=2.0)
    pol = BulldozerPolicy(env, r, Bk, Hd).load(w)
    rec = env.rollout_policy(pol, K, seed=11)
    assert tuple(rec["action"].shape) == (K, E, 2) and tuple(rec["logits"].shape) == (K, E, 11)
    _, _, next_value = env.act(pol, seed=11)
    terminal = rec["terminated"] | rec["truncated"]
    term = terminal.cpu().numpy().astype(np.uint8)
    assert rec["truncated"].cpu().numpy().astype(bool)[:K - 1].any() and not term.all()  # inside the window
    adv, ret = ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95, terminal=terminal)
    host = {k: v.cpu().numpy() for k, v in rec.items()}
    want_a, want_r = R.host_gae(host["reward"], host["value"], next_value.cpu().numpy(), term, 0.99, 0.95)
    assert np.array_equal(_bits(adv.cpu().numpy()), _bits(want_a))
    assert np.array_equal(_bits(ret.cpu().numpy()), _bits(want_r))
    no_term, _ = R.host_gae(host["reward"], host["value"], next_value.cpu().numpy(), None, 0.99, 0.95)
    assert not np.array_equal(_bits(no_term), _bits(want_a))  # the flags change the advantages
    grads, stats = pol.ppo_grad(rec, adv, ret)
    st = stats.cpu().numpy()
    rows = np.arange(K * E)
    g64, s64, _, _ = R.loss_and_grad(w, d, host, want_a, want_r, rows, BDZ.heads)
    g32, s32, _, _ = R.loss_and_grad(w, d, host, want_a, want_r, rows, BDZ.heads, dtype="float32")
    # the weights are unchanged, so every ratio the kernel forms is 1 within rounding: nothing is clipped, and
    # approx_kl = mean((r - 1) - log r) ~ mean((r - 1)^2) / 2 bounds the kernel's own |ratio - 1| in the mean square;
    # 1e-10 is (1.4e-5)^2 / 2, a hundred roundings of a logit of a few units (the bound of test_gpu_ppo.py: the heads'
    # logits are of the same size)
    assert st[5] == 0 and 0 <= st[4] < 1e-10, (st[4], st[5])
    # with ratio = 1 and normalised advantages pg is -mean(A^), zero but for rounding: an absolute figure
    assert abs(st[1]) < 1e-6 and abs(s64[1]) < 1e-6
    e = R.errors({k: v.cpu().numpy() for k, v in grads.items()}, st, g64, s64)
    e32 = R.errors(g32, s32, g64, s64)
    keep = ("loss", "v_loss", "entropy", "adv_mean", "adv_std", "b2", "w_out")  # w_local / w_coarse / b1: relu kinks
    R.assert_within({k: e[k] for k in keep}, e32, "end to end")
