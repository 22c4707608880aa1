"""GPU: the fused bulldozer kernels' instantiations for cell codes other than (0, 3, 25) (STD = false: byte compares
instead of the bit tests), which the env itself never takes. A batched env with its private codes and params set to
(0, 2, 9) before reset(): the fused step, with and without the meeting slots, against the gca_bulldozer_pre /
gca_windy_step / gca_bulldozer_post sequence after every step, and rollout_random(K) against K step_random calls, on
grids whose last strip is ragged. Bit-exact: the grids, every state tensor and every per-step record. `chain`: the effect
{TREE: FIRE, FIRE: EMPTY}, whose Modify changes the FIRE count (the rollout's barrier-per-step instantiation)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMPTY, TREE, FIRE = 0, 2, 9
E, K = 6, 24
# (33, 256): two strips of 32 rows, the second a single row; (17, 512): two strips of 16 rows, the same
CASES = [(33, 256, False), (17, 512, False), (33, 256, True)]
STATE = ("parity", "accu", "steps", "counts", "pos", "hit", "done", "rng_step", "steps_elapsed")


def _envs(device, H, W, chain, fused):
    """One env per entry of `fused`, all in the same state: fires sprinkled over the grid, the bulldozer of every other
    env in the ragged last row, fractions of time in [0, 0.9), env 0 finished."""
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv

    rng = np.random.default_rng(3)
    sprinkle = rng.random((E, H, W)) < 0.04
    accu = rng.random(E) * 0.9
    start = np.stack([np.where(np.arange(E) % 2 == 0, H - 1, 2), (np.arange(E) * 37) % W], axis=1)
    envs = []
    for f in fused:
        env = BatchedForestFireBulldozerEnv(E, H, W, device=device, seed=29, fused=f, materialize_obs=False, t_move=0.4,
                                            t_shoot=0.3, p_tree=0.6, p_empty=0.4)
        env._tree, env._fire = TREE, FIRE
        p = env.params
        p.tree, p.fire = TREE, FIRE
        p.effect[3] = -1
        p.effect[TREE] = FIRE if chain else EMPTY
        if chain:
            p.effect[FIRE] = EMPTY
        env.reset(seed=4, positions=start)
        g = env.grids()
        assert set(torch.unique(g).tolist()) == {EMPTY, TREE, FIRE}
        g[torch.as_tensor(sprinkle, device=device)] = FIRE
        env.buf[0].copy_(g)
        env.buf[1].copy_(g)
        env.accu.copy_(torch.as_tensor(accu, device=device))
        call("gca_count_cells", dev.ptr(env.buf[0]), E, H, W, EMPTY, TREE, FIRE, dev.ptr(env.counts),
             dev.stream_ptr(device))
        env.done[0] = 1
        envs.append(env)
    return envs


def _same(x, y):
    import torch

    return torch.equal(torch.nan_to_num(x), torch.nan_to_num(y)) and (
        not x.is_floating_point() or torch.equal(torch.isnan(x), torch.isnan(y)))


def _assert_equal(a, b, where):
    import torch

    assert torch.equal(a.buf, b.buf), f"{where}: buf (both planes)"
    for name in STATE + ("reward",):
        assert _same(getattr(a, name), getattr(b, name)), f"{where}: {name}"


def _assert_run_is_not_degenerate(steps, env):
    """steps: the (K, E) record of env.steps. The run has env steps with and without a CA pass, an env finished before
    the first step and an env whose fire still burns after the last one."""
    assert (steps > 0).any() and (steps == 0).any(), steps
    assert (steps[0] == -1).any(), steps[0]
    assert ((env.counts[:, 2] > 0) & (env.done == 0)).any(), (env.counts, env.done)


@pytest.mark.parametrize("H,W,chain", CASES)
def test_fused_step_equals_three_kernel_step(device, H, W, chain):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    parts, one, three = _envs(device, H, W, chain, fused=(True, True, False))
    one._meet = None  # one workgroup per env
    assert parts.fused and one.fused and not three.fused and parts._meet is not None
    act = torch.zeros((E, 2), dtype=torch.int32, device=device)
    steps = []
    for k in range(K):
        call("gca_random_actions", dev.ptr(act), E, 0, 13, dev.ptr(three.rng_step), dev.stream_ptr(device))
        for env in (parts, one, three):
            env.step(act)
        steps.append(three.steps.clone())
        _assert_equal(parts, three, f"with meet, step {k}")
        _assert_equal(one, three, f"without meet, step {k}")
    assert int(parts._meet.abs().sum()) == 0
    _assert_run_is_not_degenerate(torch.stack(steps), three)


@pytest.mark.parametrize("H,W,chain", CASES)
def test_rollout_random_equals_step_random(device, H, W, chain):
    import torch

    eager, roll = _envs(device, H, W, chain, fused=(True, True))
    a_step = torch.zeros((E, 2), dtype=torch.int32, device=device)
    acts, rews, dones, steps = [], [], [], []
    for _ in range(K):
        eager.step_random(9, a_step)
        acts.append(a_step.clone())
        rews.append(eager.reward.clone())
        dones.append(eager.done.clone())
        steps.append(eager.steps.clone())
    a_out = torch.full((K, E, 2), -1, dtype=torch.int32, device=device)
    r_out = torch.full((K, E), 5.0, dtype=torch.float64, device=device)
    d_out = torch.full((K, E), 7, dtype=torch.uint8, device=device)
    roll.rollout_random(K, 9, a_out, r_out, d_out)
    torch.cuda.synchronize(device)
    _assert_equal(eager, roll, "after the rollout")
    assert torch.equal(a_out, torch.stack(acts)), "action record"
    assert _same(r_out, torch.stack(rews)), "reward record"
    assert torch.equal(d_out, torch.stack(dones)), "done record"
    _assert_run_is_not_degenerate(torch.stack(steps), eager)
