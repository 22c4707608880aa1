"""GPU: BatchedForestFireBulldozerEnv.rollout / gca_bulldozer_rollout (K env steps in one launch with the caller's
actions or the random policy, and the per-env reset inside the launch under autoreset) against K eager env.step /
env.step_random calls on a twin env -- the eager pair of launches is pinned to the oracle by
tests/test_gpu_bulldozer_reset.py -- and, for one shape, against the numpy restatement (tests/_bulldozer_rollout_ref.py).
Bit-exact: both grid planes, every state tensor, env.reward and the per-step records."""
import numpy as np
import pytest

import _bulldozer_reset_ref as rref
import _bulldozer_rollout_ref as ref

pytestmark = pytest.mark.gpu

# (6, 8, 256): one wave, fewer quads than a full strip; (5, 40, 256): two waves, partial last strip; (3, 24, 512): the
# 512-wide rows, partial strip; (2, 544, 256): 17 strips over 16 waves (the strip loop wraps, the refill loops)
SHAPES = [(6, 8, 256), (5, 40, 256), (3, 24, 512), (2, 544, 256)]
STATE = ("parity", "pos", "counts", "accu", "done", "hit", "steps", "rng_step", "steps_elapsed", "episode",
         "last_episode_length", "_terminated", "_truncated_u8")
MOVES = np.array([0, 1, 2, 3, 5, 6, 7, 8])
EMPTY_GRID = dict(p_tree=0.0, p_empty=1.0)  # EMPTY but for the one FIRE cell: an episode ends within two steps


def _env(E, H, W, device, **kw):
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv

    kw.setdefault("t_move", 0.4)
    kw.setdefault("t_shoot", 0.3)
    return BatchedForestFireBulldozerEnv(E, H, W, device=device, seed=17, materialize_obs=False, **kw)


def _pair(device, shape, n=2, prepare=None, chain=False, **kw):
    """n envs with the same constructor arguments, seed and state."""
    envs = [_env(*shape, device, **kw) for _ in range(n)]
    for env in envs:
        if chain:  # a Modify that changes the FIRE count: the rollout kernel's barrier-per-step path
            env.params.effect[3], env.params.effect[25] = 25, 0
        env.reset(seed=5)
        if prepare is not None:
            prepare(env)
    return envs


def _mid_episode(env):
    """Fires sprinkled over both planes, random parity and fractions of time in [0, 0.9), two envs finished."""
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    E, H, W = env.num_envs, env.nrows, env.ncols
    rng = np.random.default_rng(11)
    g = env.grids().cpu().numpy()
    g[rng.random(g.shape) < 0.05] = 25
    g = torch.as_tensor(g, device=env.device)
    env.buf[0].copy_(g)
    env.buf[1].copy_(g)
    env.parity.copy_(torch.as_tensor(rng.integers(0, 2, E).astype(np.uint8), device=env.device))
    env.accu.copy_(torch.as_tensor(rng.random(E) * 0.9, device=env.device))
    call("gca_count_cells", dev.ptr(env.buf[0]), E, H, W, 0, 3, 25, dev.ptr(env.counts), dev.stream_ptr(env.device))
    _finish(env)


def _finish(env):
    env.done[0] = 1
    env.done[env.num_envs - 1] = 1


def _actions(rng, K, E, device, wild=False):
    import torch

    a = np.stack([rng.integers(0, 9, (K, E)), rng.integers(0, 2, (K, E))], axis=2)
    if wild:  # outside [0, 9) x {0, 1}: clamped for the time, recorded as they are
        a[1, :, 0], a[2, :, 1], a[3, 1], a[4, -2] = 12, 5, (-3, -1), (9, 2)
    return torch.as_tensor(a.astype(np.int32), device=device)


def _fire_out_actions(rng, K, E, device):
    import torch

    a = np.stack([rng.choice(MOVES, (K, E)), np.ones((K, E), np.int64)], axis=2)
    return torch.as_tensor(a.astype(np.int32), device=device)


def _eager(env, actions, K, seed=9, ca_steps=None):
    """K eager steps; the per-step records (actions, reward, terminated, truncated) as the rollout defines them.
    ca_steps: a list that receives each step's env.steps (the CA passes the step ran)."""
    import torch

    a_step = torch.zeros((env.num_envs, 2), dtype=torch.int32, device=env.device)
    acts, rews, terms, truncs = [], [], [], []
    for k in range(K):
        if actions is None:
            env.step_random(seed, a_step)
            acts.append(a_step.clone())
        else:
            env.step(actions[k])
            acts.append(actions[k].clone())
        rews.append(env.reward.clone())
        if ca_steps is not None:
            ca_steps.append(env.steps.clone())
        terms.append((env._terminated if env.autoreset else env.done).clone())
        truncs.append(env._truncated_u8.clone() if env.autoreset else torch.zeros_like(env.done))
    return torch.stack(acts), torch.stack(rews), torch.stack(terms), torch.stack(truncs)


def _rollout(env, actions, K, seed=9):
    import torch

    E = env.num_envs
    a_out = torch.full((K, E, 2), -7, dtype=torch.int32, device=env.device)
    r_out = torch.full((K, E), 5.0, dtype=torch.float64, device=env.device)
    t_out = torch.full((K, E), 7, dtype=torch.uint8, device=env.device)
    u_out = torch.full((K, E), 7, dtype=torch.uint8, device=env.device)
    got = env.rollout(actions, None if actions is not None else K, seed, a_out, r_out, t_out, u_out)
    assert got[0] is r_out and got[1] is t_out and got[2] is u_out
    return a_out, r_out, t_out, u_out


def _same(x, y):
    import torch

    if x.is_floating_point():  # NaN where NaN, equal elsewhere
        return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    return torch.equal(x, y)


def _assert_envs_equal(a, b, where=""):
    import torch

    torch.cuda.synchronize(a.device)
    assert torch.equal(a.buf, b.buf), f"{where}: buf (both planes)"
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), f"{where}: {k}"
    assert _same(a.reward, b.reward), f"{where}: reward"


def _assert_records_equal(want, got, where=""):
    for name, w, g in zip(("action", "reward", "terminated", "truncated"), want, got):
        assert _same(w, g), f"{where}: {name} record"


def _snapshot(env):
    return [env.buf.clone(), env.reward.clone()] + [getattr(env, k).clone() for k in STATE]


def _assert_unchanged(env, before, where=""):
    import torch

    torch.cuda.synchronize(env.device)
    for name, old, new in zip(("buf", "reward") + STATE, before, _snapshot(env)):
        assert _same(old, new), f"{where}: {name} changed"


@pytest.mark.parametrize("shape", SHAPES)
def test_callers_actions_autoreset_off(device, shape):
    K = 14
    eager, roll = _pair(device, shape, prepare=_mid_episode)
    assert roll.fused
    act = _actions(np.random.default_rng(1), K, shape[0], device, wild=True)
    want = _eager(eager, act, K)
    got = _rollout(roll, act, K)
    _assert_envs_equal(eager, roll)
    _assert_records_equal(want, got)
    assert _same(got[0], act) and int(got[0].max()) == 12 and int(got[0].min()) == -3  # unclamped
    assert not got[3].any() and got[2][:, 0].all() and (got[1][:, 0] == 0).all()  # finished on entry: no-op steps


@pytest.mark.parametrize("shape", SHAPES)
def test_autoreset_fire_out_episodes(device, shape):
    """Every env finishes within two steps of an episode's start (test_autoreset_episode_chain_matches_oracle's scheme):
    the in-launch reset runs every other step of every env. (6, 8, 256) is also compared with the numpy restatement."""
    E, H, W = shape
    K = 12
    eager, roll = _pair(device, shape, prepare=_finish, autoreset=True, **EMPTY_GRID)
    act = _fire_out_actions(np.random.default_rng(2), K, E, device)
    state = ref.env_state(roll)
    want = _eager(eager, act, K)
    assert (eager.episode >= 2).all(), eager.episode  # a condition on the yardstick
    got = _rollout(roll, act, K)
    _assert_envs_equal(eager, roll)
    _assert_records_equal(want, got)
    if shape == SHAPES[0]:
        rew, term, trunc = ref.ref_rollout(state, act.cpu().numpy(), roll.wind[0].cpu().numpy(), roll.t_act_move,
                                           roll.t_act_shoot, roll.t_any, seed=17, reset_seed=5, cdf=rref.env_cdf(roll),
                                           autoreset=True)
        ref.assert_states_equal(ref.env_state(roll), state, "restatement")
        assert np.array_equal(got[1].cpu().numpy(), rew, equal_nan=True)
        assert np.array_equal(got[2].cpu().numpy(), term) and np.array_equal(got[3].cpu().numpy(), trunc)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_time_limit(device, shape):
    """Clocks staggered over the limit's period: truncations fall on different steps, some of them steps without a CA
    pass (no barrier of their own before the refill)."""
    import torch

    E = shape[0]
    K = 12

    def stagger(env):
        env.steps_elapsed.copy_(torch.arange(E, device=device) % 5)

    eager, roll = _pair(device, shape, prepare=stagger, autoreset=True, max_episode_steps=5, p_tree=0.5, p_empty=0.1)
    act = _actions(np.random.default_rng(3), K, E, device)
    ca_steps = []
    want = _eager(eager, act, K, ca_steps=ca_steps)
    assert int(want[3].any(dim=1).sum()) >= 2, want[3]  # conditions on the yardstick: truncations in different rows,
    assert (want[3].bool() & (torch.stack(ca_steps) == 0)).any()  # some on steps without a CA pass
    got = _rollout(roll, act, K)
    _assert_envs_equal(eager, roll)
    _assert_records_equal(want, got)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]])
def test_random_policy_autoreset(device, shape):
    K = 16
    eager, roll = _pair(device, shape, prepare=_finish, autoreset=True, **EMPTY_GRID)
    want = _eager(eager, None, K, seed=9)
    assert int(eager.episode.sum()) > 0
    got = _rollout(roll, None, K, seed=9)
    _assert_envs_equal(eager, roll)
    _assert_records_equal(want, got)


def test_random_policy_autoreset_off_equals_rollout_random(device):
    import torch

    K, shape = 16, SHAPES[1]
    a, b = _pair(device, shape, prepare=_mid_episode)
    got = _rollout(a, None, K, seed=4)
    d_out = torch.zeros((K, shape[0]), dtype=torch.uint8, device=device)
    r_out = torch.zeros((K, shape[0]), dtype=torch.float64, device=device)
    a_out = torch.zeros((K, shape[0], 2), dtype=torch.int32, device=device)
    b.rollout_random(K, 4, a_out, r_out, d_out)
    _assert_envs_equal(a, b)
    _assert_records_equal((a_out, r_out, d_out, torch.zeros_like(d_out)), got)


def test_barrier_per_step_path_with_reset(device):
    """A Modify that changes the FIRE count (TREE -> FIRE -> EMPTY) takes the kernel's barrier-per-step path; the time
    limit and two finished envs make it reset."""
    K, shape = 14, SHAPES[1]
    eager, roll = _pair(device, shape, prepare=_finish, chain=True, autoreset=True, max_episode_steps=4, p_tree=0.3,
                        p_empty=0.7)
    act = _actions(np.random.default_rng(5), K, shape[0], device)
    act[:, :, 1] = 1
    want = _eager(eager, act, K)
    assert (eager.episode >= 2).all()
    got = _rollout(roll, act, K)
    _assert_envs_equal(eager, roll)
    _assert_records_equal(want, got)


def test_sharded_rollout_reproduces_the_unsharded_envs(device):
    import torch

    K, (E, H, W) = 12, SHAPES[0]
    kw = dict(autoreset=True, **EMPTY_GRID)
    full = _env(E, H, W, device, **kw)
    shards = [_env(E // 2, H, W, device, env_offset=off, **kw) for off in (0, E // 2)]
    for env in [full] + shards:
        env.reset(seed=5)
    act = _fire_out_actions(np.random.default_rng(6), K, E, device)
    whole = _rollout(full, act, K)
    parts = [_rollout(sh, act[:, i * (E // 2):(i + 1) * (E // 2)].contiguous(), K) for i, sh in enumerate(shards)]
    torch.cuda.synchronize(device)
    assert (full.episode >= 2).all()
    assert torch.equal(full.buf, torch.cat([sh.buf for sh in shards], dim=1))
    for k in STATE:
        assert torch.equal(getattr(full, k), torch.cat([getattr(sh, k) for sh in shards])), k
    assert _same(full.reward, torch.cat([sh.reward for sh in shards]))
    for j in range(4):
        assert _same(whole[j], torch.cat([p[j] for p in parts], dim=1)), j


def test_not_fusable_loops_over_step(device):
    import torch

    K, shape = 12, (6, 32, 32)
    eager, roll = _pair(device, shape, prepare=_finish, autoreset=True, t_move=None, t_shoot=None, **EMPTY_GRID)
    assert not roll.fused and roll.max_passes == 2
    act = _fire_out_actions(np.random.default_rng(7), K, shape[0], device)
    want = _eager(eager, act, K)
    assert (eager.episode >= 2).all()
    got = _rollout(roll, act, K)
    _assert_envs_equal(eager, roll)
    _assert_records_equal(want, got)
    # the random policy there: sample_actions(tag=seed) + step, which is what step_random fuses where it exists
    drawn = []
    for _ in range(4):
        drawn.append(eager.sample_actions(tag=9).clone())
        eager.step(drawn[-1])
    got = _rollout(roll, None, 4, seed=9)
    _assert_envs_equal(eager, roll)
    assert _same(got[0], torch.stack(drawn))


def test_interleaving_and_k_zero(device):
    import torch

    K1, K2, shape = 5, 7, SHAPES[1]
    eager, roll = _pair(device, shape, prepare=_finish, autoreset=True, max_episode_steps=6, p_tree=0.5, p_empty=0.1)
    act = _actions(np.random.default_rng(8), K1 + 1 + K2, shape[0], device)
    want = _eager(eager, act, K1 + 1 + K2)
    first = _rollout(roll, act[:K1].cpu().numpy().astype(np.int64), K1)  # host actions are converted
    roll.rebind()  # drops the bound rollout call; the next one binds again
    assert roll._rollout_call is None
    roll.step(act[K1])
    second = _rollout(roll, act[K1 + 1:], K2)
    _assert_envs_equal(eager, roll)
    for j in range(4):
        assert _same(want[j][:K1], first[j]) and _same(want[j][K1 + 1:], second[j]), j
    before = _snapshot(roll)
    out = roll.rollout(K=0)
    assert [tuple(t.shape) for t in out] == [(0, shape[0])] * 3
    roll.rollout(act[:0])
    _assert_unchanged(roll, before, "K = 0")


def test_graph_of_rollouts_replays_as_eager(device):
    import torch

    from gymca_amd.graph import StepGraph

    K, shape = 6, SHAPES[1]
    E = shape[0]
    a, b = _pair(device, shape, prepare=_finish, autoreset=True, **EMPTY_GRID)
    act = _fire_out_actions(np.random.default_rng(9), K, E, device)
    recs = [(torch.zeros((K, E), dtype=torch.float64, device=device), torch.zeros((K, E), dtype=torch.uint8, device=device),
             torch.zeros((K, E), dtype=torch.uint8, device=device)) for _ in range(2)]
    graph = StepGraph(lambda: a.rollout(act, reward_out=recs[0][0], terminated_out=recs[0][1],
                                        truncated_out=recs[0][2]), n_steps=2, device=device, warmup=1)
    run_b = lambda: b.rollout(act, reward_out=recs[1][0], terminated_out=recs[1][1], truncated_out=recs[1][2])
    run_b()  # the graph's one eager warm-up call
    for _ in range(2):
        graph.replay()
        run_b()
        run_b()
    _assert_envs_equal(a, b)
    for x, y in zip(*recs):
        assert _same(x, y)
    assert (a.episode >= 10).all()


def test_errors(device):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd import _lib

    E, H, W = SHAPES[0]
    K = 3
    env = _env(E, H, W, device, autoreset=True)
    env.reset(seed=5)
    before = _snapshot(env)
    good = torch.zeros((K, E, 2), dtype=torch.int32, device=device)
    for bad in (good.double(), good.bool(), np.zeros((K, E, 2)), good[:, :, 0], good[:, :-1], np.zeros((K, E), np.int64),
                good.cpu()):
        with pytest.raises(ValueError, match="actions"):
            env.rollout(bad)
    with pytest.raises(ValueError, match="disagrees"):
        env.rollout(good, K=K + 1)
    with pytest.raises(ValueError, match="K >= 0"):
        env.rollout(K=-1)
    with pytest.raises(ValueError, match="K is needed"):
        env.rollout()
    f64 = torch.zeros((K, E), dtype=torch.float64, device=device)
    u8 = torch.zeros((K, E), dtype=torch.uint8, device=device)
    for kw in (dict(reward_out=u8), dict(reward_out=f64[:-1]), dict(terminated_out=f64), dict(truncated_out=u8[:, :-1]),
               dict(truncated_out=u8.cpu()), dict(action_out=u8), dict(action_out=good[:, :, :1]),
               dict(terminated_out=u8.t())):
        with pytest.raises(ValueError, match="_out"):
            env.rollout(good, **kw)
    # a null `done` through the raw ABI: GCA_ERR_ARG (1) before any launch
    one = dev.ptr(env.hit)
    status = _lib.load().gca_bulldozer_rollout(env.params, None, 9, K, None, None, None, None, 1, 5, 0,
                                               dev.ptr(env._reset_cdf), dev.ptr(env._reset_vals), one, one, one, one,
                                               one, one, None, one, 9, one, one, dev.ptr(env.buf[0]),
                                               dev.ptr(env.buf[1]), H, W, one, one, one, one, one, E,
                                               dev.stream_ptr(device))
    assert status == 1 and b"null" in _lib.load().gca_last_error()
    _assert_unchanged(env, before, "after refused calls")
