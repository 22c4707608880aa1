"""GPU: the per-env reset of the batched ForestFireBulldozer env (env.reset_where / autoreset=True,
gca_bulldozer_reset_where) against reset() itself, the numpy restatement (tests/_bulldozer_reset_ref.py) and, over
chains of episodes, the CPU oracle of the env step (oracle.windy.BulldozerOracle). Bit-exact states."""
import numpy as np
import pytest

import _bulldozer_reset_ref as ref
from oracle import windy as owindy

pytestmark = pytest.mark.gpu

# (2, 64, 256): more quads of cells than the reset's workgroup has threads; (5, 7, 9): unaligned env bases and a
# partial last quad; (3, 33, 40): rows that are no multiple of anything
SHAPES = [(5, 7, 9), (3, 33, 40), (4, 16, 256), (3, 8, 512), (2, 64, 256)]
STATE = ("parity", "pos", "counts", "accu", "done", "hit", "steps_elapsed")
MOVES = np.array([0, 1, 2, 3, 5, 6, 7, 8])


def _env(E, H, W, device, **kw):
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv

    return BatchedForestFireBulldozerEnv(E, H, W, device=device, seed=17, **kw)


def _random_actions(rng, E):
    return np.stack([rng.integers(0, 9, E), rng.integers(0, 2, E)], axis=1)


def _snapshot(env):
    d = {k: getattr(env, k).cpu().numpy().copy() for k in STATE}
    d["grids"] = env.grids().cpu().numpy()
    d["buf0"] = env.buf[0].cpu().numpy()
    return d


@pytest.mark.parametrize("shape", SHAPES)
def test_episode_zero_equals_reset(device, shape):
    import torch

    E, H, W = shape
    env = _env(E, H, W, device)
    env.reset(seed=5)
    want = _snapshot(env)
    assert (want["counts"][:, 2] == 1).all() and want["counts"].sum() == E * H * W
    ones = torch.ones(E, dtype=torch.uint8, device=device)
    env.reset_where(ones, episode=0)
    got = _snapshot(env)
    for k in want:
        assert np.array_equal(got[k], want[k]), f"fresh: {k}"
    rng = np.random.default_rng(1)
    for _ in range(10):
        env.step(_random_actions(rng, E))
    rs = env.rng_step.clone()
    env.reset_where(ones.bool(), episode=0)
    got = _snapshot(env)
    for k in want:
        assert np.array_equal(got[k], want[k]), f"after 10 steps: {k}"
    assert torch.equal(env.rng_step, rs) and (env.episode == 0).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_partial_mask_equals_the_restatement(device, shape):
    import torch

    E, H, W = shape
    env = _env(E, H, W, device, p_tree=0.6, p_empty=0.1)
    env.reset(seed=5)
    rng = np.random.default_rng(2)
    for _ in range(6):
        env.step(_random_actions(rng, E))
    mask = np.zeros(E, np.uint8)
    mask[::2] = 1
    env.done[1] = 1  # an unmasked done env stays done
    for k in (1, 2):
        s = ref.env_state(env)
        rs = env.rng_step.clone()
        ref.ref_reset_where(s, 5, 0, ref.env_cdf(env), mask=mask)
        obs, info = env.reset_where(torch.as_tensor(mask, device=device) if k == 1 else mask)
        ref.assert_states_equal(ref.env_state(env), s, f"episode {k}")  # both buffers and every state tensor
        assert (s["episode"][::2] == k).all() and (s["episode"][1::2] == 0).all() and s["done"][1] == 1
        assert torch.equal(env.rng_step, rs)
        assert info["episode"] is env.episode and torch.equal(obs[0], env.grids())
        env.step(_random_actions(rng, E))
    # an explicit episode index replays that episode
    s = ref.env_state(env)
    ref.ref_reset_where(s, 5, 0, ref.env_cdf(env), mask=mask, set_episode=300)
    env.reset_where(mask, episode=300)
    ref.assert_states_equal(ref.env_state(env), s, "episode 300")


def _chain(env, seed, steps, env_offset=0):
    """Step `env` (autoreset=True, after reset(seed)) with move != 4, shoot = 1 and compare every step with the oracle;
    where an env terminated, its new episode with the restatement, which is then spliced into the oracle. Returns the
    number of episodes each env completed."""
    E, H, W = env.num_envs, env.nrows, env.ncols
    o = owindy.BulldozerOracle(env.grids().cpu().numpy(), env.pos.cpu().numpy(),
                               env.wind[0].cpu().numpy().reshape(3, 3), env.t_act_move, env.t_act_shoot, env.t_any,
                               seed=17, env_offset=env_offset)
    rng = np.random.default_rng(1)
    episodes, length = np.zeros(E, np.int64), np.zeros(E, np.int64)
    cdf = ref.env_cdf(env)
    for s in range(steps):
        act = np.stack([rng.choice(MOVES, E), np.ones(E, np.int64)], axis=1)
        _, rew, term, trunc, info = env.step(act)
        exp = o.step(act)
        length += 1
        term = term.cpu().numpy()
        assert np.array_equal(term, o.done), f"step {s}"
        assert not trunc.any()
        r = rew.cpu().numpy()
        assert np.array_equal(np.isnan(r), np.isnan(exp)) and np.array_equal(r[~np.isnan(r)], exp[~np.isnan(exp)])
        grids, pos, accu = env.grids().cpu().numpy(), env.pos.cpu().numpy(), env.accu.cpu().numpy()
        counts, done = env.counts.cpu().numpy(), env.done.cpu().numpy()
        ep, last = info["episode"].cpu().numpy(), info["last_episode_length"].cpu().numpy()
        for e in range(E):
            if term[e]:
                episodes[e] += 1
                g, p, c = ref.new_episode(seed, env_offset + e, int(episodes[e]), H, W, cdf)
                assert last[e] == length[e], f"step {s} env {e}"
                assert counts[e].tolist() == c
                o.grids[e], o.pos[e], o.accu[e], o.done[e] = g.astype(np.int64), p, 0.0, False
                length[e] = 0
            assert np.array_equal(grids[e], o.grids[e]), f"step {s} env {e}"
            assert tuple(pos[e]) == tuple(o.pos[e]) and accu[e] == o.accu[e] and done[e] == 0, f"step {s} env {e}"
            assert ep[e] == episodes[e]
        o.rng_step[:] = env.rng_step.cpu().numpy().view(np.uint32)
    return episodes


@pytest.mark.parametrize("E,N,fused", [(6, 32, False), (3, 256, True), (3, 512, True)])
def test_autoreset_episode_chain_matches_oracle(device, E, N, fused):
    """p_tree = 0: the grid is EMPTY but for the one FIRE cell, which dies at the first CA step, so every env finishes
    within two steps and autoreset starts its next episode: 40 steps are a chain of at least 20 episodes per env."""
    kw = dict(t_move=0.4, t_shoot=0.3) if fused else {}
    env = _env(E, N, N, device, p_tree=0.0, p_empty=1.0, autoreset=True, **kw)
    assert env.fused == fused and env.max_passes == (1 if fused else 2)
    env.reset(seed=5)
    episodes = _chain(env, 5, 40)
    assert (episodes >= 3).all(), episodes


def test_autoreset_chain_with_trees_matches_oracle(device):
    env = _env(3, 256, 256, device, p_tree=0.5, p_empty=0.1, autoreset=True, t_move=0.4, t_shoot=0.3)
    env.reset(seed=5)
    episodes = _chain(env, 5, 60)
    assert episodes.sum() >= 1, episodes


def test_time_limit_truncates(device):
    import torch

    E, H, W = 4, 16, 256
    env = _env(E, H, W, device, autoreset=True, max_episode_steps=5)
    twin = _env(E, H, W, device)
    env.reset(seed=5)
    twin.reset(seed=5)
    rng = np.random.default_rng(3)
    for s in range(1, 6):
        act = _random_actions(rng, E)
        _, rew, term, trunc, info = env.step(act)
        _, rew2, term2, _, _ = twin.step(act)
        assert torch.equal(rew, rew2) and torch.equal(term, term2) and not term.any()
        if s < 5:
            assert not trunc.any() and torch.equal(env.grids(), twin.grids())
            for k in STATE + ("rng_step",):
                assert torch.equal(getattr(env, k), getattr(twin, k)), k
            assert (env.episode == 0).all()
    assert trunc.all() and not term.any()
    assert (env.steps_elapsed == 0).all() and (env.episode == 1).all() and (env.last_episode_length == 5).all()
    assert torch.equal(env.rng_step, twin.rng_step)
    for e in range(E):
        g, p, c = ref.new_episode(5, e, 1, H, W, ref.env_cdf(env))
        assert np.array_equal(env.grids()[e].cpu().numpy(), g) and env.counts[e].tolist() == c


@pytest.mark.parametrize("H,W", [(32, 32), (8, 256)])
def test_sharded_autoreset_reproduces_the_unsharded_envs(device, H, W):
    import torch

    kw = dict(p_tree=0.0, p_empty=1.0, autoreset=True, t_move=0.4, t_shoot=0.3)
    full = _env(6, H, W, device, **kw)
    shards = [_env(3, H, W, device, env_offset=off, **kw) for off in (0, 3)]
    for env in [full] + shards:
        env.reset(seed=5)
    rng = np.random.default_rng(4)
    for s in range(8):
        act = np.stack([rng.choice(MOVES, 6), np.ones(6, np.int64)], axis=1)
        outs = [full.step(act)] + [sh.step(act[3 * i:3 * i + 3]) for i, sh in enumerate(shards)]
        for j in (1, 2):  # reward and terminated
            assert torch.equal(torch.nan_to_num(outs[0][j]), torch.nan_to_num(torch.cat([outs[1][j], outs[2][j]])))
        assert torch.equal(full.grids(), torch.cat([sh.grids() for sh in shards]))
        for k in STATE + ("rng_step", "episode", "last_episode_length"):
            assert torch.equal(getattr(full, k), torch.cat([getattr(sh, k) for sh in shards])), f"step {s}: {k}"
    assert (full.episode >= 2).all()


def test_autoreset_graph_replay_equals_eager(device):
    """A linear graph of 4 step_random + reset launches replays as the eager calls do."""
    import torch

    from gymca_amd.graph import StepGraph

    E, G = 8, 4
    envs = [_env(E, 16, 256, device, p_tree=0.0, p_empty=1.0, autoreset=True, t_move=0.4, t_shoot=0.3,
                 materialize_obs=False) for _ in range(2)]
    for env in envs:
        env.reset(seed=3)
    graph = StepGraph(lambda: envs[0].step_random(9), n_steps=G, device=device, warmup=1)
    envs[1].step_random(9)  # the graph's one eager warm-up step
    for _ in range(2):
        graph.replay()
        for _ in range(G):
            envs[1].step_random(9)
    torch.cuda.synchronize(device)
    a, b = envs
    assert torch.equal(a.grids(), b.grids())
    for k in STATE + ("rng_step", "episode", "last_episode_length", "_terminated", "_truncated_u8"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(torch.nan_to_num(a.reward), torch.nan_to_num(b.reward))
    assert (a.episode > 0).any()


def test_errors(device):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd import _lib

    E = 3
    env = _env(E, 8, 256, device, autoreset=True, t_move=0.4, t_shoot=0.3)
    env.reset(seed=5)
    before = ref.env_state(env)
    for bad in (torch.ones(E, dtype=torch.int32, device=device), torch.ones(E + 1, dtype=torch.uint8, device=device),
                torch.ones(E, dtype=torch.uint8), np.ones(E, np.int64), np.ones((E, 1), np.uint8)):
        with pytest.raises(ValueError, match="mask"):
            env.reset_where(bad)
    for bad in (-1, 2**32, 1.5):
        with pytest.raises(ValueError, match="episode"):
            env.reset_where(episode=bad)
    with pytest.raises(ValueError, match="autoreset"):
        env.rollout_random(2)
    with pytest.raises(ValueError, match="autoreset"):
        _env(E, 8, 256, device, max_episode_steps=5, t_move=0.4, t_shoot=0.3).rollout_random(2)
    with pytest.raises(ValueError):
        _env(E, 8, 256, device, max_episode_steps=0)
    # a null `done` through the raw ABI: GCA_ERR_ARG (1) before any launch
    one = dev.ptr(env.hit)
    status = _lib.load().gca_bulldozer_reset_where(env.params, 5, None, 0, -1, dev.ptr(env._reset_cdf),
                                                   dev.ptr(env._reset_vals), None, one, one, one, one, one, one,
                                                   dev.ptr(env.buf[0]), dev.ptr(env.buf[1]), 8, 256, one, one, one, one,
                                                   E, dev.stream_ptr(device))
    assert status == 1 and b"null" in _lib.load().gca_last_error()
    ref.assert_states_equal(ref.env_state(env), before, "after refused calls")
