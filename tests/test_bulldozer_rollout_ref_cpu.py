"""CPU: the numpy restatement of BatchedForestFireBulldozerEnv.rollout (tests/_bulldozer_rollout_ref.py: K x (the oracle's
env step, then the restated per-env reset)) against itself -- K steps equal K1 + K2 steps -- and against flags worked
out by hand on grids without trees. tests/test_gpu_bulldozer_rollout.py pins the device rollout to it."""
import numpy as np

import _bulldozer_reset_ref as rref
import _bulldozer_rollout_ref as ref

WIND = np.array([[0.3, 0.6, 0.2], [0.5, 0.0, 0.4], [0.1, 0.7, 0.35]])
T = dict(t_move=0.4, t_shoot=0.3, t_any=0.001)


def _actions(rng, K, E):
    return np.stack([rng.integers(0, 9, (K, E)), rng.integers(0, 2, (K, E))], axis=2)


def _run(s, actions, cdf, **kw):
    return ref.ref_rollout(s, actions, WIND, T["t_move"], T["t_shoot"], T["t_any"], seed=17, reset_seed=5, cdf=cdf,
                           **kw)


def test_k_steps_equal_k1_plus_k2_steps():
    E, H, W, K = 4, 12, 20, 14
    cdf = rref.cdf_of(0.1, 0.5)
    a = ref.make_state(E, H, W, seed=3, p=(0.3, 0.68, 0.02))
    a["done"][1] = 1
    b, ep0 = ref.copy_state(a), a["episode"].copy()
    act = _actions(np.random.default_rng(1), K, E)
    kw = dict(env_offset=2, autoreset=True, max_steps=5)
    whole = _run(a, act, cdf, **kw)
    first, second = _run(b, act[:6], cdf, **kw), _run(b, act[6:], cdf, **kw)
    ref.assert_states_equal(a, b, "K = 6 + 8")
    for w, f, g in zip(whole, first, second):
        assert np.array_equal(w, np.concatenate([f, g]), equal_nan=True)
    assert whole[2].sum() >= 2 and (a["episode"] > ep0).all()  # the time limit truncated, episodes moved on
    # autoreset off: a finished env stays finished, the limit is ignored
    c = ref.make_state(E, H, W, seed=3, p=(0.3, 0.68, 0.02))
    c["done"][1] = 1
    ep = c["episode"].copy()
    rew, term, trunc = _run(c, act, cdf, env_offset=2, max_steps=5)
    assert not trunc.any() and term[:, 1].all() and (rew[:, 1] == 0).all() and np.array_equal(c["episode"], ep)
    assert (c["steps_elapsed"][[0, 2, 3]] >= 5).any()


def _empty_state(E, H, W, reset_seed, cdf):
    """Episode 0 of E envs without trees: EMPTY but for the one FIRE cell."""
    s = ref.make_state(E, H, W)
    for k in ("parity", "episode", "rng_step", "steps_elapsed"):
        s[k][:] = 0
    s["accu"][:] = 0.0
    for e in range(E):
        g, pos, counts = rref.new_episode(reset_seed, e, 0, H, W, cdf)
        s["buf"][:, e], s["pos"][e], s["counts"][e] = g, pos, counts
    return s


def test_hand_computed_termination_chain():
    """p_tree = 0, move != 4 and shoot = 1 cost 0.701 time units per step: the first step of an episode runs no CA pass
    (the fire still burns: reward -1), the second runs one, the lone FIRE cell burns out (no tree, no fire: reward NaN,
    terminated) and the reset starts the next episode. Env 1 is finished on entry: a no-op step (reward 0, terminated),
    then the same chain one step late."""
    E, H, W, K = 2, 12, 24, 6
    cdf = rref.cdf_of(1.0, 0.0)
    s = _empty_state(E, H, W, 5, cdf)
    s["done"][1] = 1
    act = np.stack([np.full((K, E), 1), np.ones((K, E), np.int64)], axis=2)
    rew, term, trunc = _run(s, act, cdf, autoreset=True)
    nan = np.nan
    assert np.array_equal(term, np.array([[0, 1], [1, 0], [0, 1], [1, 0], [0, 1], [1, 0]], np.uint8))
    assert not trunc.any()
    assert np.array_equal(rew, np.array([[-1, 0], [nan, -1], [-1, nan], [nan, -1], [-1, nan], [nan, -1]]),
                          equal_nan=True)
    assert s["episode"].tolist() == [3, 3] and s["last_length"].tolist() == [2, 2] and not s["done"].any()
    assert s["steps_elapsed"].tolist() == [0, 1] and s["rng_step"].tolist() == [3, 2]
    assert s["terminated"].tolist() == [1, 0] and s["accu"].tolist() == [0.0, (0.4 + 0.3) + 0.001]
    for e in range(E):
        g, pos, counts = rref.new_episode(5, e, 3, H, W, cdf)
        if e == 0:  # freshly reset: plane 0 holds the new episode's grid
            assert s["parity"][e] == 0 and np.array_equal(s["buf"][0, e], g) and s["counts"][e].tolist() == counts
        assert s["counts"][e].tolist() == [H * W - 1, 0, 1]


def test_hand_computed_time_limit():
    """not_move / no shot costs 0.001 time units: no CA pass, the fire burns on (reward -1, never terminated), and with
    max_steps = 3 and clocks staggered by one step env 0 is truncated at steps 2 and 5, env 1 at steps 1 and 4."""
    E, H, W, K = 2, 12, 24, 6
    cdf = rref.cdf_of(1.0, 0.0)
    s = _empty_state(E, H, W, 5, cdf)
    s["steps_elapsed"][:] = [0, 1]
    act = np.stack([np.full((K, E), 4), np.zeros((K, E), np.int64)], axis=2)
    rew, term, trunc = _run(s, act, cdf, autoreset=True, max_steps=3)
    assert not term.any() and (rew == -1.0).all()
    assert np.array_equal(trunc, np.array([[0, 0], [0, 1], [1, 0], [0, 0], [0, 1], [1, 0]], np.uint8))
    assert s["episode"].tolist() == [2, 2] and s["last_length"].tolist() == [3, 3]
    assert s["steps_elapsed"].tolist() == [0, 1] and s["rng_step"].tolist() == [0, 0]
    assert s["truncated"].tolist() == [1, 0] and s["accu"].tolist() == [0.0, 0.001]
