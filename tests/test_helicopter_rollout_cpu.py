"""CPU: K env steps in one call (gca_helicopter_rollout) in the host build of the C-ABI against K calls of the numpy
restatement (tests/_helicopter_ref.py ref_step) and K calls of the host gca_helicopter_step: every state tensor and the
three per-step records, exactly (rewards as bits). No GPU."""
import numpy as np
import pytest

import _helicopter_ref as ref

SEED = 0x1234ABCD5678
THR = np.array([[0.05, 0.4], [0.3, 0.3], [0.033, 0.333]])


def _grids(E, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 3, (E, H, W)).astype(np.uint8)


def host_rollout(s, actions, max_freeze, seed, env_offset, K=None, action_seed=0, action_out=None, reward_out=None,
                 hit_out=None, overrides=None):
    """The host build's gca_helicopter_rollout, in place on the state `s` (actions None: the random policy, K
    steps). `overrides` replaces named pointer arguments (the argument-error tests)."""
    from gymca_amd import _lib

    E, H, W = s["buf"].shape[1:]
    a = None if actions is None else np.ascontiguousarray(actions, dtype=np.int32)
    K = a.shape[0] if K is None else K
    p = lambda x: None if x is None else x.ctypes.data
    ptrs = {k: p(s[k]) for k in ("thresholds", "freeze", "rng_step", "parity", "pos", "counts", "hit", "reward",
                                 "steps_elapsed")}
    ptrs["buf0"], ptrs["buf1"] = p(s["buf"][0]), p(s["buf"][1])
    ptrs.update(overrides or {})
    _lib.call_cpu("gca_helicopter_rollout", 0, 1, 2, int(max_freeze), int(seed) & (2**64 - 1), int(env_offset), p(a),
                  int(action_seed) & (2**64 - 1), int(K), p(action_out), p(reward_out), p(hit_out),
                  ptrs["thresholds"], ptrs["freeze"], ptrs["rng_step"], ptrs["parity"], ptrs["buf0"], ptrs["buf1"], H,
                  W, ptrs["pos"], ptrs["counts"], ptrs["hit"], ptrs["reward"], ptrs["steps_elapsed"], E, None)


def _records(K, E):
    return (np.full((K, E), -7, np.int32), np.full((K, E), np.nan, np.float64), np.full((K, E), 9, np.uint8))


def _start(max_freeze, seed=1):
    return ref.make_state(_grids(3, 6, 9, seed), THR, max_freeze, rng_step=[0, 7, 0xFFFFFFFF])


@pytest.mark.parametrize("max_freeze", [0, 2])
def test_host_rollout_equals_k_steps(max_freeze):
    E, K, off = 3, 12, 5
    a = _start(max_freeze)
    b, c = ref.copy_state(a), ref.copy_state(a)
    actions = np.random.default_rng(2).integers(-1, 10, (K, E)).astype(np.int32)  # -1 and 9 exercise the clamp
    assert actions.min() == -1 and actions.max() == 9
    want_r, want_h = np.zeros((K, E)), np.zeros((K, E), np.uint8)
    for k in range(K):
        ref.ref_step(a, actions[k], max_freeze, SEED, off)
        ref.host_step(b, actions[k], max_freeze, SEED, off)
        ref.assert_states_equal(a, b, f"step {k}")
        want_r[k], want_h[k] = a["reward"], a["hit"]
    act_o, rew_o, hit_o = _records(K, E)
    host_rollout(c, actions, max_freeze, SEED, off, action_out=act_o, reward_out=rew_o, hit_out=hit_o)
    ref.assert_states_equal(c, a, "rollout vs K ref_step")
    ref.assert_states_equal(c, b, "rollout vs K host_step")
    assert np.array_equal(act_o, actions)
    assert np.array_equal(rew_o.view(np.uint64), want_r.view(np.uint64))
    assert np.array_equal(hit_o, want_h)
    assert (c["steps_elapsed"] == K).all() and c["rng_step"].tolist() == [12, 19, 11]  # the third wrapped


def test_host_rollout_random_policy():
    E, K, off = 3, 12, 5
    a = _start(2, seed=3)
    c = ref.copy_state(a)
    taken, want_r, want_h = np.zeros((K, E), np.int32), np.zeros((K, E)), np.zeros((K, E), np.uint8)
    for k in range(K):
        taken[k] = ref.ref_step(a, None, 2, SEED, off, action_seed=9)
        want_r[k], want_h[k] = a["reward"], a["hit"]
    act_o, rew_o, hit_o = _records(K, E)
    host_rollout(c, None, 2, SEED, off, K=K, action_seed=9, action_out=act_o, reward_out=rew_o, hit_out=hit_o)
    ref.assert_states_equal(c, a, "random rollout")
    assert np.array_equal(act_o, taken) and ((0 <= act_o) & (act_o < 9)).all() and len(np.unique(act_o)) > 3
    assert np.array_equal(rew_o.view(np.uint64), want_r.view(np.uint64)) and np.array_equal(hit_o, want_h)


def test_host_rollout_edge_cases():
    E, off = 3, 5
    actions = np.random.default_rng(4).integers(-1, 10, (12, E)).astype(np.int32)
    a = _start(2)
    before = ref.copy_state(a)
    host_rollout(a, actions[:0], 2, SEED, off, K=0)  # K = 0 changes nothing
    ref.assert_states_equal(a, before, "K = 0")
    host_rollout(a, None, 2, SEED, off, K=0)
    ref.assert_states_equal(a, before, "K = 0, random")
    one, two = ref.copy_state(a), ref.copy_state(a)
    r1, r2 = np.zeros((12, E)), np.zeros((12, E))
    host_rollout(one, actions, 2, SEED, off, reward_out=r1)  # the other records null
    host_rollout(two, actions[:5], 2, SEED, off, reward_out=r2[:5])
    host_rollout(two, actions[5:], 2, SEED, off, reward_out=r2[5:])
    ref.assert_states_equal(two, one, "5 + 7 vs 12")
    assert np.array_equal(r1.view(np.uint64), r2.view(np.uint64))
    none = ref.copy_state(a)
    host_rollout(none, actions, 2, SEED, off)  # every record null
    ref.assert_states_equal(none, one, "null records")
    assert not np.array_equal(ref.current_grids(one), ref.current_grids(before))


def test_host_rollout_refuses_bad_arguments():
    from gymca_amd import GCAError, _lib

    a = _start(2)
    before = ref.copy_state(a)
    actions = np.zeros((2, 3), np.int32)
    with pytest.raises(GCAError, match="K >= 0"):
        host_rollout(a, actions, 2, SEED, 0, K=-1)
    assert b"K >= 0" in _lib.load_cpu().gca_last_error()
    with pytest.raises(GCAError, match="null argument"):
        host_rollout(a, actions, 2, SEED, 0, overrides={"freeze": None})
    with pytest.raises(GCAError, match="must differ"):
        host_rollout(a, actions, 2, SEED, 0, overrides={"buf1": a["buf"][0].ctypes.data})
    with pytest.raises(GCAError, match="max_freeze"):
        host_rollout(a, actions, -1, SEED, 0)
    ref.assert_states_equal(a, before, "nothing ran")
