"""numpy restatement of gca_bulldozer_rollout (BatchedForestFireBulldozerEnv.rollout): K x (the CPU oracle of the env
step, oracle.windy.BulldozerOracle.step, then -- under autoreset -- the restatement of the per-env reset,
_bulldozer_reset_ref.ref_reset_where with mask=None) over a state dict. Test infrastructure only.

A state is _bulldozer_reset_ref's dict (both grid planes, parity, done, hit, terminated, truncated, accu, pos, counts,
steps_elapsed, last_length, episode) plus rng_step (E,) u32, steps (E,) i32 and reward (E,) f64."""
import numpy as np

import _bulldozer_reset_ref as rref
from oracle import windy as owindy

FIELDS = rref.FIELDS + ("rng_step", "steps", "reward")
ENV_FIELDS = dict(rref.ENV_FIELDS, rng_step="rng_step", steps="steps", reward="reward")


def env_state(env):
    """The batched env's tensors as a state dict (host copies; episode and rng_step as uint32)."""
    s = {k: getattr(env, attr).cpu().numpy().copy() for k, attr in ENV_FIELDS.items()}
    s["episode"] = s["episode"].view(np.uint32)
    s["rng_step"] = s["rng_step"].view(np.uint32)
    return s


def make_state(E, H, W, seed=0, p=(0.1, 0.6, 0.3)):
    """A mid-episode state: consistent counts, both planes holding the grid, random clocks and fractions of time."""
    rng = np.random.default_rng(seed)
    g = rng.choice(np.array(rref.CODES, np.uint8), size=(E, H, W), p=p)
    return {
        "buf": np.stack([g, g]),
        "parity": rng.integers(0, 2, E).astype(np.uint8),
        "done": np.zeros(E, np.uint8),
        "hit": np.zeros(E, np.uint8),
        "terminated": np.zeros(E, np.uint8),
        "truncated": np.zeros(E, np.uint8),
        "accu": rng.random(E) * 0.9,
        "pos": np.stack([rng.integers(0, H, E), rng.integers(0, W, E)], axis=1).astype(np.int32),
        "counts": np.stack([(g == v).sum(axis=(1, 2)) for v in rref.CODES], axis=1).astype(np.int32),
        "steps_elapsed": rng.integers(0, 4, E).astype(np.int64),
        "last_length": np.zeros(E, np.int64),
        "episode": rng.integers(0, 3, E).astype(np.uint32),
        "rng_step": rng.integers(0, 100, E).astype(np.uint32),
        "steps": np.zeros(E, np.int32),
        "reward": np.zeros(E, np.float64),
    }


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def ref_step(s, action, wind, t_move, t_shoot, t_any, seed, env_offset=0):
    """One env step of every env, in place: the oracle on the envs' current grids, written back as the device keeps
    them (a CA pass writes the other plane and flips the parity, Modify patches the current plane; a finished env takes
    the no-op step: reward 0, steps -1, nothing else)."""
    _, E, H, W = s["buf"].shape
    par = s["parity"].astype(np.int64)
    o = owindy.BulldozerOracle([s["buf"][par[e], e] for e in range(E)], s["pos"], np.asarray(wind).reshape(3, 3),
                               t_move, t_shoot, t_any, seed=seed, env_offset=env_offset)
    o.accu[:] = s["accu"]
    o.rng_step[:] = s["rng_step"]
    o.done[:] = s["done"] != 0
    live = ~o.done.copy()
    rew = o.step(np.asarray(action))
    for e in range(E):
        if not live[e]:
            s["steps"][e] = -1
            continue
        n = int(o.rng_step[e]) - int(s["rng_step"][e])
        assert n in (0, 1)
        if n:
            s["parity"][e] ^= 1
        g = o.grids[e].astype(np.uint8)
        s["buf"][s["parity"][e], e] = g
        s["steps"][e] = n
        s["counts"][e] = [int(np.sum(g == v)) for v in rref.CODES]
        s["pos"][e] = o.pos[e]
        s["hit"][e] = o.hit[e]
        s["steps_elapsed"][e] += 1
    s["accu"][:] = o.accu
    s["rng_step"][:] = (o.rng_step & 0xFFFFFFFF).astype(np.uint32)
    s["done"][:] = o.done
    s["reward"][:] = rew
    return rew


def ref_rollout(s, actions, wind, t_move, t_shoot, t_any, seed, reset_seed, cdf, env_offset=0, autoreset=False,
                max_steps=0):
    """K = len(actions) env steps in place on the state dict; returns the (K, E) records (reward f64, terminated u8,
    truncated u8): under autoreset the flags each step's reset saw, otherwise `done` after the step and zeros."""
    actions = np.asarray(actions)
    K, E = actions.shape[0], s["done"].shape[0]
    rew = np.zeros((K, E), np.float64)
    term, trunc = np.zeros((K, E), np.uint8), np.zeros((K, E), np.uint8)
    for k in range(K):
        rew[k] = ref_step(s, actions[k], wind, t_move, t_shoot, t_any, seed, env_offset)
        if autoreset:
            rref.ref_reset_where(s, reset_seed, env_offset, cdf, mask=None, max_steps=max_steps)
            term[k], trunc[k] = s["terminated"], s["truncated"]
        else:
            term[k] = s["done"]
    return rew, term, trunc


def assert_states_equal(a, b, where="", fields=FIELDS):
    for k in fields:
        assert a[k].dtype == b[k].dtype, f"{where}: {k} dtype"
        if a[k].dtype.kind == "f":
            assert np.array_equal(a[k], b[k], equal_nan=True), f"{where}: {k}"
        else:
            assert np.array_equal(a[k], b[k]), f"{where}: {k}"
