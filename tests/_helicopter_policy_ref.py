"""What is the helicopter's own about its policy (include/gca.h "helicopter policy"): the Philox key of its action
draw, the sampling rule over its one head, drivers of the host build's act and rollout entry points and the record
helpers the CPU and GPU tests share. The network itself, its float64 bound and the head rule are _policy_ref's, passed
on under the names the tests use. Test infrastructure only: the product never imports it."""
import ctypes
import functools

import numpy as np

from oracle import philox

import _helicopter_ref as href
import _policy_obs_ref as obs
import _policy_ref as P
from _policy_ref import dims, outputs_f64, outputs_ref, policy_struct  # noqa: F401

AGENT = P.HELICOPTER
TAG_POLICY = AGENT.tag
SHAPES = AGENT.shapes
make_weights = functools.partial(P.make_weights, n_out=AGENT.n_out)  # (d, seed=0, scale=1.0, head=1.0)


def policy_u(seed, env_ids, rng_steps):
    """u01_f32(x.x) of Philox((0, env id, rng_step, POLI), seed): float32 in [0, 1)."""
    n = len(env_ids)
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 1] = np.asarray(env_ids, np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 2] = np.asarray(rng_steps, np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 3] = TAG_POLICY
    return P.u01(philox.philox4x32_10(ctr, philox.seed_key(seed))[:, 0])


def sample_ref(logits, u, rel=1e-5):
    """(action, near) of P.sample_head on the nine logits."""
    return P.sample_head(np.asarray(logits).reshape(-1, 9), u, rel)


def greedy_ref(logits):
    return P.greedy_head(np.asarray(logits).reshape(-1, 9))


# ------------------------------------------------------------------ the host build
def host_act(w, d, local, coarse, rng_step, env_offset=0, seed=0, greedy=False, want_logits=True, want_value=True,
             C=None):
    """gca_helicopter_policy_act of the host build: (action (E,), logits (E, 9) | None, value (E,) | None)."""
    from gymca_amd import _lib

    s, keep = policy_struct(w, d)
    E = local.shape[0]
    local = np.ascontiguousarray(local, dtype=np.uint8)
    coarse = np.ascontiguousarray(coarse, dtype=np.float32)
    rs = np.ascontiguousarray(rng_step, dtype=np.uint32)
    action = np.full(E, -7, np.int32)
    logits = np.full((E, 9), np.nan, np.float32) if want_logits else None
    value = np.full(E, np.nan, np.float32) if want_value else None
    p = lambda x: None if x is None else x.ctypes.data
    _lib.call_cpu("gca_helicopter_policy_act", ctypes.byref(s), d["C"] if C is None else C, p(local), p(coarse), p(rs),
                  int(env_offset), int(seed) & (2**64 - 1), 1 if greedy else 0, p(action), p(logits), p(value), E, None)
    return action, logits, value


RECORDS = ("action", "logits", "value", "reward", "hit", "local", "coarse")


def empty_records(d, K, E, names=RECORDS):
    shapes = {"action": ((K, E), np.int32), "logits": ((K, E, 9), np.float32), "value": ((K, E), np.float32),
              "reward": ((K, E), np.float64), "hit": ((K, E), np.uint8), "local": ((K, E, d["S"], d["S"]), np.uint8),
              "coarse": ((K, E, 2, d["Hc"], d["Wc"]), np.float32)}
    return {n: np.full(shapes[n][0], 0x55, shapes[n][1]) for n in names}


def host_rollout_policy(s, w, d, K, max_freeze, seed, env_offset, policy_seed=0, greedy=False, names=RECORDS,
                        overrides=None):
    """gca_helicopter_policy_rollout of the host build, in place on the state `s` (_helicopter_ref layout). Returns the
    records named in `names`."""
    from gymca_amd import _lib

    st, keep = policy_struct(w, d)
    E, H, W = s["buf"].shape[1:]
    rec = empty_records(d, max(K, 0), E, names)
    p = lambda x: None if x is None else x.ctypes.data
    ptrs = {k: p(s[k]) for k in ("thresholds", "freeze", "rng_step", "parity", "pos", "counts", "hit", "reward",
                                 "steps_elapsed")}
    ptrs["buf0"], ptrs["buf1"] = p(s["buf"][0]), p(s["buf"][1])
    ptrs.update(overrides or {})
    _lib.call_cpu("gca_helicopter_policy_rollout", 0, 1, 2, int(max_freeze), int(seed) & (2**64 - 1), int(env_offset),
                  ctypes.byref(st), int(policy_seed) & (2**64 - 1), 1 if greedy else 0, int(K),
                  *[p(rec.get(n)) for n in RECORDS], None, ptrs["thresholds"], ptrs["freeze"], ptrs["rng_step"],
                  ptrs["parity"], ptrs["buf0"], ptrs["buf1"], H, W, ptrs["pos"], ptrs["counts"], ptrs["hit"],
                  ptrs["reward"], ptrs["steps_elapsed"], E, None)
    return rec


def host_observe(s, d):
    """(local, coarse) of the state `s` by the host build's gca_policy_observation."""
    return obs.host_observe(s["buf"], s["parity"], s["pos"], obs.HELI_CODES, d["radius"], d["block"])


def host_k_steps(s, w, d, K, max_freeze, seed, env_offset, policy_seed=0, greedy=False):
    """K x (host observation, host act, host step), in place on `s`; the records as the rollout defines them."""
    E = s["buf"].shape[1]
    rec = empty_records(d, K, E)
    for k in range(K):
        lo, co = host_observe(s, d)
        act, lg, va = host_act(w, d, lo, co, s["rng_step"], env_offset, policy_seed, greedy)
        href.host_step(s, act, max_freeze, seed, env_offset)
        rec["local"][k], rec["coarse"][k], rec["action"][k], rec["logits"][k], rec["value"][k] = lo, co, act, lg, va
        rec["reward"][k], rec["hit"][k] = s["reward"], s["hit"]
    return rec


def assert_records_equal(a, b, where=""):
    for n in a:
        x, y = np.asarray(a[n]), np.asarray(b[n])
        assert x.shape == y.shape and x.dtype == y.dtype, f"{where}: {n} shape / dtype"
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{where}: record {n} differs"  # as bits


def grids(E, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 3, (E, H, W)).astype(np.uint8)
