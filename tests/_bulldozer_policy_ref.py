"""What is the bulldozer's own about its policy (include/gca.h "bulldozer policy"): the Philox key of its two action
draws, the sampling rule over its two heads, a driver of the host build's act entry point, and the cases that hold its
trunk against the helicopter's. The network itself, its float64 bound and the head rule are _policy_ref's, passed on
under the names the tests use. Test infrastructure only: the product never imports it."""
import ctypes
import functools

import numpy as np

from oracle import philox

import _policy_ref as P
from _policy_ref import dims, outputs_f64, outputs_ref, policy_struct  # noqa: F401

AGENT = P.BULLDOZER
TAG_BPOLICY = AGENT.tag
N_OUT = AGENT.n_out
SHAPES = AGENT.shapes
make_weights = functools.partial(P.make_weights, n_out=N_OUT)  # (d, seed=0, scale=1.0, head=1.0)


def weights_from_helicopter(wh, seed=0):
    """Bulldozer weights that share a helicopter network's trunk: the hidden layer as it is, the nine logit columns of
    w_out / b2 in columns 0..8, the value column in column 11, and arbitrary shoot columns 9..10."""
    rng = np.random.default_rng(seed)
    Hd = wh["w_out"].shape[0]
    w_out = rng.standard_normal((Hd, N_OUT)).astype(np.float32)
    b2 = rng.standard_normal(N_OUT).astype(np.float32)
    w_out[:, :9], w_out[:, 11] = wh["w_out"][:, :9], wh["w_out"][:, 9]
    b2[:9], b2[11] = wh["b2"][:9], wh["b2"][9]
    return {"w_local": wh["w_local"], "w_coarse": wh["w_coarse"], "b1": wh["b1"], "w_out": w_out, "b2": b2}


# the two ends of the helicopter's and the bulldozer's SHAPES in one: the smallest and the largest network on grids
# both agents' kernels take
TRUNK_SHAPES = [(0, 8, 32, 32, 256), (31, 32, 256, 64, 256)]


def trunk_case(shape, E=3):
    """(d, helicopter weights, bulldozer weights sharing their trunk, local, coarse) for the tests that hold the two
    agents' act entry points against each other."""
    import _policy_obs_ref as obs

    r, B, Hd, H, W = shape
    d = dims(*shape)
    wh = P.make_weights(d, P.HELICOPTER.n_out, seed=Hd, head=2.0)
    buf, parity, _ = obs.make_case(E, H, W, B)
    local, coarse = obs.host_observe(buf, parity, obs.positions(E, H, W), obs.CODES, r, B)
    return d, wh, weights_from_helicopter(wh, seed=Hd + 1), local, coarse


def assert_same_trunk(heli, bdz):
    """heli = (action (E,), logits (E, 9), value (E,)), bdz = (action (E, 2), logits (E, 11), value (E,)), host arrays."""
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(bits(heli[1]), bits(bdz[1][:, :9])), "the nine logits"
    assert np.array_equal(bits(heli[2]), bits(bdz[2])), "the value"
    assert np.array_equal(heli[0], bdz[0][:, 0]), "the move"
    assert np.isfinite(heli[1]).all() and len(np.unique(bits(heli[1]))) > heli[1].shape[0]  # nothing left unwritten


def policy_u(seed, env_ids, steps_elapsed, episode):
    """(u_move, u_shoot): u01_f32 of words 0 and 1 of Philox(((uint32)steps_elapsed, env id, episode, BPOL), seed)."""
    n = len(env_ids)
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0] = np.asarray(steps_elapsed).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 1] = np.asarray(env_ids).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 2] = np.asarray(episode).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 3] = TAG_BPOLICY
    x = philox.philox4x32_10(ctr, philox.seed_key(seed))
    return P.u01(x[:, 0]), P.u01(x[:, 1])


def sample_ref(logits, u_move, u_shoot, rel=1e-5):
    """(action (n, 2), near (n,)): P.sample_head on the nine move logits and on the two shoot logits; near if either
    head is."""
    l = np.asarray(logits).reshape(-1, 11)
    move, near_m = P.sample_head(l[:, :9], u_move, rel)
    shoot, near_s = P.sample_head(l[:, 9:11], u_shoot, rel)
    return np.stack([move, shoot], 1), near_m | near_s


def greedy_ref(logits):
    l = np.asarray(logits).reshape(-1, 11)
    return np.stack([P.greedy_head(l[:, :9]), P.greedy_head(l[:, 9:11])], 1)


# ------------------------------------------------------------------ the host build
def host_act(w, d, local, coarse, steps_elapsed, episode=None, env_offset=0, seed=0, greedy=False, want_logits=True,
             want_value=True, C=None):
    """gca_bulldozer_policy_act of the host build: (action (E, 2), logits (E, 11) | None, value (E,) | None)."""
    from gymca_amd import _lib

    s, keep = policy_struct(w, d)
    E = local.shape[0]
    local = np.ascontiguousarray(local, dtype=np.uint8)
    coarse = np.ascontiguousarray(coarse, dtype=np.float32)
    se = np.ascontiguousarray(steps_elapsed, dtype=np.int64)
    ep = None if episode is None else np.ascontiguousarray(episode, dtype=np.uint32)
    action = np.full((E, 2), -7, np.int32)
    logits = np.full((E, 11), np.nan, np.float32) if want_logits else None
    value = np.full(E, np.nan, np.float32) if want_value else None
    p = lambda x: None if x is None else x.ctypes.data
    _lib.call_cpu("gca_bulldozer_policy_act", ctypes.byref(s), d["C"] if C is None else C, p(local), p(coarse), p(se),
                  p(ep), int(env_offset), int(seed) & (2**64 - 1), 1 if greedy else 0, p(action), p(logits), p(value),
                  E, None)
    return action, logits, value
