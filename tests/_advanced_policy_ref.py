"""gca_advanced_policy_act (include/gca.h "advanced policy") for the tests: the cases the CPU and the GPU tests share, the
composition of the two numpy restatements it is defined by (_policy_obs_ref, then _bulldozer_policy_ref on the widened
time_step) and a driver of the host build's entry point. Test infrastructure only: the product never imports it."""
import ctypes

import numpy as np

import _bulldozer_policy_ref as bref
import _policy_obs_ref as obs

CODES = (0, 1, 2)  # the Advanced env's (empty, tree, fire)
SEED = 0x0ADC0FFEE123
SENTINEL = -77     # what the caller keeps in the action's third column
# (E, H, W, block, radius, hidden) of the host test; the GPU test's first and seventh case
HOST_SHAPES = [(3, 32, 256, 8, 5, 64), (2, 24, 40, 4, 3, 32)]


def positions(E, H, W):
    """A corner, a position outside the grid (the window then misses the grid on two sides, or altogether) and the
    middle, in turn."""
    three = [(0, 0), (H + 1, -2), (H // 2, W // 2)]
    return np.array([three[e % 3] for e in range(E)], np.int32)


def make_case(shape, seed=0):
    """(d, w, planes u8 (E, H, W), pos i32 (E, 2), time_step i32 (E,)): cells drawn from the three codes and a fourth
    one, env 0's first block all FIRE and the last env's last block all TREE; time steps all different, one negative
    (the key takes its low 32 bits)."""
    E, H, W, B, r, Hd = shape
    d = bref.dims(r, B, Hd, H, W)
    w = bref.make_weights(d, seed=seed + Hd)
    rng = np.random.default_rng(seed + 1000 * H + W)
    vals = np.array(list(CODES) + [obs.OTHER], np.uint8)
    planes = rng.choice(vals, size=(E, H, W), p=[0.2, 0.4, 0.3, 0.1])
    planes[0, :B, :B] = CODES[2]
    planes[E - 1, (d["Hc"] - 1) * B:, (d["Wc"] - 1) * B:] = CODES[1]
    ts = np.array([1, 401, -3, 77, 12345], np.int32)[:E]
    return d, w, np.ascontiguousarray(planes), positions(E, H, W), ts


def observe_ref(planes, pos, r, B):
    """(local, coarse) of _policy_obs_ref.ref, for positions anywhere: a window cell that misses the grid is class 3."""
    E, H, W = planes.shape
    S = 2 * r + 1
    _, tree, fire = CODES
    inside = np.stack([np.clip(pos[:, 0], 0, H - 1), np.clip(pos[:, 1], 0, W - 1)], 1)
    loc_in, coarse = obs.ref(planes, inside, CODES, r, B)
    cls = np.where(planes == tree, 1, np.where(planes == fire, 2, 0)).astype(np.uint8)
    local = np.full((E, S, S), 3, np.uint8)
    for e in range(E):
        rows = int(pos[e, 0]) - r + np.arange(S)
        cols = int(pos[e, 1]) - r + np.arange(S)
        ok = ((rows >= 0) & (rows < H))[:, None] & ((cols >= 0) & (cols < W))[None, :]
        g = cls[e][np.clip(rows, 0, H - 1)[:, None], np.clip(cols, 0, W - 1)[None, :]]
        local[e] = np.where(ok, g, 3)
        if (inside[e] == pos[e]).all():
            assert np.array_equal(local[e], loc_in[e])  # the restatement's own window wherever it has one
    return local, coarse


def composed(d, w, planes, pos, ts, env_offset=0, seed=SEED, greedy=False):
    """The contract's right-hand side: observation, then the bulldozer policy on (int64)time_step with no episode.
    Returns (action, logits, value, local, coarse, out32): the action and outputs of the host build's
    gca_bulldozer_policy_act on the restated observation, and the float32 restatement of the twelve outputs."""
    local, coarse = observe_ref(planes, pos, d["radius"], d["block"])
    out32, _ = bref.outputs_ref(w, d, local, coarse)
    action, logits, value = bref.host_act(w, d, local, coarse, ts.astype(np.int64), None, env_offset=env_offset,
                                          seed=seed, greedy=greedy)
    return action, logits, value, local, coarse, out32


ORDER = ("policy", "grid", "pos", "time_step", "E", "H", "W", "empty", "tree", "fire", "env_offset", "policy_seed",
         "greedy", "action", "action_stride", "logits", "value", "local_out", "coarse_out", "stream")


def host_act(d, w, planes, pos, ts, env_offset=0, seed=SEED, greedy=False, stride=2, logits=True, value=True, local=True,
             coarse=True):
    """gca_advanced_policy_act of the host build: (action (E, stride), logits, value, local, coarse), None for an
    output passed as NULL. The action starts as SENTINEL everywhere."""
    from gymca_amd import _lib

    s, keep = bref.policy_struct(w, d)
    E, H, W = planes.shape
    action = np.full((E, stride), SENTINEL, np.int32)
    lg = np.full((E, 11), np.nan, np.float32) if logits else None
    va = np.full(E, np.nan, np.float32) if value else None
    lo = np.full((E, d["S"], d["S"]), 0xAA, np.uint8) if local else None
    co = np.full((E, 2, d["Hc"], d["Wc"]), -1.0, np.float32) if coarse else None
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    ts = np.ascontiguousarray(ts, dtype=np.int32)
    p = lambda x: None if x is None else x.ctypes.data
    _lib.call_cpu("gca_advanced_policy_act", ctypes.byref(s), p(planes), p(pos), p(ts), E, H, W, *CODES,
                  int(env_offset), int(seed) & (2**64 - 1), 1 if greedy else 0, p(action), stride, p(lg), p(va), p(lo),
                  p(co), None)
    return action, lg, va, lo, co


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
