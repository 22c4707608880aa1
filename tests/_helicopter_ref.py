"""numpy restatement of one batched ForestFireHelicopter env step (gca_helicopter_step), test infrastructure only:
the draws from oracle.philox, the cell rule of oracle.drossel.ds_step (ca_DrosselSchwabl.py:32-66), Move / Modify of
move_modify.py:37-134, the freeze countdown of helicopter.py:220-236 and the reward of helicopter.py:120-135.
Not imported by the product. Also: the state layout shared by the tests and a driver of the host build."""
import numpy as np

from oracle import philox

TAG_ACTION = 0x41435449
TAG_DS_CELL = 0x44534345
UP, DOWN, LEFT, RIGHT = {0, 1, 2}, {6, 7, 8}, {0, 3, 6}, {2, 5, 8}
STATE_KEYS = ("buf", "parity", "freeze", "pos", "counts", "rng_step", "hit", "reward", "steps_elapsed")


def make_state(grids, thresholds, max_freeze, pos=None, freeze=None, rng_step=0):
    """Host state arrays in the device layout; env e's grid is buf[parity[e], e]."""
    g = np.ascontiguousarray(grids, dtype=np.uint8)
    E, H, W = g.shape
    buf = np.zeros((2, E, H, W), np.uint8)
    buf[0] = g
    counts = np.stack([(g == v).reshape(E, -1).sum(1) for v in (0, 1, 2)], axis=1).astype(np.int32)
    return {
        "buf": buf,
        "parity": np.zeros(E, np.uint8),
        "freeze": np.broadcast_to(np.asarray(max_freeze if freeze is None else freeze, np.int32), (E,)).copy(),
        "pos": (np.tile(np.array([[H // 2, W // 2]], np.int32), (E, 1)) if pos is None
                else np.ascontiguousarray(pos, dtype=np.int32).reshape(E, 2).copy()),
        "counts": counts,
        "rng_step": np.broadcast_to(np.asarray(rng_step, np.uint32), (E,)).copy(),
        "hit": np.zeros(E, np.uint8),
        "reward": np.zeros(E, np.float64),
        "steps_elapsed": np.zeros(E, np.int64),
        "thresholds": np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, np.float64), (E, 2))),
    }


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def current_grids(s):
    E = s["parity"].shape[0]
    return s["buf"][s["parity"].astype(np.int64), np.arange(E)]


def assert_states_equal(a, b, where=""):
    for k in STATE_KEYS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == "reward":  # bit for bit
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), f"{where}: {k} differs"


def move(a, r, c, H, W):
    """Move.update: the four set tests in order, each against the bounds of the starting position."""
    vu, vd, vl, vr = r > 0, r < H - 1, c > 0, c < W - 1
    if a in UP and vu:
        r -= 1
    if a in DOWN and vd:
        r += 1
    if a in LEFT and vl:
        c -= 1
    if a in RIGHT and vr:
        c += 1
    return r, c


def ca_step(grid, thr_fire, thr_tree, seed, env_id, step, empty=0, tree=1, fire=2):
    """One Drossel-Schwabl step with u = u01_f64 of Philox((cell, env_id, step, DSCE), seed) for the cells that draw."""
    g = np.asarray(grid)
    H, W = g.shape
    ctr = np.zeros((H * W, 4), np.uint64)
    ctr[:, 0] = np.arange(H * W)
    ctr[:, 1] = env_id & 0xFFFFFFFF
    ctr[:, 2] = int(step) & 0xFFFFFFFF
    ctr[:, 3] = TAG_DS_CELL
    x = philox.philox4x32_10(ctr, philox.seed_key(seed))
    u = philox.u01_f64(x[:, 0], x[:, 1]).reshape(H, W)
    pad = np.full((H + 2, W + 2), empty, dtype=g.dtype)
    pad[1:-1, 1:-1] = g
    nb = np.zeros((H, W), bool)
    for dr in (0, 1, 2):
        for dc in (0, 1, 2):
            if (dr, dc) != (1, 1):
                nb |= pad[dr:dr + H, dc:dc + W] == fire
    out = g.copy()
    is_tree, is_empty = g == tree, g == empty
    out[is_tree & nb] = fire
    out[is_tree & ~nb & (u < thr_fire)] = fire
    out[is_empty & (u < thr_tree)] = tree
    out[g == fire] = empty
    return out


def ref_step(s, action, max_freeze, seed, env_offset, action_seed=0):
    """One env step of every env, in place on the state `s`. action: (E,) ints or None (the random policy).
    Returns the actions taken (unclamped)."""
    E, H, W = s["buf"].shape[1:]
    n = float(H * W)
    taken = np.zeros(E, np.int32)
    for e in range(E):
        rs = int(s["rng_step"][e])
        env_id = (env_offset + e) & 0xFFFFFFFF
        if action is None:
            x = philox.philox4x32_10(np.array([0, env_id, rs, TAG_ACTION], np.uint64), philox.seed_key(action_seed))
            act = int(philox.randint_ms(x[0], 0, 9))
        else:
            act = int(action[e])
        taken[e] = act
        r, c = move(min(max(act, 0), 8), int(s["pos"][e, 0]), int(s["pos"][e, 1]), H, W)
        s["pos"][e] = (r, c)
        p = int(s["parity"][e])
        hit = 0
        if s["freeze"][e] == 0:
            g = ca_step(s["buf"][p, e], s["thresholds"][e, 0], s["thresholds"][e, 1], seed, env_id, rs)
            if g[r, c] == 2:
                g[r, c] = 0
                hit = 1
            s["buf"][p ^ 1, e] = g
            s["parity"][e] = p ^ 1
            s["freeze"][e] = max_freeze
            s["counts"][e] = [(g == 0).sum(), (g == 1).sum(), (g == 2).sum()]
        else:
            g = s["buf"][p, e]
            if g[r, c] == 2:
                g[r, c] = 0
                hit = 1
                s["counts"][e, 0] += 1
                s["counts"][e, 2] -= 1
            s["freeze"][e] -= 1
        s["hit"][e] = hit
        s["reward"][e] = np.float64(s["counts"][e, 1]) / np.float64(n) - np.float64(s["counts"][e, 2]) / np.float64(n)
        s["rng_step"][e] = (rs + 1) & 0xFFFFFFFF
        s["steps_elapsed"][e] += 1
    return taken


def host_step(s, action, max_freeze, seed, env_offset, action_seed=0, action_out=None):
    """The host build's gca_helicopter_step, in place on the state `s` (action None: the random policy)."""
    from gymca_amd import _lib

    E, H, W = s["buf"].shape[1:]
    a = None if action is None else np.ascontiguousarray(action, dtype=np.int32)
    p = lambda x: x.ctypes.data
    _lib.call_cpu("gca_helicopter_step", 0, 1, 2, int(max_freeze), int(seed) & (2**64 - 1), int(env_offset),
                  None if a is None else p(a), int(action_seed) & (2**64 - 1),
                  None if action_out is None else p(action_out), p(s["thresholds"]), p(s["freeze"]),
                  p(s["rng_step"]), p(s["parity"]), p(s["buf"][0]), p(s["buf"][1]), H, W, p(s["pos"]), p(s["counts"]),
                  p(s["hit"]), p(s["reward"]), p(s["steps_elapsed"]), None, E, None)
