"""numpy restatement of gca_bulldozer_reset_where (the per-env reset of the batched ForestFireBulldozer env), built on
oracle.philox and gymca_amd._seeding, and a driver of the host build of the same entry point. Test infrastructure only.

A state is a dict of numpy arrays shaped like the batched env's tensors: buf (2, E, H, W) u8, parity, done, hit,
terminated, truncated (E,) u8, accu (E,) f64, pos (E, 2) i32, counts (E, 3) i32, steps_elapsed, last_length (E,) i64,
episode (E,) u32."""
import numpy as np

from gymca_amd import _seeding
from oracle import philox

TAG_INIT = 0x494E4954
CODES = (0, 3, 25)  # EMPTY, TREE, FIRE of the bulldozer env
FIELDS = ("buf", "parity", "done", "hit", "terminated", "truncated", "accu", "pos", "counts", "steps_elapsed",
          "last_length", "episode")


def cdf_of(p_empty=0.10, p_tree=0.90):
    return np.array([p_empty, p_empty + p_tree, 1.0], dtype=np.float32)


def fill_grid(seed, env_id, episode, H, W, cdf, values=CODES):
    """gca_fill_categorical's definition for one env with counter word 2 = episode: flat cell i takes word i & 3 of
    Philox((i >> 2, env_id, episode, INIT), seed), u01_f32, the first cdf[j] > u."""
    n = H * W
    quads = (n + 3) // 4
    ctr = np.zeros((quads, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(quads)
    ctr[:, 1] = env_id
    ctr[:, 2] = episode
    ctr[:, 3] = TAG_INIT
    u = philox.u01_f32(philox.philox4x32_10(ctr, philox.seed_key(seed)).reshape(-1)[:n])
    cdf = np.asarray(cdf, dtype=np.float32)
    j = np.where(u < cdf[0], 0, np.where(u < cdf[1], 1, 2))
    return np.asarray(values, dtype=np.uint8)[j].reshape(H, W)


def noise(seed, env_id, tag, n, episode):
    return int(_seeding.env_integers_episode(seed, env_id, 1, tag, 0, max(1, n // 12), episode)[0])


def fire_cell(seed, env_id, episode, H, W):
    return 3 * H // 4 + noise(seed, env_id, 1, H, episode), W // 4 + noise(seed, env_id, 2, W, episode)


def position(seed, env_id, episode, H, W):
    return H // 4 + noise(seed, env_id, 3, H, episode), 3 * W // 4 + noise(seed, env_id, 4, W, episode)


def new_episode(seed, env_id, episode, H, W, cdf, codes=CODES):
    """(grid, pos, counts) of episode `episode` of the env with global id env_id."""
    g = fill_grid(seed, env_id, episode, H, W, cdf, codes)
    g[fire_cell(seed, env_id, episode, H, W)] = codes[2]
    return g, position(seed, env_id, episode, H, W), [int(np.sum(g == v)) for v in codes]


def make_state(E, H, W, seed=0):
    """A mid-episode state with every field non-trivial, so that an untouched env shows as untouched."""
    rng = np.random.default_rng(seed)
    return {
        "buf": rng.choice(np.array(CODES, np.uint8), size=(2, E, H, W)),
        "parity": rng.integers(0, 2, E).astype(np.uint8),
        "done": np.zeros(E, np.uint8),
        "hit": rng.integers(0, 2, E).astype(np.uint8),
        "terminated": np.full(E, 7, np.uint8),
        "truncated": np.full(E, 7, np.uint8),
        "accu": rng.random(E),
        "pos": np.stack([rng.integers(0, H, E), rng.integers(0, W, E)], axis=1).astype(np.int32),
        "counts": rng.integers(0, H * W + 1, (E, 3)).astype(np.int32),
        "steps_elapsed": rng.integers(1, 50, E).astype(np.int64),
        "last_length": np.full(E, -3, np.int64),
        "episode": rng.integers(0, 5, E).astype(np.uint32),
    }


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def selected(s, mask, max_steps):
    by_limit = (s["steps_elapsed"] >= max_steps) if max_steps > 0 else np.zeros(len(s["done"]), bool)
    by_mask = (np.asarray(mask) != 0) if mask is not None else (s["done"] != 0)
    return by_mask | by_limit, by_limit


def ref_reset_where(s, seed, env_offset, cdf, mask=None, max_steps=0, set_episode=-1, codes=CODES):
    """The restatement, in place on the state dict. Returns the selection."""
    _, E, H, W = s["buf"].shape
    sel, by_limit = selected(s, mask, max_steps)
    was_done = s["done"] != 0
    s["terminated"][:] = was_done
    s["truncated"][:] = by_limit & ~was_done
    for e in np.flatnonzero(sel):
        k = int(set_episode) if set_episode >= 0 else (int(s["episode"][e]) + 1) & 0xFFFFFFFF
        g, pos, counts = new_episode(seed, env_offset + e, k, H, W, cdf, codes)
        s["buf"][0, e] = g
        s["pos"][e] = pos
        s["counts"][e] = counts
        s["last_length"][e] = s["steps_elapsed"][e]
        s["episode"][e] = k
        for name in ("parity", "accu", "done", "hit", "steps_elapsed"):
            s[name][e] = 0
    return sel


def host_reset_where(s, seed, env_offset, cdf, mask=None, max_steps=0, set_episode=-1, codes=CODES):
    """gca_bulldozer_reset_where of the host build (libgca_cpu.so), in place on the state dict."""
    from gymca_amd import _lib

    _, E, H, W = s["buf"].shape
    p = _lib.BulldozerParams()
    p.env_offset = env_offset
    p.empty, p.tree, p.fire = codes
    cdf = np.ascontiguousarray(cdf, dtype=np.float32)
    vals = np.array(codes, dtype=np.uint8)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    assert all(s[k].flags.c_contiguous for k in FIELDS)
    _lib.call_cpu("gca_bulldozer_reset_where", p, seed & (2**64 - 1), None if m is None else m.ctypes.data, max_steps,
                  set_episode, cdf.ctypes.data, vals.ctypes.data, s["done"].ctypes.data, s["terminated"].ctypes.data,
                  s["truncated"].ctypes.data, s["episode"].ctypes.data, s["last_length"].ctypes.data,
                  s["accu"].ctypes.data, s["parity"].ctypes.data, s["buf"][0].ctypes.data, s["buf"][1].ctypes.data, H,
                  W, s["pos"].ctypes.data, s["counts"].ctypes.data, s["hit"].ctypes.data,
                  s["steps_elapsed"].ctypes.data, E, None)


def assert_states_equal(a, b, where=""):
    for k in FIELDS:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), f"{where}: {k}"


# ---------------------------------------------------------------- the batched env on the device
ENV_FIELDS = {"buf": "buf", "parity": "parity", "done": "done", "hit": "hit", "terminated": "_terminated",
              "truncated": "_truncated_u8", "accu": "accu", "pos": "pos", "counts": "counts",
              "steps_elapsed": "steps_elapsed", "last_length": "last_episode_length", "episode": "episode"}


def env_state(env):
    """The batched env's tensors as a state dict (host copies; episode as uint32)."""
    s = {k: getattr(env, attr).cpu().numpy().copy() for k, attr in ENV_FIELDS.items()}
    s["episode"] = s["episode"].view(np.uint32)
    return s


def env_cdf(env):
    return cdf_of(env._p_empty, env._p_tree)
