"""The helicopter policy network (include/gca.h "helicopter policy") restated in numpy float32, in the header's
summation order -- the definition the device kernels and the host build are held against, bit for bit -- plus a float64
evaluation with its rounding bound, the sampling rule in float64, drivers of the host build and the cases the CPU and
GPU tests share. Test infrastructure only: the product never imports it."""
import ctypes

import numpy as np

from oracle import philox

import _helicopter_ref as href
import _policy_obs_ref as obs

TAG_POLICY = 0x504F4C49
U = 2.0 ** -24  # the unit roundoff of float32
# (radius, block, hidden, H, W): odd sizes, the flagship 42 x 42, one cell with a zero radius, a block larger than the grid
SHAPES = [(2, 4, 32, 7, 9), (3, 8, 64, 42, 42), (0, 1, 32, 1, 1), (1, 64, 32, 5, 5)]


def dims(r, B, Hd, H, W):
    S, Hc, Wc = 2 * r + 1, -(-H // B), -(-W // B)
    return dict(radius=r, block=B, hidden=Hd, H=H, W=W, S=S, SS=S * S, Hc=Hc, Wc=Wc, C=2 * Hc * Wc)


def make_weights(d, seed=0, scale=1.0, head=1.0):
    """Five float32 arrays with both signs everywhere (b1 shifted down a little, so relu clips a good share)."""
    rng = np.random.default_rng(seed)
    n_in = d["SS"] + d["C"]
    f = lambda shape, s: (rng.standard_normal(shape) * s).astype(np.float32)
    return {"w_local": f((d["SS"], 4, d["hidden"]), scale * np.sqrt(2.0 / n_in)),
            "w_coarse": f((d["C"], d["hidden"]), scale * np.sqrt(2.0 / n_in)),
            "b1": f((d["hidden"],), 0.3 * scale) - np.float32(0.1 * scale),
            "w_out": f((d["hidden"], 10), head / np.sqrt(d["hidden"])),
            "b2": f((10,), 0.5 * head)}


def hidden_ref(w, d, local, coarse):
    """(E, Hd) float32 pre-activations b1 + p_0 + ... + p_{G-1} in the header's order."""
    E, Hd, SS, C = local.shape[0], d["hidden"], d["SS"], d["C"]
    G = 1024 // Hd
    loc = local.reshape(E, SS).astype(np.int64) & 3
    co = coarse.reshape(E, C).astype(np.float32)
    p = np.zeros((G, E, Hd), np.float32)
    for n in range(SS + C):
        if n < SS:
            t = w["w_local"][n][loc[:, n]]                     # a lookup, no multiply
        else:
            t = w["w_coarse"][n - SS][None, :] * co[:, n - SS][:, None]  # one rounded product
        p[n % G] = p[n % G] + t
    a = np.broadcast_to(w["b1"], (E, Hd)).astype(np.float32)
    for g in range(G):
        a = a + p[g]
    return a


def outputs_ref(w, d, local, coarse):
    """(E, 10) float32: the nine logits and the value, every multiply and add rounded on its own, in the header's
    order. Also returns the pre-activations (the relu-clipping assertions)."""
    a = hidden_ref(w, d, local, coarse)
    h = np.where(a > 0, a, np.float32(0)).astype(np.float32)
    E, Hd = h.shape
    q = np.zeros((16, E, 10), np.float32)
    for j in range(Hd):
        q[j % 16] = q[j % 16] + w["w_out"][j][None, :] * h[:, j][:, None]
    for half in (8, 4, 2, 1):
        q[:half] = q[:half] + q[half:2 * half]
    return (w["b2"][None, :] + q[0]).astype(np.float32), a


def outputs_f64(w, d, local, coarse):
    """(out (E, 10) float64, bound (E, 10)): the network in float64 and the rounding bound of ANY float32 summation
    order, (n + 2) * 2^-24 * sum|terms| per output.

    Derivation. A float32 sum of k addends, each at most one rounded product, in any order, differs from the exact sum
    by at most k u sum|addends| to first order (u = 2^-24). The hidden pre-activation a_j has N + 1 addends (b1 and
    the N = S*S + C input terms), so |a^_j - a_j| <= (N + 1) u T_j with T_j = |b1_j| + sum_n |t_n[j]|; relu is
    1-Lipschitz, so the same holds for h_j, and h_j <= T_j. An output has Hd + 1 addends b2_o, w_jo h^_j: its own
    rounding is at most (Hd + 1) u (|b2_o| + sum_j |w_jo| h^_j) and the hidden errors arrive scaled by |w_jo|. With
    sum|terms|_o = |b2_o| + sum_j |w_jo| T_j and n = (N + 1) + (Hd + 1) addends along the deepest path the total is at
    most n u sum|terms|_o to first order; the second-order remainder is below (n u)^2 sum|terms|, which the + 2 covers
    while n^2 u <= 2, i.e. n <= 5792 (here n <= 4300 even at radius 31; the test shapes have n <= 250)."""
    E, Hd, SS, C = local.shape[0], d["hidden"], d["SS"], d["C"]
    loc = local.reshape(E, SS).astype(np.int64) & 3
    co = coarse.reshape(E, C).astype(np.float64)
    wl, wc = w["w_local"].astype(np.float64), w["w_coarse"].astype(np.float64)
    tl = wl[np.arange(SS)[None, :], loc]                       # (E, SS, Hd)
    tc = co[:, :, None] * wc[None]                             # (E, C, Hd)
    a = w["b1"].astype(np.float64) + tl.sum(1) + tc.sum(1)
    T = np.abs(w["b1"].astype(np.float64)) + np.abs(tl).sum(1) + np.abs(tc).sum(1)
    wo = w["w_out"].astype(np.float64)
    out = w["b2"].astype(np.float64) + np.maximum(a, 0.0) @ wo
    terms = np.abs(w["b2"].astype(np.float64)) + T @ np.abs(wo)
    n = (SS + C + 1) + (Hd + 1)
    assert n * n * U <= 2.0
    return out, (n + 2) * U * terms


def policy_u(seed, env_ids, rng_steps):
    """u01_f32(x.x) of Philox((0, env id, rng_step, POLI), seed): float32 in [0, 1)."""
    n = len(env_ids)
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 1] = np.asarray(env_ids, np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 2] = np.asarray(rng_steps, np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 3] = TAG_POLICY
    x = philox.philox4x32_10(ctr, philox.seed_key(seed))
    return ((x[:, 0].astype(np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def sample_ref(logits, u, rel=1e-5):
    """(action, near): the sampling rule with the CDF in float64 (np.exp). near[i]: u * c_8 lies within relative `rel`
    of one of the boundaries c_0..c_7, where the float32 CDF of the product may fall on the other side."""
    l = np.asarray(logits, np.float64).reshape(-1, 9)
    p = np.exp(l - l.max(1, keepdims=True))
    c = np.cumsum(p, 1)
    t = np.asarray(u, np.float64) * c[:, 8]
    below = t[:, None] < c[:, :8]
    action = np.where(below.any(1), below.argmax(1), 8).astype(np.int32)
    near = (np.abs(t[:, None] - c[:, :8]) <= rel * c[:, :8]).any(1)
    return action, near


def greedy_ref(logits):
    return np.argmax(np.asarray(logits).reshape(-1, 9), 1).astype(np.int32)  # the first maximum


# ------------------------------------------------------------------ the host build
def policy_struct(w, d):
    """(struct, keep): _lib.HeliPolicy with the host arrays' addresses; `keep` holds the contiguous arrays."""
    from gymca_amd import _lib

    keep = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}
    s = _lib.HeliPolicy()
    s.radius, s.block, s.hidden, s.reserved = d["radius"], d["block"], d["hidden"], 0
    for k, v in keep.items():
        setattr(s, k, v.ctypes.data)
    return s, keep


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
