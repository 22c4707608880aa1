"""The bulldozer policy network (include/gca.h "bulldozer policy") restated in numpy float32, in the header's summation
order -- the definition the device kernels and the host build are held against, bit for bit -- with both heads'
sampling rule in float64, the Philox key, a driver of the host build and the shapes the CPU and GPU tests share. It
builds on _helicopter_policy_ref (the hidden layer and the float64 bound do not depend on the number of outputs). Test
infrastructure only: the product never imports it."""
import ctypes

import numpy as np

from oracle import philox

import _helicopter_policy_ref as href

TAG_BPOLICY = 0x42504F4C
N_OUT = 12
# (radius, block, hidden, H, W): a zero radius at one wave's height, H no multiple of 32, both widths, the largest window
SHAPES = [(0, 8, 32, 32, 256), (2, 8, 64, 40, 256), (5, 16, 128, 64, 512), (31, 32, 256, 64, 256)]

dims = href.dims
outputs_f64 = href.outputs_f64  # (out (E, 12) float64, bound (E, 12)): written for any number of outputs


def make_weights(d, seed=0, scale=1.0, head=1.0):
    """Five float32 arrays with both signs everywhere (b1 shifted down a little, so relu clips a good share)."""
    rng = np.random.default_rng(seed)
    n_in = d["SS"] + d["C"]
    f = lambda shape, s: (rng.standard_normal(shape) * s).astype(np.float32)
    return {"w_local": f((d["SS"], 4, d["hidden"]), scale * np.sqrt(2.0 / n_in)),
            "w_coarse": f((d["C"], d["hidden"]), scale * np.sqrt(2.0 / n_in)),
            "b1": f((d["hidden"],), 0.3 * scale) - np.float32(0.1 * scale),
            "w_out": f((d["hidden"], N_OUT), head / np.sqrt(d["hidden"])),
            "b2": f((N_OUT,), 0.5 * head)}


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
    wh = href.make_weights(d, seed=Hd, head=2.0)
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


def outputs_ref(w, d, local, coarse):
    """(E, 12) float32: nine move logits, two shoot logits, the value; every multiply and add rounded on its own, in the
    header's order. Also returns the pre-activations."""
    a = href.hidden_ref(w, d, local, coarse)
    h = np.where(a > 0, a, np.float32(0)).astype(np.float32)
    E, Hd = h.shape
    q = np.zeros((16, E, N_OUT), np.float32)
    for j in range(Hd):
        q[j % 16] = q[j % 16] + w["w_out"][j][None, :] * h[:, j][:, None]
    for half in (8, 4, 2, 1):
        q[:half] = q[:half] + q[half:2 * half]
    return (w["b2"][None, :] + q[0]).astype(np.float32), a


def policy_u(seed, env_ids, steps_elapsed, episode):
    """(u_move, u_shoot): u01_f32 of words 0 and 1 of Philox(((uint32)steps_elapsed, env id, episode, BPOL), seed)."""
    n = len(env_ids)
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0] = np.asarray(steps_elapsed).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 1] = np.asarray(env_ids).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 2] = np.asarray(episode).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    ctr[:, 3] = TAG_BPOLICY
    x = philox.philox4x32_10(ctr, philox.seed_key(seed))
    u = lambda col: ((x[:, col].astype(np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    return u(0), u(1)


def sample_ref(logits, u_move, u_shoot, rel=1e-5):
    """(action (n, 2), near (n,)): both heads' rule with the CDF in float64. near: a head's u * c_last lies within
    relative `rel` of one of its boundaries, where the float32 CDF may fall on the other side."""
    l = np.asarray(logits, np.float64).reshape(-1, 11)
    move, near_m = href.sample_ref(l[:, :9], u_move, rel)
    s = l[:, 9:11]
    p = np.exp(s - s.max(1, keepdims=True))
    c0, c1 = p[:, 0], p[:, 0] + p[:, 1]
    t = np.asarray(u_shoot, np.float64) * c1
    shoot = np.where(t < c0, 0, 1).astype(np.int32)
    near = near_m | (np.abs(t - c0) <= rel * c0)
    return np.stack([move, shoot], 1), near


def greedy_ref(logits):
    l = np.asarray(logits).reshape(-1, 11)
    return np.stack([np.argmax(l[:, :9], 1), np.argmax(l[:, 9:11], 1)], 1).astype(np.int32)  # the first maxima


# ------------------------------------------------------------------ the host build
def policy_struct(w, d):
    """(struct, keep): _lib.BulldozerPolicyStruct with the host arrays' addresses; `keep` holds the contiguous arrays."""
    from gymca_amd import _lib

    keep = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}
    s = _lib.BulldozerPolicyStruct()
    s.radius, s.block, s.hidden, s.reserved = d["radius"], d["block"], d["hidden"], 0
    for k, v in keep.items():
        setattr(s, k, v.ctypes.data)
    return s, keep


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
