"""Yardsticks of the PPO update (include/gca.h "PPO update"): the GAE recurrence restated in numpy float32, the loss
and its gradient by torch autograd of the network restated in float64 (and, for the tolerance, in float32), the sample
filter of the kinks, the shared cases and drivers of the host build. Test infrastructure only: the product never imports
it."""
import ctypes
import functools

import numpy as np

import _helicopter_policy_ref as pref

U = pref.U
FLOOR = 64 * U   # the tolerance's floor, for the cases where torch's float32 happens to be exact
# Tolerance: 4 x the error torch's own float32 autograd of the restated network shows against the float64 yardstick on
# the same case, at least FLOOR. Worst observed kernel error / max(torch-f32 error, FLOOR / 4) on an MI355X, per shape
# of SHAPES in order: 1.09, 1.68, 2.36, 1.41, 1.97, 2.37 (pg_loss or loss; the gradients stay below 1.3): DESIGN.md
# section 3.
MARGIN = 4.0
SHAPES = pref.SHAPES + [(5, 8, 128, 42, 42), (1, 4, 256, 5, 5)]
STATS = ("loss", "pg_loss", "v_loss", "entropy", "approx_kl", "clip_fraction", "adv_mean", "adv_std")
GRADS = ("w_local", "w_coarse", "b1", "w_out", "b2")


def gae_ref(reward, value, next_value, terminal, gamma, gae_lambda):
    """The recurrence of gca.h, every operation an individually rounded float32 one."""
    f = np.float32
    K, E = value.shape
    g, gl = f(gamma), f(float(gamma) * float(gae_lambda))
    adv, ret = np.zeros((K, E), f), np.zeros((K, E), f)
    A = np.zeros(E, f)
    nv = next_value.astype(f)
    for k in range(K - 1, -1, -1):
        r = reward[k].astype(f)
        nn = np.ones(E, f) if terminal is None else np.where(terminal[k] != 0, f(0), f(1)).astype(f)
        delta = (r + (g * nv) * nn) - value[k]
        A = delta + (gl * nn) * A
        adv[k] = A
        ret[k] = A + value[k]
        nv = value[k]
    return adv, ret


def host_gae(reward, value, next_value, terminal, gamma, gae_lambda, K=None):
    """gca_gae of the host build on numpy arrays, outputs prefilled with NaN."""
    from gymca_amd import _lib
    from gymca_amd.forest_fire import ppo

    Kv, E = value.shape
    adv, ret = np.full((Kv, E), np.nan, np.float32), np.full((Kv, E), np.nan, np.float32)
    p = lambda a: None if a is None else a.ctypes.data
    _lib.call_cpu("gca_gae", p(reward), p(value), p(next_value), p(terminal), float(gamma),
                  ppo.gamma_lambda(gamma, gae_lambda), Kv if K is None else K, E, p(adv), p(ret), None)
    return adv, ret


def gae_case(K, E, mode, seed=0):
    """(reward f64, value f32, next_value f32, terminal u8 | None). mode: None, "ones", "random" (row K-1 all set)."""
    rng = np.random.default_rng(seed + 131 * K + E)
    reward = rng.standard_normal((K, E)) * 0.7
    value = rng.standard_normal((K, E)).astype(np.float32)
    nxt = rng.standard_normal(E).astype(np.float32)
    if mode is None:
        term = None
    elif mode == "ones":
        term = np.ones((K, E), np.uint8)
    else:
        term = (rng.random((K, E)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (K, E)).astype(np.uint8)
        term[K - 1] = 1
    return reward, value, nxt, term


# ------------------------------------------------------------------ the loss and its gradient by autograd
def _network(w, onehot, coarse):
    import torch

    Hd = w["b1"].shape[0]
    a = onehot @ w["w_local"].reshape(-1, Hd) + coarse @ w["w_coarse"] + w["b1"]
    out = torch.relu(a) @ w["w_out"] + w["b2"]
    return a, out


def loss_and_grad(w, d, rec, adv, ret, idx, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, norm_adv=True, dtype="float64"):
    """The loss of gca.h on rows `idx` of the records by torch autograd on the CPU in `dtype`, the network restated as
    a one-hot matmul (the Dense layer over the one-hot classes that the lookup stands for). Returns (grads, stats, pre,
    ratio): numpy float64 arrays; pre (N, Hd) the hidden pre-activations, ratio (N,)."""
    import torch

    dt = getattr(torch, dtype)
    idx = np.asarray(idx, np.int64)
    N, SS = len(idx), d["SS"]
    leaves = {k: torch.tensor(np.asarray(v), dtype=dt, requires_grad=True) for k, v in w.items()}
    cls = rec["local"].reshape(-1, SS)[idx].astype(np.int64) & 3
    onehot = torch.zeros((N, SS * 4), dtype=dt)
    onehot[np.arange(N)[:, None], np.arange(SS)[None, :] * 4 + cls] = 1
    coarse = torch.tensor(rec["coarse"].reshape(-1, d["C"])[idx], dtype=dt)
    a, out = _network(leaves, onehot, coarse)
    logits, value = out[:, :9], out[:, 9]
    act = torch.tensor(rec["action"].reshape(-1)[idx].astype(np.int64))
    old = torch.tensor(rec["logits"].reshape(-1, 9)[idx], dtype=dt)
    logp = torch.log_softmax(logits, 1)
    logp_new = logp.gather(1, act[:, None])[:, 0]
    logp_old = torch.log_softmax(old, 1).gather(1, act[:, None])[:, 0]
    logratio = logp_new - logp_old
    ratio = torch.exp(logratio)
    A = torch.tensor(np.asarray(adv).reshape(-1)[idx], dtype=dt)
    mean, std = A.mean(), A.std(unbiased=False)
    if norm_adv:
        A = (A - mean) / (std + 1e-8)
    pg = torch.maximum(-A * ratio, -A * torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef)).mean()
    R = torch.tensor(np.asarray(ret).reshape(-1)[idx], dtype=dt)
    vl = (0.5 * (value - R) ** 2).mean()
    ent = (-(torch.exp(logp) * logp).sum(1)).mean()
    loss = pg - ent_coef * ent + vf_coef * vl
    loss.backward()
    with torch.no_grad():
        kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio < 1 - clip_coef) | (ratio > 1 + clip_coef)).to(dt).mean()
        stats = np.array([float(x) for x in (loss, pg, vl, ent, kl, clipfrac, mean, std)], np.float64)
    grads = {k: leaves[k].grad.numpy().astype(np.float64) for k in GRADS}
    return grads, stats, a.detach().numpy().astype(np.float64), ratio.detach().numpy().astype(np.float64)


def pre_bound(w, d, rec):
    """(T, Hd): the rounding bound (S^2 + C + 1) 2^-24 T_j of every row's pre-activations in ANY float32 summation
    order (the derivation in _helicopter_policy_ref.outputs_f64)."""
    SS, C = d["SS"], d["C"]
    cls = rec["local"].reshape(-1, SS).astype(np.int64) & 3
    wl = np.abs(w["w_local"].astype(np.float64))
    T = np.abs(w["b1"].astype(np.float64)) + wl[np.arange(SS)[None, :], cls].sum(1) + \
        np.abs(rec["coarse"].reshape(-1, C).astype(np.float64)) @ np.abs(w["w_coarse"].astype(np.float64))
    return (SS + C + 1) * U * T


def decided(pre, bound, ratio, clip_coef):
    """A sample is decided when no pre-activation lies within 4 x its bound of 0 and its ratio is at least 1e-3 away
    from 1 +- clip_coef: an f32 evaluation cannot legitimately take the other side of a kink."""
    relu_ok = (np.abs(pre) > 4 * bound).all(1)
    ratio_ok = (np.abs(ratio - (1 - clip_coef)) >= 1e-3) & (np.abs(ratio - (1 + clip_coef)) >= 1e-3)
    return relu_ok & ratio_ok


@functools.lru_cache(maxsize=None)
def case(shape, T=1200, seed=0, clip_coef=0.2):
    """The records of T rows for `shape`, shared (and left unchanged) by the tests: dims, weights (head = 2.0),
    uniformly random class windows with one byte of 7, a coarse map, actions, old logits from perturbed head weights
    scaled so that clipping is active on both sides, advantages of both signs, returns; `rows`: the decided rows."""
    d = pref.dims(*shape)
    rng = np.random.default_rng(seed + 7919 * shape[2] + shape[0])
    w = pref.make_weights(d, seed=seed + shape[2], head=2.0)
    local = rng.integers(0, 4, (T, d["S"], d["S"])).astype(np.uint8)
    local[3, 0, 0] = 7  # a class byte above 3 counts modulo 4
    coarse = (rng.integers(0, shape[1] ** 2 + 1, (T, 2, d["Hc"], d["Wc"])) / shape[1] ** 2).astype(np.float32)
    action = rng.integers(0, 9, T).astype(np.int32)
    adv = (rng.standard_normal(T) + 0.3).astype(np.float32)
    ret = rng.standard_normal(T).astype(np.float32)
    rec = {"local": local, "coarse": coarse, "action": action, "logits": np.zeros((T, 9), np.float32)}
    out64, _ = pref.outputs_f64(w, d, local, coarse)
    # the old policy: the head's weights perturbed, at the scale at which about 45 % of the ratios are clipped; a draw
    # that leaves less than 12 % on either side is drawn again
    SS, C = d["SS"], d["C"]
    cls = local.reshape(T, SS).astype(np.int64) & 3
    a64 = w["b1"].astype(np.float64) + w["w_local"].astype(np.float64)[np.arange(SS)[None, :], cls].sum(1) + \
        coarse.reshape(T, C).astype(np.float64) @ w["w_coarse"].astype(np.float64)

    def lp(l):
        z = l - l.max(1, keepdims=True)
        return (z - np.log(np.exp(z).sum(1, keepdims=True)))[np.arange(T), action]

    for _ in range(50):
        dw, db = rng.standard_normal(w["w_out"].shape) / np.sqrt(d["hidden"]), rng.standard_normal(10)
        delta = (np.maximum(a64, 0) @ dw + db)[:, :9]
        ratios = lambda scale: np.exp(lp(out64[:, :9]) - lp(out64[:, :9] - scale * delta))
        lo, hi = 0.0, 8.0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            r = ratios(mid)
            lo, hi = (mid, hi) if ((r < 1 - clip_coef) | (r > 1 + clip_coef)).mean() < 0.45 else (lo, mid)
        r = ratios(lo)
        if min((r < 1 - clip_coef).mean(), (r > 1 + clip_coef).mean()) >= 0.12:
            break
    rec["logits"] = (out64[:, :9] - lo * delta).astype(np.float32)
    _, _, pre, ratio = loss_and_grad(w, d, rec, adv, ret, np.arange(T), clip_coef)
    ok = decided(pre, pre_bound(w, d, rec), ratio, clip_coef)
    for a in (local, coarse, action, adv, ret, rec["logits"]):
        a.setflags(write=False)
    return dict(d=d, w=w, rec=rec, adv=adv, ret=ret, rows=np.flatnonzero(ok), ratio=ratio, T=T, clip_coef=clip_coef)


def minibatch(c, N, seed=0):
    """N decided rows with repeats, in a permuted order, row 3 (the class byte above 3) first. A seed that leaves row 3
    undecided is no case: pick another."""
    assert 3 in c["rows"] and c["rec"]["local"][3, 0, 0] == 7, "row 3 (the class byte 7) is undecided: another seed"
    rng = np.random.default_rng(seed + N)
    idx = rng.choice(c["rows"], N).astype(np.int32)
    idx[0] = 3
    return idx


def kernel_tile(lib, c):
    """The kernels' sample tile, read off the library itself (nothing restates the constant): the workspace holds whole
    tiles, so the tile is the largest N that needs no more than N = 1 does."""
    s, keep = pref.policy_struct(c["w"], c["d"])
    q = lambda N: lib.gca_helicopter_policy_grad_workspace(ctypes.byref(s), c["d"]["C"], N)
    N = 1
    while q(N + 1) == q(1):
        N += 1
        assert N < 4096
    return N


def errors(grads, stats, g64, s64):
    """{name: error}: per gradient tensor max|g - g64| / max|g64|, per statistic the relative error."""
    e = {k: float(np.abs(np.asarray(grads[k], np.float64) - g64[k]).max() / max(np.abs(g64[k]).max(), 1e-300))
         for k in GRADS}
    for i, k in enumerate(STATS):
        e[k] = float(abs(float(stats[i]) - s64[i]) / max(abs(s64[i]), 1e-300)) if s64[i] != 0 else abs(float(stats[i]))
    return e


def assert_within(got, torch32, where):
    """Every error of `got` within MARGIN x torch float32's on the same case, at least FLOOR; prints each figure."""
    bad = []
    for k, e in got.items():
        tol = max(MARGIN * torch32[k], FLOOR)
        print(f"{where} {k}: err {e:.3e} torch-f32 {torch32[k]:.3e} ratio {e / max(torch32[k], 1e-300):.2f}")
        if not e <= tol:
            bad.append((k, e, tol))
    assert not bad, (where, bad)


# ------------------------------------------------------------------ the host build
def host_grad(w, d, rec, adv, ret, idx, N=None, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, norm_adv=True, T=None,
              ws_bytes=None, alias=None, ws_offset=0):
    """gca_helicopter_policy_grad of the host build: (grads dict, stats), outputs prefilled with NaN."""
    from gymca_amd import _lib

    s, keep = pref.policy_struct(w, d)
    c = lambda a, t: np.ascontiguousarray(a, dtype=t)
    local, coarse = c(rec["local"], np.uint8), c(rec["coarse"], np.float32)
    action, logits = c(rec["action"], np.int32), c(rec["logits"], np.float32)
    adv, ret = c(adv, np.float32), c(ret, np.float32)
    Tn = action.size if T is None else T
    idx = None if idx is None else c(idx, np.int32)
    N = (Tn if idx is None else idx.size) if N is None else N
    grads = {k: np.full(np.asarray(w[k]).shape, np.nan, np.float32) for k in GRADS}
    if alias == "outputs":
        grads["b1"] = grads["w_coarse"].reshape(-1)[:d["hidden"]]
    if alias == "weights":
        grads["w_out"] = keep["w_out"]
    stats = np.full(8, np.nan, np.float32)
    need = _lib.load_cpu().gca_helicopter_policy_grad_workspace(ctypes.byref(s), d["C"], max(N, 1))
    ws = np.zeros(max(need if ws_bytes is None else ws_bytes, 16) + 16, np.uint8)[ws_offset:]
    p = lambda a: None if a is None else a.ctypes.data
    _lib.call_cpu("gca_helicopter_policy_grad", ctypes.byref(s), d["C"], p(local), p(coarse), p(action), p(logits),
                  p(adv), p(ret), Tn, p(idx), N, clip_coef, ent_coef, vf_coef, 1 if norm_adv else 0,
                  *[p(grads[k]) for k in GRADS], p(stats), p(ws), need if ws_bytes is None else ws_bytes, None)
    return grads, stats
