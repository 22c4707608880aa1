"""Yardstick of the learner's clipped value loss (include/gca.h gca_*_policy_grad_vclip), for both agents: the network
and the per-head terms of _ppo_ref.loss_and_grad with the reference's five lines (agents/jax_ppo.py:1021-1030, the batch
mean of the unclipped loss BEFORE the maximum) in place of 0.5 (v - R)^2, by torch autograd on the CPU in float64 (and
float32, for the tolerance); the recorded values of the shared cases, the filter of the two value kinks, the minibatches
and the driver of the host build. Test infrastructure only: the product never imports it."""
import ctypes
import functools

import numpy as np

import _policy_ref as P
import _ppo_ref as R

VSTATS = ("v_loss_unclipped", "u_share", "v_clip_fraction")
KINK = 1e-3        # a row's | |v - vo| - c | and a minibatch's min |q - U| / max(1, U) stay at least this far from 0
MIN_SHARE = 0.05   # for N >= 65: each side of each value kink holds at least this share of the minibatch
# the seed of a minibatch (agent name, shape, N): the first for which `minibatch`'s conditions hold; one that misses is
# replaced here, the conditions are not relaxed. Every entry not listed is 0.
SEEDS = {("helicopter", (2, 4, 32, 7, 9), 300): 2, ("bulldozer", (2, 8, 64, 40, 256), 300): 1,
         ("bulldozer", (31, 32, 256, 64, 256), 1200): 2, ("bulldozer", (0, 8, 32, 32, 256), 131): 1,
         ("bulldozer", (0, 8, 32, 32, 256), 1200): 2}


def loss_and_grad(w, d, rec, adv, ret, vo, idx, heads, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, norm_adv=True,
                  dtype="float64"):
    """_ppo_ref.loss_and_grad with the clipped value loss on the recorded values `vo` (T,). Returns (grads, stats,
    vstats, v, U, q): numpy float64; vstats = (U, the COUNT of samples whose maximum is U, the COUNT of samples outside
    the clip), v (N,) the value outputs, q (N,) the clipped squared errors."""
    import torch

    dt = getattr(torch, dtype)
    idx = np.asarray(idx, np.int64)
    N, SS, Hd, n_logits = len(idx), d["SS"], d["hidden"], sum(heads)
    leaves = {k: torch.tensor(np.asarray(v), dtype=dt, requires_grad=True) for k, v in w.items()}
    cls = rec["local"].reshape(-1, SS)[idx].astype(np.int64) & 3
    onehot = torch.zeros((N, SS * 4), dtype=dt)
    onehot[np.arange(N)[:, None], np.arange(SS)[None, :] * 4 + cls] = 1
    coarse = torch.tensor(rec["coarse"].reshape(-1, d["C"])[idx], dtype=dt)
    a = onehot @ leaves["w_local"].reshape(-1, Hd) + coarse @ leaves["w_coarse"] + leaves["b1"]
    out = torch.relu(a) @ leaves["w_out"] + leaves["b2"]
    newvalue = out[:, n_logits]
    act = torch.tensor(rec["action"].reshape(-1, len(heads))[idx].astype(np.int64))
    old = torch.tensor(rec["logits"].reshape(-1, n_logits)[idx], dtype=dt)
    logratio, ent, off = [], [], 0
    for h, n in enumerate(heads):
        logp, new = R._head_logp(out[:, off:off + n], act[:, h])
        _, prev = R._head_logp(old[:, off:off + n], act[:, h])
        logratio.append(new - prev)
        ent.append(-(torch.exp(logp) * logp).sum(1))
        off += n
    logratio, ent = torch.stack(logratio, 1), torch.stack(ent, 1)
    ratio = torch.exp(logratio)
    A = torch.tensor(np.asarray(adv).reshape(-1)[idx], dtype=dt)
    mean, std = A.mean(), A.std(unbiased=False)
    if norm_adv:
        A = (A - mean) / (std + 1e-8)
    A2 = A[:, None].repeat(1, len(heads))
    pg = torch.maximum(-A2 * ratio, -A2 * torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef)).mean()
    mb_returns = torch.tensor(np.asarray(ret).reshape(-1)[idx], dtype=dt)
    mb_values = torch.tensor(np.asarray(vo).reshape(-1)[idx], dtype=dt)
    # the reference's five lines
    v_loss_unclipped = 0.5 * ((newvalue - mb_returns) ** 2).mean()
    v_clipped = mb_values + torch.clamp(newvalue - mb_values, -clip_coef, clip_coef)
    v_loss_clipped = (v_clipped - mb_returns) ** 2
    v_loss_max = torch.maximum(v_loss_unclipped, v_loss_clipped)
    v_loss = 0.5 * v_loss_max.mean()
    en = ent.mean()
    loss = pg - ent_coef * en + vf_coef * v_loss
    loss.backward()
    with torch.no_grad():
        kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio < 1 - clip_coef) | (ratio > 1 + clip_coef)).to(dt).mean()
        stats = np.array([float(x) for x in (loss, pg, v_loss, en, kl, clipfrac, mean, std)], np.float64)
        n_u = int((v_loss_unclipped >= v_loss_clipped).sum())
        n_clip = int(((newvalue - mb_values).abs() > clip_coef).sum())
        vstats = (float(v_loss_unclipped), n_u, n_clip)
    grads = {k: leaves[k].grad.numpy().astype(np.float64) for k in R.GRADS}
    return (grads, stats, vstats, newvalue.detach().numpy().astype(np.float64), vstats[0],
            v_loss_clipped.detach().numpy().astype(np.float64))


@functools.lru_cache(maxsize=None)
def case(agent, shape):
    """_ppo_ref.case(agent, shape) unchanged, plus `vo` (T,) float32, the recorded values: the float64 value output with
    noise of 0.3 (the clip is 0.2: both sides of it are populated), and `vrows`, the rows decided by _ppo_ref AND at
    least KINK away from the clip's kink."""
    c = dict(R.case(agent, shape))
    d, w, T = c["d"], c["w"], c["T"]
    cls = c["rec"]["local"].reshape(T, d["SS"]).astype(np.int64) & 3
    a64 = w["b1"].astype(np.float64) + R._lookup(w["w_local"], cls) + \
        c["rec"]["coarse"].reshape(T, d["C"]).astype(np.float64) @ w["w_coarse"].astype(np.float64)
    v64 = (np.maximum(a64, 0) @ w["w_out"].astype(np.float64) + w["b2"].astype(np.float64))[:, agent.n_logits]
    rng = np.random.default_rng(4099 + 7919 * shape[2] + shape[0] + R.SALT[agent])
    vo = (v64 + 0.3 * rng.standard_normal(T)).astype(np.float32)
    ok = np.abs(np.abs(v64 - vo.astype(np.float64)) - c["clip_coef"]) >= KINK
    vo.setflags(write=False)
    c.update(vo=vo, v64=v64, vrows=np.intersect1d(c["rows"], np.flatnonzero(ok)))
    return c


def draw(c, N, seed):
    """(idx, U, q, outside) of the seed's draw, in numpy float64 from the case's v64: what `minibatch` tests."""
    rng = np.random.default_rng(seed + N)
    idx = rng.choice(c["vrows"], N).astype(np.int32)
    idx[0] = 3
    v, vo, ret = c["v64"][idx], c["vo"][idx].astype(np.float64), c["ret"][idx].astype(np.float64)
    U = 0.5 * ((v - ret) ** 2).mean()
    q = (vo + np.clip(v - vo, -c["clip_coef"], c["clip_coef"]) - ret) ** 2
    return idx, U, q, np.abs(v - vo) > c["clip_coef"]


def is_decided(N, U, q, outside):
    if np.abs(q - U).min() < KINK * max(1.0, U):
        return False
    shares = ((U >= q).mean(), (U < q).mean(), outside.mean(), 1 - outside.mean())
    return N < 65 or min(shares) >= MIN_SHARE


def minibatch(c, N, norm_adv=True):
    """(idx, f64, f32): N decided rows with repeats (row 3, the class byte above 3, first) and the yardstick's two
    results on them. The minibatch is decided: min_s |q_s - U| >= KINK max(1, U) in float64, and for N >= 65 each side
    of each value kink holds MIN_SHARE of it. A seed that misses is replaced in SEEDS."""
    agent = c["agent"]
    key = (agent.name, tuple(c["d"][k] for k in ("radius", "block", "hidden", "H", "W")), N)
    assert 3 in c["vrows"], "row 3 (the class byte 7) is undecided: another seed"
    idx, U0, q0, outside = draw(c, N, SEEDS.get(key, 0))
    assert is_decided(N, U0, q0, outside), (key, "undecided minibatch or a nearly empty branch: another seed in SEEDS")
    args = (c["w"], c["d"], c["rec"], c["adv"], c["ret"], c["vo"], idx, agent.heads)
    f64 = loss_and_grad(*args, clip_coef=c["clip_coef"], norm_adv=norm_adv)
    f32 = loss_and_grad(*args, clip_coef=c["clip_coef"], norm_adv=norm_adv, dtype="float32")
    (U, n_u, n_clip), q = f64[2], f64[5]
    gap = np.abs(q - U).min()
    assert gap >= KINK * max(1.0, U), (key, "undecided minibatch: another seed in SEEDS", gap, U)
    if N >= 65:
        shares = (n_u / N, 1 - n_u / N, n_clip / N, 1 - n_clip / N)
        assert min(shares) >= MIN_SHARE, (key, "a branch is nearly empty: another seed in SEEDS", shares)
    assert f32[2][1:] == f64[2][1:], (key, "float32 takes another branch than float64", f32[2], f64[2])
    return idx, f64, f32


def errors(grads, stats, vstats, f):
    """_ppo_ref.errors against the yardstick result `f`, plus the relative error of U under VSTATS[0]."""
    e = R.errors(grads, stats, f[0], f[1])
    e[VSTATS[0]] = abs(float(vstats[0]) - f[2][0]) / max(abs(f[2][0]), 1e-300)
    return e


def yard_errors(f32, f64):
    return errors(f32[0], f32[1], (f32[2][0],), f64)


def assert_shares(vstats, f64, N, where):
    """The two shares are exactly the yardstick's counts / N (the double quotient rounded to float32)."""
    want = (np.float32(f64[2][1] / N), np.float32(f64[2][2] / N))
    got = (np.float32(vstats[1]), np.float32(vstats[2]))
    print(f"{where} shares: got {got} want {want}")
    assert got == want, (where, got, want)


# ------------------------------------------------------------------ the host build
def host_grad(agent, w, d, rec, adv, ret, vo, idx, N=None, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, norm_adv=True,
              T=None, ws_bytes=None, alias=None, null=None, vstats=True):
    """The agent's <entry>_grad_vclip of the host build: (grads dict, stats, vstats), outputs prefilled with NaN. null:
    the name of a record passed as a null pointer ("value": the recorded values); alias: "vstats", vstats inside
    another output; vstats=False passes a null vstats."""
    from gymca_amd import _lib

    s, keep = P.policy_struct(w, d)
    c = lambda a, t: np.ascontiguousarray(a, dtype=t)
    records = {"local": c(rec["local"], np.uint8), "coarse": c(rec["coarse"], np.float32),
               "action": c(rec["action"], np.int32), "logits": c(rec["logits"], np.float32),
               "value": c(vo, np.float32), "advantage": c(adv, np.float32), "returns": c(ret, np.float32)}
    Tn = records["action"].size // len(agent.heads) if T is None else T
    idx = None if idx is None else c(idx, np.int32)
    N = (Tn if idx is None else idx.size) if N is None else N
    grads = {k: np.full(np.asarray(w[k]).shape, np.nan, np.float32) for k in R.GRADS}
    stats = np.full(8, np.nan, np.float32)
    vs = np.full(3, np.nan, np.float32)
    if alias == "vstats":
        vs = grads["w_coarse"].reshape(-1)[1:4]
    need = getattr(_lib.load_cpu(), agent.entry + "_grad_workspace")(ctypes.byref(s), d["C"], max(N, 1))
    ws = np.zeros(max(need if ws_bytes is None else ws_bytes, 16) + 16, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data
    if null is not None:
        records[null] = None
    _lib.call_cpu(agent.entry + "_grad_vclip", ctypes.byref(s), d["C"], *[p(records[k]) for k in records], Tn, p(idx), N,
                  clip_coef, ent_coef, vf_coef, 1 if norm_adv else 0, *[p(grads[k]) for k in R.GRADS], p(stats),
                  p(vs) if vstats else None, p(ws), need if ws_bytes is None else ws_bytes, None)
    return grads, stats, vs
