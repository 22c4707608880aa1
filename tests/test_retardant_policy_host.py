"""CPU: the Advanced env's observation with the retardant in it and the act entry point on it, in the host build
(include/gca.h gca_advanced_policy_observation, gca_advanced_policy_act_retardant), against the numpy restatement
tests/_retardant_obs_ref.py and the composition with tests/_bulldozer_policy_ref.py, bit for bit; the argument contract,
refused alike by the host and the device build before they touch memory; and BulldozerPolicy(retardant=True): the draw,
forward_torch and the learner's gradient on a host policy. No GPU."""
import ctypes

import numpy as np
import pytest

import _advanced_policy_ref as aref
import _bulldozer_policy_ref as bref
import _ppo_ref as R
import _retardant_obs_ref as rref

bits = rref.bits


def _inputs_exercise(shape, planes, dousing, pos, feat):
    """What this case's inputs exercise, as a set of names; each claim is checked on the expected output too."""
    E, H, W, B, r, _ = shape
    Hc, Wc, S = -(-H // B), -(-W // B), 2 * r + 1
    share = feat[:, 2 * Hc * Wc:3 * Hc * Wc].reshape(E, Hc, Wc)
    window = feat[:, 3 * Hc * Wc:3 * Hc * Wc + S * S].reshape(E, S, S)
    seen = set()
    inside = (pos[:, 0] >= 0) & (pos[:, 0] < H) & (pos[:, 1] >= 0) & (pos[:, 1] < W)
    for e in range(E):
        if tuple(pos[e]) == (0, 0):
            seen.add("corner")
        elif not inside[e]:
            seen.add("outside")
        elif tuple(pos[e]) == (H // 2, W // 2):
            seen.add("middle")
        if inside[e]:
            assert dousing[e, pos[e, 0], pos[e, 1]] != 0 and window[e, r, r] == 1.0
            seen.add("doused cell under the agent")
    if (dousing == 0).any() and (dousing == 1).any():
        seen.add("zeros and ones")
    if (dousing > 1).any():
        seen.add("a value above 1")
    assert share[0, 1, 1] == 1.0 and (dousing[0, B:2 * B, B:2 * B] != 0).all()
    seen.add("one block fully doused")
    if H % B or W % B:
        assert dousing[E - 1, H - 1, W - 1] != 0 and share[E - 1, -1, -1] > 0
        seen.add("doused cell in a partial edge block")
    seen.add("pad word" if (Hc * Wc) % 2 == 0 else "no pad word")
    assert ((window == 0).any() or r == 0) and set(np.unique(window)) <= {0.0, 1.0}  # r = 0: the agent's cell alone
    return seen


@pytest.mark.parametrize("shape, rot", rref.HOST_CASES)
def test_host_observation_equals_the_restatement(shape, rot):
    E, H, W, B, r, _ = shape
    d, w, planes, dousing, pos, ts = rref.make_case(shape, rot)
    want_lo, want_fe = rref.ref(planes, dousing, pos, r, B)
    lo, fe = rref.host_observe(planes, dousing, pos, r, B)
    assert np.array_equal(lo, want_lo) and np.array_equal(bits(fe), bits(want_fe))
    assert fe.shape == (E, d["C"]) and d["C"] % 2 == 0
    # the head of the vector is gca_policy_observation's coarse map, the window its window
    alo, aco = aref.observe_ref(planes, pos, r, B)
    assert np.array_equal(lo, alo) and np.array_equal(bits(fe[:, :d["Cg"]]), bits(aco.reshape(E, -1)))
    seen = _inputs_exercise(shape, planes, dousing, pos, fe)
    if d["C"] != 3 * d["Hc"] * d["Wc"] + d["SS"]:
        assert "pad word" in seen and (bits(fe[:, -1]) == 0).all()
    # either output may be NULL and changes nothing of the other; the bits are validated and not read
    lo1, none = rref.host_observe(planes, dousing, pos, r, B, feat=False)
    none2, fe1 = rref.host_observe(planes, dousing, pos, r, B, local=False)
    assert none is None and none2 is None and np.array_equal(lo1, lo) and np.array_equal(bits(fe1), bits(fe))
    if W % 16 == 0:
        junk = np.full((E, H, W // 16), 0xFFFF, np.uint16)
        lo2, fe2 = rref.host_observe(planes, dousing, pos, r, B, dous_bits=junk)
        assert np.array_equal(lo2, lo) and np.array_equal(bits(fe2), bits(fe))


def test_the_host_cases_exercise_every_input_the_contract_names():
    seen = set()
    for shape, rot in rref.HOST_CASES:
        _, _, planes, dousing, pos, _ = rref.make_case(shape, rot)
        _, fe = rref.ref(planes, dousing, pos, shape[4], shape[3])
        seen |= _inputs_exercise(shape, planes, dousing, pos, fe)
    assert seen == {"corner", "outside", "middle", "zeros and ones", "a value above 1", "one block fully doused",
                    "doused cell under the agent", "doused cell in a partial edge block", "pad word", "no pad word"}
    # the bits say what the layer says, cell by cell
    _, _, _, dousing, _, _ = rref.make_case(rref.HOST_CASES[0][0])
    b = rref.pack_bits(dousing)
    for e, r, c in ((0, 8, 8), (0, 0, 0), (2, 31, 255), (1, 5, 17), (1, 5, 16)):
        assert ((b[e, r, c // 16] >> (c % 16)) & 1) == (dousing[e, r, c] != 0)


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("shape, rot", rref.HOST_CASES)
def test_host_act_equals_the_composition_of_the_restatements(shape, rot, greedy):
    d, w, planes, dousing, pos, ts = rref.make_case(shape, rot)
    E = planes.shape[0]
    want_a, want_l, want_v, want_lo, want_fe, out32 = rref.composed(d, w, planes, dousing, pos, ts, env_offset=5,
                                                                    greedy=greedy)
    action, logits, value, local, feat = rref.host_act(d, w, planes, dousing, pos, ts, env_offset=5, greedy=greedy)
    assert np.array_equal(local, want_lo) and np.array_equal(bits(feat), bits(want_fe))
    assert np.array_equal(bits(logits), bits(want_l)) and np.array_equal(bits(value), bits(want_v))
    assert np.array_equal(bits(logits), bits(out32[:, :11])) and np.array_equal(bits(value), bits(out32[:, 11]))
    assert np.array_equal(action, want_a)
    assert ((0 <= action[:, 0]) & (action[:, 0] <= 8) & (0 <= action[:, 1]) & (action[:, 1] <= 1)).all()
    # the retardant reaches the outputs: the same state without it gives other logits
    dry, *_ = rref.host_act(d, w, planes, np.zeros_like(dousing), pos, ts, env_offset=5, greedy=greedy)[1:]
    assert not np.array_equal(bits(dry), bits(logits))
    if greedy:
        assert np.array_equal(action, bref.greedy_ref(logits))
    else:
        # the draw: Philox(((uint32)time_step, env_offset + e, 0, BPOL), seed), as gca_advanced_policy_act keys it
        u_m, u_s = bref.policy_u(rref.SEED, 5 + np.arange(E), ts.astype(np.int64), np.zeros(E))
        ref_action, near = bref.sample_ref(logits, u_m, u_s)
        assert np.array_equal(action[~near], ref_action[~near])


@pytest.mark.parametrize("shape, rot", rref.HOST_CASES)
def test_stride_three_keeps_the_third_column_and_null_outputs_change_nothing_else(shape, rot):
    d, w, planes, dousing, pos, ts = rref.make_case(shape, rot, seed=1)
    action, logits, value, local, feat = rref.host_act(d, w, planes, dousing, pos, ts)
    a3, l3, v3, lo3, fe3 = rref.host_act(d, w, planes, dousing, pos, ts, stride=3)
    assert (a3[:, 2] == rref.SENTINEL).all() and np.array_equal(a3[:, :2], action)
    assert np.array_equal(bits(l3), bits(logits)) and np.array_equal(bits(v3), bits(value))
    assert np.array_equal(lo3, local) and np.array_equal(bits(fe3), bits(feat))
    full = dict(logits=logits, value=value, local=local, feat=feat)
    for drop in full:
        got = dict(zip(("action", "logits", "value", "local", "feat"),
                       rref.host_act(d, w, planes, dousing, pos, ts, **{drop: False})))
        assert got.pop(drop) is None
        assert np.array_equal(got.pop("action"), action)
        for name, t in got.items():
            assert np.array_equal(t.view(np.uint8), full[name].view(np.uint8)), (drop, name)


# ------------------------------------------------------------------ the argument contract, in both builds
def A(i):
    """Fake address number i: 16-B aligned, 1 MiB from its neighbours."""
    return 0x5000000 + 0x100000 * i


_WEIGHTS = ("w_local", "w_coarse", "b1", "w_out", "b2")
_ACT_BASE = dict(grid=A(0), dousing=A(8), dous_bits=A(9), pos=A(1), time_step=A(2), E=2, H=32, W=256, empty=0, tree=1,
                 fire=2, env_offset=0, policy_seed=0, greedy=0, action=A(3), action_stride=2, logits=A(4), value=A(5),
                 local_out=A(6), feat_out=A(7), stream=None)
_OBS_BASE = dict(grid=A(0), dousing=A(8), dous_bits=A(9), pos=A(1), E=2, H=32, W=256, empty=0, tree=1, fire=2, radius=1,
                 block=8, local_out=A(6), feat_out=A(7), stream=None)
_C2_RANGE = "C2 = 3 Hc Wc + S*S rounded up to even, at most 15088"
# what both entry points ask of the state, in the order of the checks
_STATE = [("grid is null", dict(grid=None)), ("grid is null", dict(grid=None, dousing=None)),
          ("dousing is null", dict(dousing=None)), ("dousing is null", dict(dousing=None, pos=None)),
          ("pos is null", dict(pos=None)), ("pos is null", dict(pos=None, E=0)),
          ("E, H, W must be positive", dict(E=0)), ("E, H, W must be positive", dict(W=-1, dous_bits=A(9) + 1)),
          ("grid too large (H * W < 2^30)", dict(H=32768, W=32768)),
          ("the codes must be u8 values", dict(fire=256)), ("the codes must be u8 values", dict(empty=-1, W=40)),
          ("dous_bits needs W % 16 == 0", dict(W=40)), ("dous_bits needs W % 16 == 0", dict(W=250, dous_bits=A(9) + 1)),
          ("dous_bits must be 2-B aligned", dict(dous_bits=A(9) + 1))]
_ACT = [("policy is null", dict(policy=None))] + [(f"policy.{n} is null", {"p_" + n: None}) for n in _WEIGHTS] + [
    ("policy.radius in [0, 31]", dict(p_radius=32, grid=None)),
    ("policy.block must be a power of two in [1, 64]", dict(p_block=3)),
    ("policy.hidden must be a power of two in [32, 256]", dict(p_hidden=48, dousing=None)),
    ("time_step is null", dict(time_step=None, dousing=None)), ("action is null", dict(action=None, grid=None))] + \
    _STATE + [("action_stride >= 2", dict(action_stride=1)), ("action_stride >= 2", dict(action_stride=0, p_block=1)),
              (_C2_RANGE, dict(p_block=1)), (_C2_RANGE, dict(H=4096, W=4096, p_block=8)),
              # 2 Hc Wc = 15000 passes gca_advanced_policy_act's limit; 3 Hc Wc + 9 does not pass this one
              (_C2_RANGE, dict(H=400, W=1200, p_block=8, dous_bits=None))]
_OBS = _STATE + [("local_out or feat_out required", dict(local_out=None, feat_out=None)),
                 ("radius in [0, 31]", dict(radius=32)), ("radius in [0, 31]", dict(radius=-1, block=3)),
                 ("block must be a power of two in [1, 64]", dict(block=3)),
                 ("block must be a power of two in [1, 64]", dict(block=128)),
                 ("feat too large (C2 = 3 Hc Wc + S*S < 2^31)", dict(H=32767, W=32767, block=1, dous_bits=None))]
# refused by the device build alone (the kernel's 16-B loads of the weights), after every shared check
_DEVICE = [("policy.w_local and policy.w_coarse must be 16-B aligned", dict(p_w_local=A(20) + 8)),
           ("policy.w_local and policy.w_coarse must be 16-B aligned", dict(p_w_coarse=A(20) + 4)),
           (_C2_RANGE, dict(p_w_local=A(20) + 8, p_block=1))]


def _call(build, name, over):
    from gymca_amd import _lib

    p = _lib.BulldozerPolicyStruct()
    p.radius, p.block, p.hidden = 1, 8, 32
    for i, n in enumerate(_WEIGHTS):
        setattr(p, n, A(10 + i))
    act = name == "gca_advanced_policy_act_retardant"
    args = dict(_ACT_BASE, policy=ctypes.byref(p)) if act else dict(_OBS_BASE)
    for k, v in over.items():
        if k.startswith("p_"):
            setattr(p, k[2:], v)
        else:
            args[k] = v
    lib = {"host": _lib.load_cpu, "device": _lib.load}[build]()
    status = getattr(lib, name)(*[args[n] for n in (rref.ACT_ORDER if act else rref.OBS_ORDER)])
    return status, lib.gca_last_error().decode()


_CASES = {"gca_advanced_policy_act_retardant": ("advanced_policy_act_retardant", _ACT),
          "gca_advanced_policy_observation": ("advanced_policy_observation", _OBS)}


@pytest.mark.parametrize("name", sorted(_CASES))
@pytest.mark.parametrize("build", ["host", "device"])
def test_argument_errors_name_the_argument(build, name):
    from gymca_amd import _lib

    assert len(rref.ACT_ORDER) == len(_lib._SIGNATURES["gca_advanced_policy_act_retardant"][0])
    assert len(rref.OBS_ORDER) == len(_lib._SIGNATURES["gca_advanced_policy_observation"][0])
    who, cases = _CASES[name]
    texts = {text for text, _ in cases}
    assert {"dousing is null", "dous_bits needs W % 16 == 0"} <= texts
    assert (_C2_RANGE in texts) == name.endswith("act_retardant")
    for text, over in cases:
        status, msg = _call(build, name, over)
        assert status == 1 and msg == f"argument: {who}: {text}", (over, status, msg)


def test_both_builds_refuse_alike_and_the_device_checks_alignment():
    for name, (who, cases) in _CASES.items():
        for _, over in cases:
            host, device = _call("host", name, over), _call("device", name, over)
            assert host == device and host[0] == 1, (name, over, host, device)
    for text, over in _DEVICE:
        status, msg = _call("device", "gca_advanced_policy_act_retardant", over)
        assert status == 1 and msg == f"argument: advanced_policy_act_retardant: {text}", (over, status, msg)


def test_the_symbols_are_exported_by_both_builds():
    from gymca_amd import _lib

    for name in _CASES:
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib.CPU_BULLDOZER_POLICY_SYMBOLS
        assert name not in _lib.CPU_SYMBOLS
        assert hasattr(_lib.load_cpu(), name) and hasattr(_lib.load(), name)


# ------------------------------------------------------------------ BulldozerPolicy(retardant=True)
def test_without_the_keyword_nothing_changes_and_with_it_the_coarse_part_widens():
    import torch

    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy
    from gymca_amd.forest_fire.helicopter import HelicopterPolicy

    for r, B, Hd, H, W in ((5, 8, 64, 32, 256), (3, 4, 32, 24, 40), (0, 8, 32, 21, 33)):
        old = BulldozerPolicy((H, W), r, B, Hd, seed=4, device="cpu")
        off = BulldozerPolicy((H, W), r, B, Hd, seed=4, device="cpu", retardant=False)
        assert off.retardant is False and old.retardant is False and off.C == old.C == 2 * old.Hc * old.Wc
        assert off.weight_shapes() == old.weight_shapes()
        for x, y in zip(old.tensors(), off.tensors()):
            assert x.dtype is y.dtype and x.numpy().tobytes() == y.numpy().tobytes()
        on = BulldozerPolicy((H, W), r, B, Hd, seed=4, device="cpu", retardant=True)
        C2 = rref.c2(H, W, B, r)
        assert on.retardant is True and on.C == C2 and on.weight_shapes()["w_coarse"] == (C2, Hd)
        assert tuple(on.w_coarse.shape) == (C2, Hd) and on.weight_shapes()["w_local"] == old.weight_shapes()["w_local"]
        # the seeded draw's scale is that of n_in = S*S + C2 inputs
        n_in = on.S * on.S + C2
        assert abs(float(on.w_coarse.std()) / np.sqrt(2.0 / n_in) - 1) < 0.1  # 2 Hc Wc for C2 would be off by 1.2 x
        again = BulldozerPolicy((H, W), r, B, Hd, seed=4, device="cpu", retardant=True)
        assert all(torch.equal(x, y) for x, y in zip(on.tensors(), again.tensors()))
        # load keeps the widened shapes
        w = bref.make_weights(rref.dims(r, B, Hd, H, W), seed=1)
        assert torch.equal(on.load(w).w_coarse, torch.from_numpy(w["w_coarse"]))
        with pytest.raises(ValueError, match="w_coarse"):
            on.load(bref.make_weights(bref.dims(r, B, Hd, H, W), seed=1))
    with pytest.raises(TypeError):
        HelicopterPolicy((32, 256), device="cpu", retardant=True)


@pytest.mark.parametrize("shape, rot", rref.HOST_CASES)
def test_forward_torch_agrees_with_the_host_act_to_rounding(shape, rot):
    """The tolerance is test_bulldozer_policy_host.py's: forward_torch within the float64 evaluation's rounding bound, and
    within twice that bound of the host build's outputs."""
    import torch

    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    E, H, W, B, r, Hd = shape
    d, w, planes, dousing, pos, ts = rref.make_case(shape, rot, seed=2)
    local, feat = rref.ref(planes, dousing, pos, r, B)
    pol = BulldozerPolicy((H, W), r, B, Hd, device="cpu", retardant=True).load(w)
    move, shoot, value = pol.forward_torch(torch.from_numpy(local), torch.from_numpy(feat))
    assert tuple(move.shape) == (E, 9) and tuple(shoot.shape) == (E, 2) and tuple(value.shape) == (E,)
    out64, bound = bref.outputs_f64(w, d, local, feat)
    got = torch.cat([move, shoot, value[:, None]], 1).numpy().astype(np.float64)
    assert (np.abs(got - out64) <= bound).all()
    _, logits, val, _, _ = rref.host_act(d, w, planes, dousing, pos, ts)
    host = np.concatenate([logits, val[:, None]], 1).astype(np.float64)
    assert (np.abs(got - host) <= 2 * bound).all()
    m2, s2, v2 = pol.forward_torch(torch.from_numpy(local)[None], torch.from_numpy(feat)[None])
    assert tuple(m2.shape) == (1, E, 9) and torch.equal(m2[0], move) and torch.equal(v2[0], value)


def _records(doused, T=96, shape=(1, 24, 40, 4, 3, 32), seed=0):
    """T recorded samples of one small grid: random planes, a dousing layer with a share `doused` of doused cells,
    positions anywhere in the grid, the restated observation, random actions, old logits of perturbed head weights,
    advantages and returns."""
    _, H, W, B, r, Hd = shape
    d = rref.dims(r, B, Hd, H, W)
    w = bref.make_weights(d, seed=seed + 3, head=2.0)
    rng = np.random.default_rng(seed + 11)
    planes = rng.choice(np.array([0, 1, 2, 7], np.uint8), size=(T, H, W), p=[0.2, 0.4, 0.3, 0.1])
    dousing = (rng.random((T, H, W)) < doused).astype(np.uint8)
    pos = np.stack([rng.integers(0, H, T), rng.integers(0, W, T)], 1).astype(np.int32)
    local, feat = rref.ref(planes, dousing, pos, r, B)
    w_old = dict(w, w_out=(w["w_out"] + 0.3 * rng.standard_normal(w["w_out"].shape)).astype(np.float32))
    old, _ = bref.outputs_ref(w_old, d, local, feat)
    rec = {"local": local, "coarse": feat, "logits": np.ascontiguousarray(old[:, :11]),
           "action": np.stack([rng.integers(0, 9, T), rng.integers(0, 2, T)], 1).astype(np.int32)}
    adv = (rng.standard_normal(T) + 0.3).astype(np.float32)
    ret = rng.standard_normal(T).astype(np.float32)
    return d, w, rec, adv, ret


def _grad_through_forward_torch(pol, w, rec, adv, ret, idx, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5):
    """(grads, stats) of gca.h's per-head loss by torch's float32 autograd through pol.forward_torch on leaf copies of
    the weights: _ppo_ref.loss_and_grad's loss with forward_torch as the network."""
    import torch

    leaves = {k: torch.from_numpy(np.array(v, np.float32)).requires_grad_(True) for k, v in w.items()}
    sel = lambda a: torch.from_numpy(np.ascontiguousarray(a[idx]))
    move, shoot, value = pol.forward_torch(sel(rec["local"]), sel(rec["coarse"]), weights=leaves)
    act, old = sel(rec["action"]).long(), sel(rec["logits"])
    logratio, ent = [], []
    for h, (new, prev) in enumerate(((move, old[:, :9]), (shoot, old[:, 9:11]))):
        lp, lo = torch.log_softmax(new, 1), torch.log_softmax(prev, 1)
        logratio.append(lp.gather(1, act[:, h:h + 1])[:, 0] - lo.gather(1, act[:, h:h + 1])[:, 0])
        ent.append(-(torch.exp(lp) * lp).sum(1))
    logratio, ent = torch.stack(logratio, 1), torch.stack(ent, 1)
    ratio = torch.exp(logratio)
    A = sel(adv)
    mean, std = A.mean(), A.std(unbiased=False)
    A2 = ((A - mean) / (std + 1e-8))[:, None].repeat(1, 2)
    pg = torch.maximum(-A2 * ratio, -A2 * torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef)).mean()
    vl = (0.5 * (value - sel(ret)) ** 2).mean()
    loss = pg - ent_coef * ent.mean() + vf_coef * vl
    loss.backward()
    with torch.no_grad():
        kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio < 1 - clip_coef) | (ratio > 1 + clip_coef)).float().mean()
        stats = np.array([float(x) for x in (loss, pg, vl, ent.mean(), kl, clipfrac, mean, std)], np.float64)
    return {k: leaves[k].grad.numpy().astype(np.float64) for k in R.GRADS}, stats


@pytest.mark.parametrize("doused", [0.2, 0.0], ids=["retardant", "none"])
def test_ppo_grad_of_a_host_retardant_policy_matches_autograd_through_forward_torch(doused):
    """The tolerance is test_ppo_host.py's (_ppo_ref.assert_within): every error against the float64 autograd yardstick
    within 4 x the error of torch's own float32 autograd on the same rows, here taken through forward_torch."""
    import torch

    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    d, w, rec, adv, ret = _records(doused)
    T = len(adv)
    g64, s64, pre, ratio = R.loss_and_grad(w, d, rec, adv, ret, np.arange(T), R.BDZ.heads)
    idx = np.flatnonzero(R.decided(pre, R.pre_bound(w, d, rec), ratio, 0.2)).astype(np.int32)
    assert len(idx) >= 0.8 * T
    g64, s64, _, _ = R.loss_and_grad(w, d, rec, adv, ret, idx, R.BDZ.heads)
    pol = BulldozerPolicy((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device="cpu", retardant=True).load(w)
    assert pol.C == d["C"]
    gft, sft = _grad_through_forward_torch(pol, w, rec, adv, ret, idx)
    grads, stats = pol.ppo_grad({k: torch.from_numpy(v) for k, v in rec.items()}, torch.from_numpy(adv),
                                torch.from_numpy(ret), torch.from_numpy(idx))
    assert {k: tuple(v.shape) for k, v in grads.items()} == pol.weight_shapes()
    got = {k: v.numpy() for k, v in grads.items()}
    R.assert_within(R.errors(got, stats.numpy(), g64, s64), R.errors(gft, sft, g64, s64), f"retardant policy {doused}")
    tail = got["w_coarse"][d["Cg"]:]
    assert tail.shape[0] == d["C"] - d["Cg"] and np.abs(got["w_coarse"][:d["Cg"]]).max() > 0
    if doused:
        share, window = tail[:d["Hc"] * d["Wc"]], tail[d["Hc"] * d["Wc"]:d["Hc"] * d["Wc"] + d["SS"]]
        assert np.abs(share).max() > 0 and np.abs(window).max() > 0  # the learner reaches the retardant's weights
    else:
        assert (tail == 0).all() and (rec["coarse"][:, d["Cg"]:] == 0).all()
