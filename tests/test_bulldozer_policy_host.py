"""CPU: the bulldozer policy network of the host build (gca_bulldozer_policy_act) against the numpy float32 restatement
in the header's summation order (tests/_bulldozer_policy_ref.py), bit for bit; against a float64 evaluation within the
derivable rounding bound; both heads' sampling rule; BulldozerPolicy (forward_torch, load, assignment); and the argument
contract of gca_bulldozer_policy_act, refused alike by the host and the device build before they touch memory. No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _bulldozer_policy_ref as bref
import _policy_obs_ref as obs
from conftest import ROOT

SEED = 0x1234ABCD5678


def _case(shape, E=4, seed=0):
    """dims, weights and an observation of E envs whose windows hang over every grid edge (positions (0, 0),
    (H - 1, W - 1) and the centre), with per-env step and episode counters that are non-zero and all different."""
    r, B, Hd, H, W = shape
    d = bref.dims(*shape)
    w = bref.make_weights(d, seed=seed + Hd)
    buf, parity, _ = obs.make_case(E, H, W, B, seed=seed)
    pos = obs.positions(E, H, W, rot=seed)
    local, coarse = obs.host_observe(buf, parity, pos, obs.CODES, r, B)
    if r > 0:
        assert (local == 3).any() and (local != 3).any()
        tl = int(np.flatnonzero((pos == 0).all(1))[0])
        br = int(np.flatnonzero((pos == (H - 1, W - 1)).all(1))[0])
        assert (local[tl, 0] == 3).all() and (local[tl, :, 0] == 3).all()      # the top and the left edge
        assert (local[br, -1] == 3).all() and (local[br, :, -1] == 3).all()    # the bottom and the right edge
    se = np.array([3, 17, 2**32 + 5, 250], np.int64)[:E]   # the key takes the low 32 bits
    ep = np.array([1, 2, 7, 0xFFFFFFFF], np.uint32)[:E]
    return d, w, local, coarse, se, ep


@pytest.mark.parametrize("shape", bref.SHAPES)
def test_outputs_and_actions_equal_the_float32_restatement(shape):
    d, w, local, coarse, se, ep = _case(shape)
    E = local.shape[0]
    want, pre = bref.outputs_ref(w, d, local, coarse)
    assert (pre < 0).any() and (pre > 0).any()  # relu clips some units and passes others
    action, logits, value = bref.host_act(w, d, local, coarse, se, ep, env_offset=5, seed=SEED)
    assert np.array_equal(logits.view(np.uint32), np.ascontiguousarray(want[:, :11]).view(np.uint32))
    assert np.array_equal(value.view(np.uint32), np.ascontiguousarray(want[:, 11]).view(np.uint32))
    u_m, u_s = bref.policy_u(SEED, 5 + np.arange(E), se, ep)
    ref_action, near = bref.sample_ref(logits, u_m, u_s)
    assert np.array_equal(action[~near], ref_action[~near])
    assert ((0 <= action[:, 0]) & (action[:, 0] <= 8) & (0 <= action[:, 1]) & (action[:, 1] <= 1)).all()
    greedy, _, _ = bref.host_act(w, d, local, coarse, se, ep, env_offset=5, seed=SEED, greedy=True)
    assert np.array_equal(greedy, bref.greedy_ref(logits))
    # the nullable outputs (logits, value, episode), and no env state to change: the counters are read only
    a2, l2, v2 = bref.host_act(w, d, local, coarse, se, ep, env_offset=5, seed=SEED, want_logits=False,
                               want_value=False)
    assert l2 is None and v2 is None and np.array_equal(a2, action)
    a3, _, _ = bref.host_act(w, d, local, coarse, se, None, env_offset=5, seed=SEED)
    a4, _, _ = bref.host_act(w, d, local, coarse, se, np.zeros(E, np.uint32), env_offset=5, seed=SEED)
    assert np.array_equal(a3, a4)  # episode == NULL keys the draw with 0
    assert se[2] == 2**32 + 5 and ep[3] == 0xFFFFFFFF


@pytest.mark.parametrize("shape", bref.SHAPES)
def test_outputs_within_the_rounding_bound_of_float64(shape):
    d, w, local, coarse, se, ep = _case(shape, seed=1)
    out64, bound = bref.outputs_f64(w, d, local, coarse)
    assert out64.shape == (local.shape[0], 12)
    _, logits, value = bref.host_act(w, d, local, coarse, se, ep)
    got = np.concatenate([logits, value[:, None]], 1).astype(np.float64)
    gap = np.abs(got - out64)
    print("max gap / bound:", (gap / bound).max())
    assert (gap <= bound).all()
    ref32, _ = bref.outputs_ref(w, d, local, coarse)
    assert (np.abs(ref32.astype(np.float64) - out64) <= bound).all()


def _inject(logits11):
    """A network whose outputs are exactly `logits11` (and value 0) whatever it observes: zero w_out, b2 = the logits."""
    d = bref.dims(0, 1, 32, 1, 1)
    w = {k: np.zeros_like(v) for k, v in bref.make_weights(d).items()}
    w["b2"][:11] = logits11
    return d, w


def _zeros_obs(n):
    return np.zeros((n, 1, 1), np.uint8), np.zeros((n, 2, 1, 1), np.float32)


def test_sampling_frequencies_match_the_softmax_of_both_heads():
    """4096 (env, step) keys with fixed logits: 64 envs x 64 values of steps_elapsed. Both heads' empirical frequencies
    within 5 standard deviations of their softmax."""
    l11 = np.array([0.3, -1.2, 2.0, 0.0, 0.5, -0.4, 1.1, -2.5, 0.9, 0.7, -0.6], np.float32)
    d, w = _inject(l11)
    n_env, n_step = 64, 64
    moves, shoots = [], []
    local, coarse = _zeros_obs(n_env)
    for step in range(n_step):
        action, logits, _ = bref.host_act(w, d, local, coarse, np.full(n_env, step, np.int64),
                                          np.full(n_env, 3, np.uint32), env_offset=100, seed=99)
        assert np.array_equal(logits, np.broadcast_to(l11, (n_env, 11)))
        moves.append(action[:, 0])
        shoots.append(action[:, 1])
    n = n_env * n_step
    assert n == 4096
    for got, l in ((np.concatenate(moves), l11[:9]), (np.concatenate(shoots), l11[9:])):
        p = np.exp(l.astype(np.float64) - l.max())
        p /= p.sum()
        freq = np.bincount(got, minlength=len(l)) / n
        sigma = np.sqrt(p * (1 - p) / n)
        print("freq", freq, "softmax", p, "in sigmas", np.abs(freq - p) / sigma)
        assert (np.abs(freq - p) <= 5 * sigma).all(), (freq, p)
    # consecutive steps draw different uniforms (the key is steps_elapsed, not rng_step), and the two heads use
    # different words of the block
    assert len({tuple(m) for m in moves}) > n_step // 2
    u_m, u_s = bref.policy_u(99, 100 + np.arange(n_env), np.zeros(n_env), np.full(n_env, 3))
    assert not np.array_equal(u_m, u_s)


def test_sampling_follows_the_float64_cdf_and_its_key():
    rng = np.random.default_rng(7)
    E, total, left_out = 256, 0, 0
    for i in range(40):
        l11 = (rng.standard_normal(11) * rng.choice([0.01, 1.0, 4.0])).astype(np.float32)
        d, w = _inject(l11)
        se = rng.integers(0, 2**33, E, dtype=np.int64)
        ep = rng.integers(0, 2**32, E, dtype=np.uint64).astype(np.uint32)
        local, coarse = _zeros_obs(E)
        action, logits, _ = bref.host_act(w, d, local, coarse, se, ep, env_offset=11, seed=SEED + i)
        u_m, u_s = bref.policy_u(SEED + i, 11 + np.arange(E), se, ep)
        want, near = bref.sample_ref(logits, u_m, u_s)
        total, left_out = total + E, left_out + int(near.sum())
        assert np.array_equal(action[~near], want[~near]), f"vector {i}"
    assert total == 10240 and left_out <= 0.01 * total, (left_out, total)


def test_greedy_takes_the_first_maximum_of_each_head_and_ignores_the_seed():
    for l11 in ([0, 1, 5, 5, 2, 5, 0, 0, 0, 1, 1], [3] * 11, [-1, -1, -1, -1, -1, -1, -1, -1, -0.5, 0, 2],
                [2, 1, 0, 0, 0, 0, 0, 0, 2, 4, -4]):
        l11 = np.array(l11, np.float32)
        d, w = _inject(l11)
        E = 6
        local, coarse = _zeros_obs(E)
        for seed in (0, 1):
            action, _, _ = bref.host_act(w, d, local, coarse, np.arange(E), np.arange(E), seed=seed, greedy=True)
            assert (action == bref.greedy_ref(l11)[0]).all(), l11


def test_non_finite_weights_keep_both_actions_in_range():
    d = bref.dims(1, 4, 32, 5, 5)
    w = bref.make_weights(d)
    local, coarse = np.zeros((8, 3, 3), np.uint8), np.ones((8, d["C"]), np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        for where in ((2, 9), (3, 10), (0, 11)):
            w2 = {k: v.copy() for k, v in w.items()}
            for o in where[:2]:
                w2["b2"][o] = bad
            w2["w_coarse"][0, 3] = bad
            for greedy in (False, True):
                action, _, _ = bref.host_act(w2, d, local, coarse, np.arange(8), greedy=greedy)
                assert ((0 <= action[:, 0]) & (action[:, 0] <= 8)).all()
                assert ((0 <= action[:, 1]) & (action[:, 1] <= 1)).all()
    w2 = {k: np.full_like(v, np.nan) for k, v in w.items()}
    action, _, _ = bref.host_act(w2, d, local, coarse, np.arange(8))
    assert ((0 <= action[:, 0]) & (action[:, 0] <= 8) & (0 <= action[:, 1]) & (action[:, 1] <= 1)).all()


@pytest.mark.parametrize("shape", bref.SHAPES)
def test_forward_torch_within_the_rounding_bound(shape):
    import torch

    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    r, B, Hd, H, W = shape
    d, w, local, coarse, se, ep = _case(shape, seed=2)
    pol = BulldozerPolicy((H, W), r, B, Hd, device="cpu")
    assert pol.weight_shapes() == {k: v.shape for k, v in w.items()} and pol.C == d["C"]
    assert pol.weight_shapes()["w_out"] == (Hd, 12) and pol.weight_shapes()["b2"] == (12,)
    assert all(t.abs().max() > 0 for t in (pol.w_local, pol.w_coarse, pol.w_out))  # a seeded, non-trivial draw
    # 0.01 on both policy heads, a unit value head
    assert pol.w_out[:, :11].std() < 0.1 * pol.w_out[:, 11].std()
    same = BulldozerPolicy((H, W), r, B, Hd, device="cpu")
    assert all(torch.equal(x, y) for x, y in zip(pol.tensors(), same.tensors()))
    pol.load(w)
    move, shoot, value = pol.forward_torch(torch.from_numpy(local), torch.from_numpy(coarse))
    E = local.shape[0]
    assert tuple(move.shape) == (E, 9) and tuple(shoot.shape) == (E, 2) and tuple(value.shape) == (E,)
    out64, bound = bref.outputs_f64(w, d, local, coarse)
    got = torch.cat([move, shoot, value[:, None]], 1).numpy().astype(np.float64)
    assert (np.abs(got - out64) <= bound).all()
    _, logits, val = bref.host_act(w, d, local, coarse, se, ep)
    host = np.concatenate([logits, val[:, None]], 1).astype(np.float64)
    assert (np.abs(got - host) <= 2 * bound).all()
    # leading (K, E) dims, and gradients to a trainer's own leaves: all five tensors
    leaves = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in w.items()}
    m2, s2, v2 = pol.forward_torch(torch.from_numpy(local)[None], torch.from_numpy(coarse)[None], weights=leaves)
    assert tuple(m2.shape) == (1, E, 9) and tuple(s2.shape) == (1, E, 2) and tuple(v2.shape) == (1, E)
    (torch.log_softmax(m2, -1)[..., 0].sum() + torch.log_softmax(s2, -1)[..., 1].sum() + v2.sum()).backward()
    assert all(t.grad is not None and t.grad.abs().sum() > 0 for t in leaves.values())


def test_policy_validation():
    import torch

    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    for hidden in (16, 48, 512, 0):
        with pytest.raises(ValueError, match="hidden"):
            BulldozerPolicy((32, 256), 1, 8, hidden, device="cpu")
    with pytest.raises(ValueError, match="radius"):
        BulldozerPolicy((32, 256), 32, 8, 32, device="cpu")
    with pytest.raises(ValueError, match="block"):
        BulldozerPolicy((32, 256), 1, 3, 32, device="cpu")
    pol = BulldozerPolicy((32, 256), 1, 8, 32, device="cpu")
    v0 = pol.version
    with pytest.raises(ValueError, match="w_out"):
        pol.w_out = torch.zeros((32, 10))                      # the helicopter's shape
    with pytest.raises(ValueError, match="b1"):
        pol.b1 = torch.zeros(32, dtype=torch.float64)          # dtype
    with pytest.raises(ValueError, match="w_local"):
        pol.w_local = torch.zeros((4, 9, 32)).permute(1, 0, 2)  # not contiguous
    with pytest.raises(ValueError, match="missing"):
        pol.load({"b1": np.zeros(32)})
    with pytest.raises(ValueError, match="shape"):
        pol.load({**pol.state_dict(), "b2": np.zeros(10)})
    with pytest.raises(ValueError, match="dtype"):
        pol.load({**pol.state_dict(), "b2": np.zeros(12, np.int32)})
    assert pol.version == v0
    new_b1 = torch.ones(32)
    pol.b1 = new_b1                                            # a replaced tensor moves the version and the struct
    assert pol.version == v0 + 1 and pol.struct.b1 == new_b1.data_ptr()
    pol.load({k: v.double().numpy() for k, v in pol.state_dict().items()})   # any float dtype, arrays
    assert pol.version == v0 + 2 and pol.b1.dtype is torch.float32 and torch.equal(pol.b1, new_b1)


# ------------------------------------------------------------------ the argument contract, in both builds
def A(i):
    """Fake address number i: 16-B aligned, 1 MiB from its neighbours."""
    return 0x5000000 + 0x100000 * i


_ORDER = ("p", "C", "local", "coarse", "steps_elapsed", "episode", "env_offset", "policy_seed", "greedy", "action",
          "logits", "value", "E", "stream")
_WEIGHTS = ("w_local", "w_coarse", "b1", "w_out", "b2")
_BASE = dict(C=8, local=A(0), coarse=A(1), steps_elapsed=A(2), episode=A(3), env_offset=0, policy_seed=0, greedy=0,
             action=A(4), logits=A(5), value=A(6), E=2, stream=None)
_C_RANGE = "C = 2 Hc Wc, at most 15088"
# (text, deviation from the baseline): every text names its argument; the order of the checks shows in the pairs
_SHARED = [("policy is null", dict(p=None))] + [(f"policy.{n} is null", {"p_" + n: None}) for n in _WEIGHTS] + [
    ("policy.w_local is null", dict(p_w_local=None, p_b2=None)),
    ("policy.radius in [0, 31]", dict(p_radius=32)), ("policy.radius in [0, 31]", dict(p_radius=-1)),
    ("policy.radius in [0, 31]", dict(p_radius=32, p_block=3)),
    ("policy.block must be a power of two in [1, 64]", dict(p_block=3)),
    ("policy.block must be a power of two in [1, 64]", dict(p_block=128)),
    ("policy.block must be a power of two in [1, 64]", dict(p_block=0, p_hidden=16)),
    ("policy.hidden must be a power of two in [32, 256]", dict(p_hidden=16)),
    ("policy.hidden must be a power of two in [32, 256]", dict(p_hidden=48)),
    ("policy.hidden must be a power of two in [32, 256]", dict(p_hidden=512, local=None)),
    ("local is null", dict(local=None)), ("local is null", dict(local=None, coarse=None)),
    ("coarse is null", dict(coarse=None)), ("steps_elapsed is null", dict(steps_elapsed=None)),
    ("action is null", dict(action=None)), ("action is null", dict(action=None, E=0)),
    ("E > 0", dict(E=0)), ("E > 0", dict(E=-1, C=3)),
    (_C_RANGE, dict(C=0)), (_C_RANGE, dict(C=3)), (_C_RANGE, dict(C=15090))]
# refused by the device build alone (the kernels' 16-B loads), after every shared check
_DEVICE = [("policy.w_local and policy.w_coarse must be 16-B aligned", dict(p_w_local=A(20) + 8)),
           ("policy.w_local and policy.w_coarse must be 16-B aligned", dict(p_w_coarse=A(20) + 4, C=15088)),
           (_C_RANGE, dict(p_w_local=A(20) + 8, C=15090))]


def _libs():
    from gymca_amd import _lib

    return {"host": _lib.load_cpu(), "device": _lib.load()}


def _call(build, over):
    from gymca_amd import _lib

    p = _lib.BulldozerPolicyStruct()
    p.radius, p.block, p.hidden = 1, 4, 32
    for i, n in enumerate(_WEIGHTS):
        setattr(p, n, A(10 + i))
    args = dict(_BASE, p=ctypes.byref(p))
    for k, v in over.items():
        if k.startswith("p_"):
            setattr(p, k[2:], v)
        else:
            args[k] = v
    lib = _libs()[build]
    status = lib.gca_bulldozer_policy_act(*[args[n] for n in _ORDER])
    return status, lib.gca_last_error().decode()


@pytest.mark.parametrize("build", ["host", "device"])
def test_argument_errors_name_the_argument(build):
    from gymca_amd import _lib

    assert len(_ORDER) == len(_lib._SIGNATURES["gca_bulldozer_policy_act"][0])
    for text, over in _SHARED:
        status, msg = _call(build, over)
        assert status == 1 and msg == f"argument: bulldozer_policy_act: {text}", (over, status, msg)


def test_both_builds_refuse_alike_and_the_device_checks_alignment():
    for _, over in _SHARED:
        host, device = _call("host", over), _call("device", over)
        assert host == device and host[0] == 1, (over, host, device)
    for text, over in _DEVICE:
        status, msg = _call("device", over)
        assert status == 1 and msg == f"argument: bulldozer_policy_act: {text}", (over, status, msg)


def test_the_rollout_refuses_before_any_launch():
    """gca_bulldozer_policy_rollout exists in the device build only; every call here is refused by an argument check,
    so the library answers without a GPU."""
    from gymca_amd import _lib

    lib = _lib.load()
    assert not hasattr(_lib.load_cpu(), "gca_bulldozer_policy_rollout")
    order = ("p", "policy", "policy_seed", "greedy", "K", "action_out", "logits_out", "value_out", "reward_out",
             "terminated_out", "truncated_out", "local_out", "coarse_out", "scratch", "autoreset", "reset_seed",
             "max_steps", "cdf", "values", "episode", "last_length", "terminated", "truncated", "accu", "steps", "done",
             "wind", "wind_stride", "rng_step", "parity", "buf0", "buf1", "H", "W", "pos", "counts", "hit", "reward",
             "steps_elapsed", "E", "stream")
    assert len(order) == len(_lib._SIGNATURES["gca_bulldozer_policy_rollout"][0])
    ptrs = [n for n in order if n not in ("p", "policy", "policy_seed", "greedy", "K", "autoreset", "reset_seed",
                                          "max_steps", "wind_stride", "H", "W", "E", "stream")]

    def call(over):
        bp = _lib.BulldozerParams()
        bp.empty, bp.tree, bp.fire = 0, 3, 25
        for a in range(9):
            bp.t_move[a] = 0.3
        bp.t_shoot[1] = 0.25
        pol = _lib.BulldozerPolicyStruct()
        pol.radius, pol.block, pol.hidden = 1, 8, 32
        for i, n in enumerate(_WEIGHTS):
            setattr(pol, n, A(60 + i))
        args = dict({n: A(i) for i, n in enumerate(ptrs)}, p=ctypes.byref(bp), policy=ctypes.byref(pol), policy_seed=0,
                    greedy=0, K=2, autoreset=1, reset_seed=0, max_steps=5, wind_stride=9, H=32, W=256, E=2, stream=None)
        for k, v in over.items():
            if k.startswith("pol_"):
                setattr(pol, k[4:], v)
            elif k.startswith("p_"):
                setattr(bp, k[2:], v)
            else:
                args[k] = v
        status = lib.gca_bulldozer_policy_rollout(*[args[n] for n in order])
        return status, lib.gca_last_error().decode()

    head = "argument: bulldozer_policy_rollout: "
    for text, over in [("null argument, empty batch or K < 0", dict(K=-1)),
                       ("null argument, empty batch or K < 0", dict(pos=None)),
                       ("W must be 256 or 512 (the row-stream CA)", dict(W=64)),
                       ("steps_elapsed is null", dict(steps_elapsed=None)),
                       ("buf0 and buf1 must differ", dict(buf1=A(ptrs.index("buf0")))),
                       ("max_steps >= 0", dict(max_steps=-1)),
                       ("autoreset needs cdf, values and episode", dict(episode=None)),
                       ("env_offset >= 0", dict(p_env_offset=-1)),
                       ("policy is null", dict(policy=None)),
                       ("policy.b2 is null", dict(pol_b2=None)),
                       ("policy.hidden must be a power of two in [32, 256]", dict(pol_hidden=100, K=0)),
                       ("C = 2 Hc Wc, at most 15088", dict(pol_block=1)),
                       ("policy.w_local and policy.w_coarse must be 16-B aligned", dict(pol_w_coarse=A(70) + 4)),
                       # block 4 is off the resident path: the K x 3 launches need somewhere to keep a step's window
                       ("this shape runs K x 3 launches and needs `scratch` for the records not kept",
                        dict(pol_block=4, scratch=None, local_out=None)),
                       ("scratch 4-B aligned", dict(scratch=A(71) + 2))]:
        status, msg = call(over)
        assert status == 1 and msg == head + text, (over, status, msg)
    # K == 0 is a no-op once the arguments are valid; episode is optional without autoreset
    assert call(dict(K=0))[0] == 0
    assert call(dict(K=0, autoreset=0, episode=None, cdf=None, values=None))[0] == 0


C_LAYOUT = r"""
#include <stdio.h>
#include <stddef.h>
#include "gca.h"
#define P(f) printf("%s %zu\n", #f, offsetof(gca_bulldozer_policy, f));
int main(void) {
  printf("sizeof %zu\n", sizeof(gca_bulldozer_policy));
  P(radius) P(block) P(hidden) P(reserved) P(w_local) P(w_coarse) P(b1) P(w_out) P(b2)
  printf("tag %u\n", GCA_TAG_BPOLICY);
  return 0;
}
"""


def test_policy_struct_layout_matches_the_header(tmp_path):
    from gymca_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text(C_LAYOUT)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.rsplit(" ", 1) for line in out if line)
    assert ctypes.sizeof(_lib.BulldozerPolicyStruct) == int(got.pop("sizeof"))
    assert int(got.pop("tag")) == _lib.TAG_BPOLICY == bref.TAG_BPOLICY == 0x42504F4C
    assert len(got) == len(_lib.BulldozerPolicyStruct._fields_)
    for f, off in got.items():
        assert getattr(_lib.BulldozerPolicyStruct, f).offset == int(off), f
    assert {"gca_bulldozer_policy_act", "gca_bulldozer_policy_rollout"} <= set(_lib.EXPORTED_SYMBOLS)
    assert "gca_bulldozer_policy_act" in _lib.CPU_BULLDOZER_POLICY_SYMBOLS
    assert _lib.load().gca_version() == 1
