"""CPU: gca_advanced_policy_act of the host build (include/gca.h "advanced policy") against the composition it is defined
by -- the numpy restatement of the observation (tests/_policy_obs_ref.py), then the bulldozer policy on the widened
time_step (tests/_bulldozer_policy_ref.py) -- bit for bit; the action's stride, the nullable outputs, and the argument
contract, refused alike by the host and the device build before they touch memory. No GPU."""
import ctypes

import numpy as np
import pytest

import _advanced_policy_ref as aref
import _bulldozer_policy_ref as bref


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("shape", aref.HOST_SHAPES)
def test_host_build_equals_the_composition_of_the_restatements(shape, greedy):
    d, w, planes, pos, ts = aref.make_case(shape)
    E, H, W = planes.shape
    assert (planes == 7).any() and all((planes == c).any() for c in aref.CODES)
    assert (pos[0] == 0).all() and pos[1, 0] >= H and pos[1, 1] < 0  # a corner, a position outside the grid
    want_a, want_l, want_v, want_lo, want_co, out32 = aref.composed(d, w, planes, pos, ts, env_offset=5, greedy=greedy)
    action, logits, value, local, coarse = aref.host_act(d, w, planes, pos, ts, env_offset=5, greedy=greedy)
    assert np.array_equal(local, want_lo)
    assert (local == 3).any() and (local != 3).any()
    assert np.array_equal(aref.bits(coarse), aref.bits(want_co))
    assert coarse[0, 1, 0, 0] == 1.0 and coarse[E - 1, 0, -1, -1] > 0  # the all-FIRE block, the all-TREE block
    assert np.array_equal(aref.bits(logits), aref.bits(want_l)) and np.array_equal(aref.bits(value), aref.bits(want_v))
    assert np.array_equal(aref.bits(logits), aref.bits(out32[:, :11]))
    assert np.array_equal(aref.bits(value), aref.bits(out32[:, 11]))
    assert np.array_equal(action, want_a)
    assert ((0 <= action[:, 0]) & (action[:, 0] <= 8) & (0 <= action[:, 1]) & (action[:, 1] <= 1)).all()
    if greedy:
        assert np.array_equal(action, bref.greedy_ref(logits))
    else:
        # the draw: Philox(((uint32)time_step, env_offset + e, 0, BPOL), seed)
        u_m, u_s = bref.policy_u(aref.SEED, 5 + np.arange(E), ts.astype(np.int64), np.zeros(E))
        ref_action, near = bref.sample_ref(logits, u_m, u_s)
        assert np.array_equal(action[~near], ref_action[~near])
        other, *_ = aref.host_act(d, w, planes, pos, ts + 1, env_offset=5)
        moved, *_ = aref.host_act(d, w, planes, pos, ts, env_offset=6)
        assert not (np.array_equal(other, action) and np.array_equal(moved, action))  # time_step and env id key it


@pytest.mark.parametrize("shape", aref.HOST_SHAPES)
def test_stride_three_keeps_the_third_column_and_null_outputs_change_nothing_else(shape):
    d, w, planes, pos, ts = aref.make_case(shape, seed=1)
    action, logits, value, local, coarse = aref.host_act(d, w, planes, pos, ts)
    a3, l3, v3, lo3, co3 = aref.host_act(d, w, planes, pos, ts, stride=3)
    assert (a3[:, 2] == aref.SENTINEL).all() and np.array_equal(a3[:, :2], action)
    assert np.array_equal(aref.bits(l3), aref.bits(logits)) and np.array_equal(aref.bits(v3), aref.bits(value))
    assert np.array_equal(lo3, local) and np.array_equal(aref.bits(co3), aref.bits(coarse))
    a0, l0, v0, lo0, co0 = aref.host_act(d, w, planes, pos, ts, logits=False, value=False, local=False, coarse=False)
    assert l0 is None and v0 is None and lo0 is None and co0 is None and np.array_equal(a0, action)
    for drop in ("logits", "value", "local", "coarse"):
        got = dict(zip(("action", "logits", "value", "local", "coarse"),
                       aref.host_act(d, w, planes, pos, ts, **{drop: False})))
        assert got.pop(drop) is None
        assert np.array_equal(got.pop("action"), action)
        full = dict(logits=logits, value=value, local=local, coarse=coarse)
        for name, t in got.items():
            assert np.array_equal(t.view(np.uint8), full[name].view(np.uint8)), (drop, name)


# ------------------------------------------------------------------ the argument contract, in both builds
def A(i):
    """Fake address number i: 16-B aligned, 1 MiB from its neighbours."""
    return 0x5000000 + 0x100000 * i


_WEIGHTS = ("w_local", "w_coarse", "b1", "w_out", "b2")
_BASE = dict(grid=A(0), pos=A(1), time_step=A(2), E=2, H=32, W=256, empty=0, tree=1, fire=2, env_offset=0, policy_seed=0,
             greedy=0, action=A(3), action_stride=2, logits=A(4), value=A(5), local_out=A(6), coarse_out=A(7),
             stream=None)
_C_RANGE = "C = 2 Hc Wc, at most 15088"
# (text, deviation from the baseline): the order of the checks shows in the pairs
_SHARED = [("policy is null", dict(policy=None))] + [(f"policy.{n} is null", {"p_" + n: None}) for n in _WEIGHTS] + [
    ("policy.radius in [0, 31]", dict(p_radius=32)), ("policy.radius in [0, 31]", dict(p_radius=-1, grid=None)),
    ("policy.block must be a power of two in [1, 64]", dict(p_block=3)),
    ("policy.block must be a power of two in [1, 64]", dict(p_block=128, p_hidden=16)),
    ("policy.hidden must be a power of two in [32, 256]", dict(p_hidden=48, pos=None)),
    ("grid is null", dict(grid=None)), ("grid is null", dict(grid=None, pos=None)),
    ("pos is null", dict(pos=None)), ("time_step is null", dict(time_step=None, action=None)),
    ("action is null", dict(action=None)), ("action is null", dict(action=None, E=0)),
    ("E, H, W must be positive", dict(E=0)), ("E, H, W must be positive", dict(H=0)),
    ("E, H, W must be positive", dict(W=-1, action_stride=1)),
    ("grid too large (H * W < 2^30)", dict(H=32768, W=32768)),
    ("the codes must be u8 values", dict(fire=256)), ("the codes must be u8 values", dict(empty=-1, action_stride=1)),
    ("action_stride >= 2", dict(action_stride=1)), ("action_stride >= 2", dict(action_stride=0, p_block=1)),
    (_C_RANGE, dict(p_block=1)), (_C_RANGE, dict(H=4096, W=4096, p_block=8))]
# refused by the device build alone (the kernel's 16-B loads of the weights), after every shared check
_DEVICE = [("policy.w_local and policy.w_coarse must be 16-B aligned", dict(p_w_local=A(20) + 8)),
           ("policy.w_local and policy.w_coarse must be 16-B aligned", dict(p_w_coarse=A(20) + 4)),
           (_C_RANGE, dict(p_w_local=A(20) + 8, p_block=1))]


def _call(build, over):
    from gymca_amd import _lib

    p = _lib.BulldozerPolicyStruct()
    p.radius, p.block, p.hidden = 1, 8, 32
    for i, n in enumerate(_WEIGHTS):
        setattr(p, n, A(10 + i))
    args = dict(_BASE, policy=ctypes.byref(p))
    for k, v in over.items():
        if k.startswith("p_"):
            setattr(p, k[2:], v)
        else:
            args[k] = v
    lib = {"host": _lib.load_cpu, "device": _lib.load}[build]()
    status = lib.gca_advanced_policy_act(*[args[n] for n in aref.ORDER])
    return status, lib.gca_last_error().decode()


@pytest.mark.parametrize("build", ["host", "device"])
def test_argument_errors_name_the_argument(build):
    from gymca_amd import _lib

    assert len(aref.ORDER) == len(_lib._SIGNATURES["gca_advanced_policy_act"][0])
    for text, over in _SHARED:
        status, msg = _call(build, over)
        assert status == 1 and msg == f"argument: advanced_policy_act: {text}", (over, status, msg)


def test_both_builds_refuse_alike_and_the_device_checks_alignment():
    for _, over in _SHARED:
        host, device = _call("host", over), _call("device", over)
        assert host == device and host[0] == 1, (over, host, device)
    for text, over in _DEVICE:
        status, msg = _call("device", over)
        assert status == 1 and msg == f"argument: advanced_policy_act: {text}", (over, status, msg)


def test_the_symbol_is_exported_by_both_builds():
    from gymca_amd import _lib

    assert "gca_advanced_policy_act" in _lib.EXPORTED_SYMBOLS
    assert "gca_advanced_policy_act" in _lib.CPU_BULLDOZER_POLICY_SYMBOLS
    assert "gca_advanced_policy_act" not in _lib.CPU_SYMBOLS
    assert hasattr(_lib.load_cpu(), "gca_advanced_policy_act") and hasattr(_lib.load(), "gca_advanced_policy_act")
