"""CPU: the argument contract of the entry points that libgca_hip.so and libgca_cpu.so both export (csrc/gca_args.h).
Per entry point a baseline of valid arguments on fake, aligned, non-overlapping addresses and a list of deviations from
it; every call made here is refused by an argument check, which both builds make before they touch memory or the GPU,
so the device library answers without one. Each deviation is refused with status 1 and one exact text, the same in
both builds; the checks that only one build makes have their own cases for that build. gca_adam_step(_workspace) and
gca_permutation are covered in the same way by tests/test_adam_host.py."""
import ctypes

import numpy as np
import pytest


def A(i):
    """Fake address number i: 16-B aligned, 1 MiB from its neighbours (more than any array of the baselines)."""
    return 0x5000000 + 0x100000 * i


_HELI_STATE = ("thresholds", "freeze", "rng_step", "parity", "buf0", "buf1", "H", "W", "pos", "counts", "hit", "reward",
               "steps_elapsed")
_HELI_HEAD = ("empty", "tree", "fire", "max_freeze", "seed", "env_offset")
_ORDER = {
    "gca_philox": ("ctr", "key0", "key1", "out", "n", "stream"),
    "gca_count_cells": ("grid", "E", "H", "W", "v0", "v1", "v2", "counts", "stream"),
    "gca_move_modify": ("p", "action", "pos", "grid", "H", "W", "hit", "E", "stream"),
    "gca_ds_count_draws": ("grid", "E", "H", "W", "empty", "tree", "fire", "n_draws", "stream"),
    "gca_ds_step": ("grid_in", "grid_out", "E", "H", "W", "empty", "tree", "fire", "thresholds", "uniforms",
                    "uniform_offset", "seed", "rng_step", "env_offset", "counts", "stream"),
    "gca_helicopter_step": _HELI_HEAD + ("action", "action_seed", "action_out") + _HELI_STATE + ("meet", "E", "stream"),
    "gca_helicopter_rollout": _HELI_HEAD + ("actions", "action_seed", "K", "action_out", "reward_out", "hit_out")
                              + _HELI_STATE + ("E", "stream"),
    "gca_bulldozer_reset_where": ("p", "reset_seed", "mask", "max_steps", "set_episode", "cdf", "values", "done",
                                  "terminated_out", "truncated_out", "episode", "last_length_out", "accu", "parity",
                                  "buf0", "buf1", "H", "W", "pos", "counts", "hit", "steps_elapsed", "E", "stream"),
    "gca_policy_observation": ("buf0", "buf1", "parity", "pos", "E", "H", "W", "empty", "tree", "fire", "radius",
                               "block", "form", "local_out", "coarse_out", "stream"),
    "gca_helicopter_policy_act": ("p", "C", "local", "coarse", "rng_step", "env_offset", "policy_seed", "greedy",
                                  "action", "logits", "value", "E", "stream"),
    "gca_helicopter_policy_rollout": _HELI_HEAD + ("p", "policy_seed", "greedy", "K", "action_out", "logits_out",
                                                   "value_out", "reward_out", "hit_out", "local_out", "coarse_out",
                                                   "scratch") + _HELI_STATE + ("E", "stream"),
    "gca_gae": ("reward", "value", "next_value", "terminal", "gamma", "gamma_lambda", "K", "E", "advantage", "returns",
                "stream"),
    "gca_helicopter_policy_grad_workspace": ("p", "C", "N"),
    "gca_helicopter_policy_grad": ("p", "C", "local", "coarse", "action", "old_logits", "advantage", "returns", "T",
                                   "idx", "N", "clip_coef", "ent_coef", "vf_coef", "norm_adv", "g_w_local",
                                   "g_w_coarse", "g_b1", "g_w_out", "g_b2", "stats", "workspace", "workspace_bytes",
                                   "stream"),
}
_POINTERS = ("ctr", "out", "grid", "counts", "action", "pos", "hit", "n_draws", "grid_in", "grid_out", "thresholds",
             "rng_step", "action_out", "freeze", "parity", "buf0", "buf1", "reward", "steps_elapsed", "meet", "actions",
             "reward_out", "hit_out", "cdf", "values", "done", "episode", "accu", "local_out", "coarse_out", "local",
             "coarse", "logits", "value", "logits_out", "value_out", "next_value", "advantage", "returns", "old_logits",
             "g_w_local", "g_w_coarse", "g_b1", "g_w_out", "g_b2", "stats", "workspace")
_WEIGHTS = ("w_local", "w_coarse", "b1", "w_out", "b2")
# valid everywhere: an 8 x 8 grid of codes 0 / 1 / 2, two envs; a policy of radius 1, block 4, 32 hidden units (a 3 x 3
# window and C = 2 * 2 * 2 coarse values); T = 16 records, a minibatch of 4. Pointers not named here are null.
_BASE = dict({n: A(i) for i, n in enumerate(_POINTERS)}, key0=0, key1=0, seed=0, env_offset=0, action_seed=0,
             reset_seed=0, max_steps=0, policy_seed=0, greedy=0, E=2, H=8, W=8, n=4, v0=0, v1=1, v2=2, empty=0, tree=1,
             fire=2, max_freeze=3, K=2, radius=1, block=4, form=0, C=8, gamma=0.99, gamma_lambda=0.95, T=16, N=4,
             clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, norm_adv=1, workspace_bytes=1 << 40, set_episode=-1)
_NULL = "null argument"
_SIZES = "E, H, W > 0 and max_freeze >= 0"
_CODES = "three distinct u8 codes"


def _env_cases(k_too):
    """The env group of the three helicopter entry points (the entry point heads each text); K where there is one."""
    cases = [(_NULL, {n: None}) for n in _HELI_STATE if n not in ("H", "W")]
    cases += [(_SIZES, dict(E=0)), (_SIZES, dict(H=0)), (_SIZES, dict(W=-1)), (_SIZES, dict(max_freeze=-1)),
              (_NULL, dict(pos=None, E=0)),
              ("buf0 and buf1 must differ", dict(buf1=_BASE["buf0"])),
              ("grid too large", dict(H=1 << 15, W=1 << 15)),
              ("grid too large", dict(H=1 << 15, W=1 << 15, tree=0)),
              (_CODES, dict(H=1 << 15, W=(1 << 15) - 1, tree=0)),   # H * W = 2^30 - 2^15 is not too large
              (_CODES, dict(tree=0)), (_CODES, dict(fire=1)), (_CODES, dict(fire=0)), (_CODES, dict(fire=256)),
              (_CODES, dict(empty=-1))]
    if k_too:
        cases += [("K >= 0", dict(K=-1)), (_CODES, dict(K=-1, fire=0))]
    return cases


_POLICY = [("null weights", dict(p=None))] + [("null weights", {"p_" + n: None}) for n in _WEIGHTS] + [
    ("radius in [0, 31]", dict(p_radius=32)), ("radius in [0, 31]", dict(p_radius=-1)),
    ("radius in [0, 31]", dict(p_radius=32, p_block=3)),
    ("block must be a power of two in [1, 64]", dict(p_block=3)),
    ("block must be a power of two in [1, 64]", dict(p_block=128)),
    ("hidden must be a power of two in [32, 256]", dict(p_hidden=16)),
    ("hidden must be a power of two in [32, 256]", dict(p_hidden=48)),
    ("hidden must be a power of two in [32, 256]", dict(p_hidden=512))]
_C_RANGE = "C = 2 Hc Wc, at most 15088"
_GRAD_WS = ("helicopter_policy_grad_workspace: radius in [0, 31], hidden a power of two in [32, 256], "
            "C = 2 Hc Wc at most 15088, N >= 1")
_ALIAS = "the outputs may alias neither each other nor the weights"

# name -> (what heads the texts, [(text, deviation from the baseline)]): refused alike by both builds
_SHARED = {
    "gca_philox": ("", [("ctr/out required", d) for d in (dict(ctr=None), dict(out=None), dict(n=-1))]),
    "gca_count_cells": ("", [("grid/counts and positive sizes required", d) for d in
                             (dict(grid=None), dict(counts=None), dict(E=0), dict(H=0), dict(W=-1))]),
    "gca_move_modify": ("move_modify: ", [("bad arguments", d) for d in
                                          (dict(p=None), dict(action=None), dict(pos=None), dict(E=0), dict(H=0),
                                           dict(W=0))]),
    "gca_ds_count_draws": ("ds_count_draws: ", [("bad arguments", d) for d in
                                                (dict(grid=None), dict(n_draws=None), dict(E=0), dict(H=-1), dict(W=0))]
                           + [("grid too large", dict(H=1 << 15, W=1 << 15)),
                              ("bad arguments", dict(H=1 << 15, W=1 << 15, n_draws=None))]),
    "gca_ds_step": ("ds_step: ", [("bad arguments", d) for d in
                                  (dict(grid_in=None), dict(grid_out=None), dict(thresholds=None), dict(E=0), dict(H=0),
                                   dict(W=0))]
                    + [("in-place update is not supported", dict(grid_out=_BASE["grid_in"])),
                       ("uniforms need uniform_offset", dict(uniforms=A(60))),
                       ("grid too large", dict(H=1 << 15, W=1 << 15)),
                       ("grid too large", dict(H=1 << 15, W=1 << 15, uniforms=A(60), uniform_offset=A(61))),
                       ("uniforms need uniform_offset", dict(H=1 << 15, W=1 << 15, uniforms=A(60)))]),
    "gca_helicopter_step": ("helicopter_step: ", _env_cases(False)),
    "gca_helicopter_rollout": ("helicopter_rollout: ", _env_cases(True)),
    "gca_bulldozer_reset_where": ("bulldozer_reset_where: ", [
        (_NULL, {n: None}) for n in ("p", "cdf", "values", "done", "episode", "accu", "parity", "buf0", "buf1", "pos",
                                     "counts", "hit", "steps_elapsed")] + [
        ("E, H, W must be positive", dict(E=0)), ("E, H, W must be positive", dict(H=0)),
        ("E, H, W must be positive", dict(W=-1)), (_NULL, dict(E=0, hit=None)),
        ("H, W < 32768", dict(H=32768)), ("H, W < 32768", dict(W=32768)),
        ("buf0 and buf1 must differ", dict(buf1=_BASE["buf0"])),
        ("buf0 and buf1 must differ", dict(buf1=_BASE["buf0"], H=32767, W=32767)),   # 32767 is not too large
        ("max_steps >= 0 and set_episode in [-1, 2^32)", dict(max_steps=-1)),
        ("max_steps >= 0 and set_episode in [-1, 2^32)", dict(set_episode=-2)),
        ("max_steps >= 0 and set_episode in [-1, 2^32)", dict(set_episode=1 << 32)),
        ("env_offset >= 0", dict(p_env_offset=-1)),
        ("env_offset >= 0", dict(p_env_offset=-1, set_episode=(1 << 32) - 1))]),   # 2^32 - 1 is an episode
    "gca_policy_observation": ("policy_observation: ", [
        ("buf0 required, and buf1 with parity", dict(buf0=None)),
        ("buf0 required, and buf1 with parity", dict(buf1=None)),
        ("local_out or coarse_out required", dict(local_out=None, coarse_out=None)),
        ("local_out or coarse_out required", dict(local_out=None, coarse_out=None, buf1=None, parity=None)),
        ("local_out needs pos", dict(pos=None)),
        ("E, H, W must be positive", dict(E=0)), ("E, H, W must be positive", dict(H=0)),
        ("E, H, W must be positive", dict(W=0)),
        ("grid too large (H * W < 2^30)", dict(H=1 << 15, W=1 << 15)),
        ("the codes must be u8 values", dict(H=1 << 15, W=(1 << 15) - 1, fire=256)),
        ("the codes must be u8 values", dict(tree=-1)),
        ("radius in [0, 31]", dict(radius=32)), ("radius in [0, 31]", dict(radius=-1)),
        ("block must be a power of two in [1, 64]", dict(block=3)),
        ("block must be a power of two in [1, 64]", dict(block=0)),
        ("block must be a power of two in [1, 64]", dict(block=128)),
        ("block must be a power of two in [1, 64]", dict(block=128, radius=31)),   # 31 is a radius
        ("form 0 (by shape), 1 (generic) or 2 (rows)", dict(form=3)),
        ("form 0 (by shape), 1 (generic) or 2 (rows)", dict(form=-1, block=64)),   # 64 is a block
        ("form 2 (rows) needs W = 256 / 512, block = 8 / 16 / 32 and H % block == 0", dict(form=2)),
        ("form 2 (rows) needs W = 256 / 512, block = 8 / 16 / 32 and H % block == 0", dict(form=2, W=256, block=8, H=12)),
        ("form 2 (rows) needs W = 256 / 512, block = 8 / 16 / 32 and H % block == 0",
         dict(form=2, W=512, block=64, H=64))]),
    "gca_helicopter_policy_act": ("", [("helicopter_policy: " + t, d) for t, d in _POLICY] + [
        ("helicopter_policy_act: " + t, d) for t, d in
        [(_NULL, {n: None}) for n in ("local", "coarse", "rng_step", "action")]
        + [("E > 0", dict(E=0)), (_NULL, dict(E=0, local=None)),
           (_C_RANGE, dict(C=0)), (_C_RANGE, dict(C=3)), (_C_RANGE, dict(C=15090)), ("E > 0", dict(C=15090, E=-1))]]),
    "gca_helicopter_policy_rollout": ("", [("helicopter_policy_rollout: " + t, d) for t, d in _env_cases(True) + [
        ("policy required", dict(p=None)), ("policy required", dict(p_block=0)),
        ("policy required", dict(p_block=-4, p_radius=32)), ("K >= 0", dict(K=-1, p=None)),
        # block = 1: C = 2 H W = 2^30, one too many for an int's worth of floats; then the policy itself
        ("coarse map too large", dict(H=1 << 15, W=1 << 14, p_block=1)),
        ("coarse map too large", dict(H=1 << 15, W=1 << 14, p_block=1, p_b2=None))]]
        + [("helicopter_policy: " + t, d) for t, d in _POLICY if d != dict(p=None) and "p_block" not in d]
        + [("helicopter_policy: block must be a power of two in [1, 64]", dict(p_block=3)),
           ("helicopter_policy: block must be a power of two in [1, 64]", dict(p_block=128)),
           ("helicopter_policy: null weights", dict(H=1 << 15, W=(1 << 14) - 1, p_block=1, p_b2=None))]),
    "gca_gae": ("gae: ", [("K >= 0", dict(K=-1)), ("K >= 0", dict(K=-1, E=0)), ("E > 0", dict(E=0)),
                          ("E > 0", dict(E=-3, reward=None))]
                + [(_NULL, {n: None}) for n in ("reward", "value", "next_value", "advantage", "returns")]),
    "gca_helicopter_policy_grad": ("", [("helicopter_policy: " + t, d) for t, d in _POLICY] + [
        ("helicopter_policy_grad: " + t, d) for t, d in
        [("null record", {n: None}) for n in ("local", "coarse", "action", "old_logits", "advantage", "returns")]
        + [("null output or workspace", {n: None})
           for n in ("g_w_local", "g_w_coarse", "g_b1", "g_w_out", "g_b2", "stats", "workspace")]
        + [("null record", dict(local=None, stats=None)),
           (_C_RANGE, dict(C=0)), (_C_RANGE, dict(C=3)), (_C_RANGE, dict(C=15090)), (_C_RANGE, dict(C=15090, T=0)),
           ("1 <= T < 2^31", dict(C=15088, T=0)),   # (15088 + 1296) * 4 = 65536: the largest C is not refused
           ("1 <= T < 2^31", dict(T=0)), ("1 <= T < 2^31", dict(T=1 << 31)),
           ("N >= 1", dict(T=(1 << 31) - 1, N=0)), ("N >= 1", dict(N=0)), ("N >= 1", dict(N=-1, clip_coef=-1.0)),
           ("N <= T without idx", dict(N=17)), ("clip_coef >= 0", dict(N=17, idx=A(62), clip_coef=-0.5)),
           ("clip_coef >= 0", dict(clip_coef=-0.5)), ("clip_coef >= 0", dict(clip_coef=float("nan"))),
           ("workspace smaller than gca_helicopter_policy_grad_workspace", dict(workspace_bytes=64)),
           ("workspace smaller than gca_helicopter_policy_grad_workspace", dict(workspace_bytes=64, workspace=A(63) + 8)),
           ("workspace, w_local, w_coarse and b1 16-B aligned", dict(workspace=A(63) + 8)),
           ("workspace, w_local, w_coarse and b1 16-B aligned", dict(p_w_local=A(64) + 4)),
           ("workspace, w_local, w_coarse and b1 16-B aligned", dict(p_w_coarse=A(64) + 8)),
           ("workspace, w_local, w_coarse and b1 16-B aligned", dict(p_b1=A(64) + 4, g_b1=_BASE["g_w_local"])),
           (_ALIAS, dict(g_b1=_BASE["g_w_local"])),                 # two outputs
           (_ALIAS, dict(g_b2=_BASE["stats"] + 28)),                # the last float of stats
           (_ALIAS, dict(g_w_local="p_w_local")),                   # an output on its weights
           (_ALIAS, dict(stats="p_b2"))]]),
}

# build -> name -> [(text, deviation)]: refused by that build alone; the other build would run the call
_OWN = {
    "device": {
        # the rows kernel's 8-B loads, and the launch's 32-bit workgroup count
        "gca_policy_observation": [
            ("policy_observation: form 2 (rows) needs 8-B aligned planes", dict(form=2, W=256, block=8, buf0=A(70) + 4)),
            ("policy_observation: form 2 (rows) needs 8-B aligned planes", dict(form=2, W=512, block=8, buf1=A(70) + 4)),
            ("policy_observation: too many envs for one launch", dict(E=1 << 20, H=1024, W=1024, block=1))],
        # the kernels' 16-B loads of the weights, after every shared check; C = 15088 is not refused for C
        "gca_helicopter_policy_act": [
            ("helicopter_policy: w_local and w_coarse must be 16-B aligned", dict(p_w_local=A(70) + 8)),
            ("helicopter_policy: w_local and w_coarse must be 16-B aligned", dict(p_w_coarse=A(70) + 4)),
            ("helicopter_policy: w_local and w_coarse must be 16-B aligned", dict(p_w_local=A(70) + 8, C=15088)),
            ("helicopter_policy_act: " + _C_RANGE, dict(p_w_local=A(70) + 8, C=15090))],
        # 256 x 256 does not fit in LDS: K x 3 launches, which need `scratch` and a coarse map the act kernel can hold
        "gca_helicopter_policy_rollout": [
            ("helicopter_policy: w_local and w_coarse must be 16-B aligned", dict(p_w_coarse=A(70) + 8)),
            ("helicopter_policy: w_local and w_coarse must be 16-B aligned", dict(p_w_coarse=A(70) + 8, K=0)),
            ("helicopter_policy_rollout: this shape runs K x 3 launches and needs `scratch` for the records not kept",
             dict(H=256, W=256, local_out=None)),
            ("helicopter_policy_rollout: this shape runs K x 3 launches and needs `scratch` for the records not kept",
             dict(H=256, W=256, local_out=None, p_block=1)),
            ("helicopter_policy_rollout: coarse map too large", dict(H=256, W=256, p_block=1)),
            ("helicopter_policy_rollout: coarse map too large", dict(H=256, W=256, p_block=1, local_out=None, scratch=A(71)))],
    },
    "host": {
        # one path, so the limit of the coarse map holds whatever K is (the device build returns at K = 0, below)
        "gca_helicopter_policy_rollout": [
            ("helicopter_policy_rollout: coarse map too large", dict(H=256, W=256, p_block=1)),
            ("helicopter_policy_rollout: coarse map too large", dict(H=256, W=256, p_block=1, K=0)),
            ("helicopter_policy_rollout: coarse map too large", dict(H=87, W=87, p_block=1)),   # C = 15138
            ("helicopter_policy: hidden must be a power of two in [32, 256]", dict(H=256, W=256, p_block=1, p_hidden=48))],
        # idx is host memory there: scanned after every shared check, before anything is read through another pointer
        "gca_helicopter_policy_grad": [
            ("helicopter_policy_grad: idx outside [0, T)", dict(idx="idx:3,16,0,1")),
            ("helicopter_policy_grad: idx outside [0, T)", dict(idx="idx:0,1,2,-1")),
            ("helicopter_policy_grad: " + _ALIAS, dict(idx="idx:3,16,0,1", stats="p_b2"))],
    },
}


def _libs():
    from gymca_amd import _lib

    return {"host": _lib.load_cpu(), "device": _lib.load()}


def _call(build, name, over):
    """(status, message) of `name` in `build` on the baseline but for `over`. Keys p_<field> edit the struct behind `p`
    (a policy, or the bulldozer's parameters), a value "p_<weights>" is that weight array's address, "idx:a,b,.." a
    real int32 array."""
    from gymca_amd import _lib

    lib = _libs()[build]
    bulldozer = name in ("gca_move_modify", "gca_bulldozer_reset_where")
    p = _lib.BulldozerParams() if bulldozer else _lib.HeliPolicy()
    if not bulldozer:
        p.radius, p.block, p.hidden = 1, 4, 32
        for i, n in enumerate(_WEIGHTS):
            setattr(p, n, A(80 + i))
    args = dict(_BASE, p=ctypes.byref(p))
    keep = []
    for k, v in over.items():
        if k.startswith("p_"):
            setattr(p, k[2:], v)
    for k, v in over.items():
        if isinstance(v, str) and v.startswith("idx:"):
            keep.append(np.array([int(x) for x in v[4:].split(",")], np.int32))
            v = keep[-1].ctypes.data
        elif isinstance(v, str):
            v = getattr(p, v[2:])
        if not k.startswith("p_"):
            args[k] = v
    status = getattr(lib, name)(*[args.get(n) for n in _ORDER[name]])
    return status, lib.gca_last_error().decode()


def test_the_orders_match_the_bindings():
    from gymca_amd import _lib

    assert set(_ORDER) | {"gca_adam_step_workspace", "gca_adam_step", "gca_permutation", "gca_last_error",
                          "gca_version"} == set(_lib.CPU_SYMBOLS)
    for name, order in _ORDER.items():
        assert len(order) == len(_lib._SIGNATURES[name][0]), name


@pytest.mark.parametrize("name", sorted(_SHARED))
@pytest.mark.parametrize("build", ["host", "device"])
def test_shared_refusals_and_their_messages(build, name):
    head, cases = _SHARED[name]
    for text, over in cases:
        status, msg = _call(build, name, over)
        assert status == 1 and msg == f"argument: {head}{text}", (over, status, msg)


@pytest.mark.parametrize("name", sorted(_SHARED))
def test_both_builds_refuse_alike(name):
    for _, over in _SHARED[name][1]:
        host, device = _call("host", name, over), _call("device", name, over)
        assert host == device and host[0] == 1, (over, host, device)


@pytest.mark.parametrize("build,name", [(b, n) for b in sorted(_OWN) for n in sorted(_OWN[b])])
def test_refusals_of_one_build_alone(build, name):
    for text, over in _OWN[build][name]:
        status, msg = _call(build, name, over)
        assert status == 1 and msg == f"argument: {text}", (over, status, msg)


@pytest.mark.parametrize("build", ["host", "device"])
def test_workspace_query_refusals(build):
    """The query answers -1 and leaves the text; C = 15088 is the largest it takes."""
    from gymca_amd import _lib

    lib = _libs()[build]

    def query(C=8, N=4, null=False, **fields):
        p = _lib.HeliPolicy()
        p.radius, p.block, p.hidden = 1, 4, 32
        for k, v in fields.items():
            setattr(p, k, v)
        return lib.gca_helicopter_policy_grad_workspace(None if null else ctypes.byref(p), C, N)

    for over in (dict(null=True), dict(radius=32), dict(radius=-1), dict(hidden=16), dict(hidden=48), dict(hidden=512),
                 dict(C=0), dict(C=3), dict(C=15090), dict(N=0), dict(N=0, null=True)):
        assert query(**over) == -1 and lib.gca_last_error().decode() == "argument: " + _GRAD_WS, over
    assert query(C=15088) > query(C=15086) > 0


def test_the_largest_coarse_map_runs_on_the_host_and_k_zero_returns_on_the_device():
    """(15088 + 1296) * 4 = 65536 bytes of LDS: gca_helicopter_policy_act takes C = 15088 (the device build's refusal
    above is of the alignment alone) and the host build runs it. And the one call the two builds answer differently on
    purpose: a rollout of K = 0 steps whose coarse map no build could hold returns at once on the device, which
    refuses that map only on its way to a launch."""
    from gymca_amd import _lib

    C, E = 15088, 1
    rng = np.random.default_rng(0)
    w = {"w_local": rng.standard_normal((9, 4, 32)), "w_coarse": rng.standard_normal((C, 32)) * 0.01,
         "b1": rng.standard_normal(32), "w_out": rng.standard_normal((32, 10)), "b2": rng.standard_normal(10)}
    w = {k: np.ascontiguousarray(v, np.float32) for k, v in w.items()}
    p = _lib.HeliPolicy()
    p.radius, p.block, p.hidden = 1, 4, 32
    for k, v in w.items():
        setattr(p, k, v.ctypes.data)
    local = rng.integers(0, 4, (E, 9)).astype(np.uint8)
    coarse = rng.random((E, C)).astype(np.float32)
    rng_step, action, value = np.zeros(E, np.uint32), np.full(E, -1, np.int32), np.full(E, np.nan, np.float32)
    ptr = lambda a: a.ctypes.data
    status = _libs()["host"].gca_helicopter_policy_act(ctypes.byref(p), C, ptr(local), ptr(coarse), ptr(rng_step), 0, 5,
                                                       1, ptr(action), None, ptr(value), E, None)
    assert status == 0 and 0 <= action[0] <= 8 and np.isfinite(value[0])
    assert _call("device", "gca_helicopter_policy_rollout", dict(H=256, W=256, p_block=1, K=0))[0] == 0
