"""The C-ABI library loads and exports every symbol include/gca.h declares; ctypes
struct layouts equal the C compiler's. No compute calls (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "gca.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gca_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from gymca_amd import _lib

    lib = _lib.load()
    names = declared_functions()
    assert len(names) >= 20
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert set(names) == set(_lib.EXPORTED_SYMBOLS), set(names) ^ set(_lib.EXPORTED_SYMBOLS)


def declared_arities():
    """{function: number of parameters} from the prototypes in include/gca.h."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(gca_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src):
        params = m.group(2).strip()
        out[m.group(1)] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_ctypes_signatures_match_the_header_arity():
    """Every ctypes signature passes as many arguments as the header's prototype takes (a stale table shifts every
    argument after the difference)."""
    from gymca_amd import _lib

    ar = declared_arities()
    assert len(ar) >= 20
    bad = {n: (len(_lib._SIGNATURES[n][0]), k) for n, k in ar.items() if len(_lib._SIGNATURES[n][0]) != k}
    assert not bad, bad


def test_version_and_error_calls_need_no_gpu():
    from gymca_amd import _lib

    lib = _lib.load()
    assert lib.gca_version() == 1
    assert isinstance(lib.gca_last_error(), bytes)


def test_argument_errors_are_reported_without_touching_the_gpu():
    from gymca_amd import _lib

    with pytest.raises(_lib.GCAError, match="E, H, W must be positive"):
        _lib.call("gca_windy_step", 1, 1, None, None, 0, 1, 0, 4, 4, 0, 3, 25, 0, None, None)
    with pytest.raises(_lib.GCAError, match="burn radius"):
        p = _lib.AlexParams()
        p.R = 0
        _lib.call("gca_alex_step", p, 1, 4, 4, *([1] * 9), None, None, None, None, None, None, None)


C_LAYOUT = r"""
#include <stdio.h>
#include <stddef.h>
#include "gca.h"
#define P(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f));
int main(void) {
  printf("gca_bulldozer_params %zu\n", sizeof(gca_bulldozer_params));
  P(gca_bulldozer_params, t_shoot) P(gca_bulldozer_params, seed) P(gca_bulldozer_params, right_mask)
  P(gca_bulldozer_params, effect)
  printf("gca_alex_params %zu\n", sizeof(gca_alex_params));
  P(gca_alex_params, heat_dw) P(gca_alex_params, p_tree) P(gca_alex_params, seed) P(gca_alex_params, n_winds)
  P(gca_alex_params, winds)
  printf("gca_advenv_params %zu\n", sizeof(gca_advenv_params));
  P(gca_advenv_params, day_length) P(gca_advenv_params, seed) P(gca_advenv_params, right_mask)
  printf("gca_obs_params %zu\n", sizeof(gca_obs_params));
  P(gca_obs_params, ext_skip_blur) P(gca_obs_params, day_length) P(gca_obs_params, color_night)
  P(gca_obs_params, tint_night) P(gca_obs_params, ext_lookup)
  printf("gca_pine_params %zu\n", sizeof(gca_pine_params));
  P(gca_pine_params, max_pinecones) P(gca_pine_params, dy) P(gca_pine_params, scale) P(gca_pine_params, den1p)
  P(gca_pine_params, seed) P(gca_pine_params, fire)
  printf("gca_pine_classic_params %zu\n", sizeof(gca_pine_classic_params));
  P(gca_pine_classic_params, dx) P(gca_pine_classic_params, burn_thr) P(gca_pine_classic_params, age_hi)
  P(gca_pine_classic_params, seed) P(gca_pine_classic_params, fire)
  return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    from gymca_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text(C_LAYOUT)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.rsplit(" ", 1) for line in out if line)
    py = {"gca_bulldozer_params": _lib.BulldozerParams, "gca_alex_params": _lib.AlexParams,
          "gca_advenv_params": _lib.AdvEnvParams, "gca_obs_params": _lib.ObsParams,
          "gca_pine_params": _lib.PineParams, "gca_pine_classic_params": _lib.PineClassicParams}
    for key, val in got.items():
        if "." in key:
            t, f = key.split(".")
            assert getattr(py[t], f).offset == int(val), key
        else:
            assert ctypes.sizeof(py[key]) == int(val), key


def test_bound_call_converts_once_and_checks_arity():
    """_lib.BoundCall (the batched envs' pre-bound step call): every argument converted to its declared ctypes type
    at bind time, structs by reference, SLOT positions rebound per call; wrong arities refused before any call."""
    from gymca_amd import _lib

    p = _lib.BulldozerParams()
    args = [p, _lib.SLOT] + [0x1000 + 16 * i for i in range(4)] + [9] + [0x2000 + 16 * i for i in range(4)] + \
        [256, 256] + [0x3000 + 16 * i for i in range(6)] + [1024, _lib.SLOT]
    bc = _lib.BoundCall("gca_bulldozer_step_fused", *args)
    assert len(bc._slots) == 2 and len(bc._args) == len(args)
    assert isinstance(bc._args[6], ctypes.c_int64) and bc._args[6].value == 9
    assert isinstance(bc._args[2], ctypes.c_void_p) and bc._args[2].value == 0x1000
    p.t_any = 0.25  # bound by reference: the call sees later edits of the struct
    assert ctypes.cast(bc._args[0], ctypes.POINTER(_lib.BulldozerParams)).contents.t_any == 0.25
    with pytest.raises(TypeError):
        _lib.BoundCall("gca_bulldozer_step_fused", *args[:-1])
    with pytest.raises(TypeError):
        _lib.BoundCall("gca_bulldozer_step_fused", _lib.SLOT, *args[1:])
    with pytest.raises(TypeError):
        bc(0x4000)  # two per-call values expected


# The fused bulldozer entry points' arguments by name, in each prototype's order (include/gca.h). Every call below is
# refused by an argument check (or returns at K = 0) before any launch, so the pointers are never dereferenced.
_STATE = ("accu", "steps", "done", "wind", "wind_stride", "rng_step", "parity", "buf0", "buf1", "H", "W", "pos", "counts",
          "hit", "reward", "steps_elapsed")
_FUSED_ORDER = {
    "gca_bulldozer_step_fused": ("p", "action") + _STATE + ("meet", "E", "stream"),
    "gca_bulldozer_step_fused_random": ("p", "action_seed", "action_out") + _STATE + ("meet", "E", "stream"),
    "gca_bulldozer_rollout_random": ("p", "action_seed", "K", "action_out", "reward_out", "done_out") + _STATE +
                                    ("E", "stream"),
    "gca_bulldozer_rollout": ("p", "actions", "action_seed", "K", "action_out", "reward_out", "done_out", "truncated_out",
                              "autoreset", "reset_seed", "max_steps", "cdf", "values", "episode", "last_length",
                              "terminated", "truncated") + _STATE + ("E", "stream"),
}
_WHO = {"gca_bulldozer_step_fused": "bulldozer_step_fused", "gca_bulldozer_step_fused_random": "bulldozer_step_fused",
        "gca_bulldozer_rollout_random": "bulldozer_rollout_random", "gca_bulldozer_rollout": "bulldozer_rollout"}
_ROLLOUTS = ("gca_bulldozer_rollout_random", "gca_bulldozer_rollout")
_T_STEP = ("an action can take >= 1 time unit (several CA passes per step): use gca_bulldozer_pre / gca_windy_step / "
           "gca_bulldozer_post")
_T_ROLL = "an action can take >= 1 time unit (several CA passes per step)"


def _fused_call(name, **over):
    """(status, message) of one fused bulldozer entry point with valid arguments but for `over` (p_* edits the params)."""
    from gymca_amd import _lib
    from gymca_amd.forest_fire.operators.move_modify import make_params

    p = make_params(None, {3: 0})
    p.empty, p.tree, p.fire, p.t_any = 0, 3, 25, 0.001
    for a in range(9):
        p.t_move[a] = 0.4
    p.t_shoot[1] = 0.3
    args = {n: 0x10000 + 0x100 * i for i, n in enumerate(
        ("action", "action_out", "actions", "reward_out", "done_out", "truncated_out", "cdf", "values", "episode",
         "last_length", "terminated", "truncated", "accu", "steps", "done", "wind", "rng_step", "parity", "buf0", "buf1",
         "pos", "counts", "hit", "reward", "steps_elapsed", "meet"))}
    args.update(p=p, action_seed=9, K=3, autoreset=0, reset_seed=5, max_steps=0, wind_stride=9, H=8, W=256, E=2,
                stream=None)
    for k, v in over.items():
        if k.startswith("p_"):
            setattr(p, k[2:], v)
        else:
            args[k] = v
    lib = _lib.load()
    status = getattr(lib, name)(*[args[n] for n in _FUSED_ORDER[name]])
    return status, lib.gca_last_error().decode()


@pytest.mark.parametrize("name", sorted(_FUSED_ORDER))
def test_fused_bulldozer_argument_messages(name):
    """Every argument check of gca_bulldozer_step_fused(_random), gca_bulldozer_rollout_random and gca_bulldozer_rollout:
    the exact text a caller receives, per entry point, and which check fires first when several fail."""
    who, roll = _WHO[name], name in _ROLLOUTS
    null = "null argument, empty batch or K < 0" if roll else "null argument or empty batch"

    def refused(text, **over):
        status, msg = _fused_call(name, **over)
        assert status == 1 and msg == f"argument: {who}: {text}", (over, status, msg)

    for over in (dict(done=None), dict(p=None), dict(reward=None), dict(buf1=None), dict(E=0), dict(H=0),
                 dict(done=None, W=128), dict(E=-1, buf0=0x10008)):
        refused(null, **over)
    refused("W must be 256 or 512 (the row-stream CA)", W=128)
    refused("W must be 256 or 512 (the row-stream CA)", W=1024, buf0=0x10008, wind_stride=-1)
    codes = "cell codes must be empty = 0 < tree < fire < 256 (the closed-form rule)"
    for over in (dict(p_empty=1), dict(p_tree=25), dict(p_tree=30), dict(p_fire=256), dict(p_tree=0),
                 dict(p_fire=256, buf1=0x10008)):
        refused(codes, **over)
    refused("buffers 16-B aligned", buf0=0x10008)
    refused("buffers 16-B aligned", buf1=0x10004, wind_stride=-1)
    refused("wind_stride >= 0", wind_stride=-1)
    refused("wind_stride >= 0", wind_stride=-9, p_t_any=1.0)
    refused(_T_ROLL if roll else _T_STEP, p_t_any=0.3)  # 0.4 + 0.3 + 0.3 >= 1
    if roll:
        refused(null, K=-1)
        refused("K x E too large", K=2**31 - 1, E=2**10)
        refused("K x E too large", K=2**31 - 1, E=2**10, p_t_any=0.3)
        assert _fused_call(name, K=0)[0] == 0  # nothing to do: no launch
    if name == "gca_bulldozer_step_fused":
        refused("action required", action=None)
        refused("action required", action=None, done=None, W=128)
    if not roll:
        refused("too many envs", E=2**29)  # with the meeting slots: 4 workgroups per env at the most
    if name == "gca_bulldozer_rollout":
        # the reset's own checks follow the shared ones, whether or not the call resets
        refused("buf0 and buf1 must differ", buf1=0x10000 + 0x100 * 18)
        refused(_T_ROLL, buf1=0x10000 + 0x100 * 18, p_t_any=0.3)
        refused("H < 32768", H=32768)
        refused("max_steps >= 0", max_steps=-1)
        refused("max_steps >= 0", max_steps=-1, autoreset=1, cdf=None)
        need = "null argument (autoreset needs cdf, values, episode and steps_elapsed)"
        for over in (dict(cdf=None), dict(values=None), dict(episode=None), dict(steps_elapsed=None)):
            refused(need, autoreset=1, **over)
            assert _fused_call(name, K=0, **over)[0] == 0  # only read under autoreset
        refused("env_offset >= 0", autoreset=1, p_env_offset=-1)
        assert _fused_call(name, K=0, autoreset=1)[0] == 0
