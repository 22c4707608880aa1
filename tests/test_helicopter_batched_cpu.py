"""CPU: the batched ForestFireHelicopter env step (gca_helicopter_step) in the host build of the C-ABI against its
numpy restatement (tests/_helicopter_ref.py), the oracle's Drossel-Schwabl rule, the host gca_ds_step and the
reference's seeded 5x5 episode (tests/golden/helicopter.npz). No GPU."""
import numpy as np
import pytest

import _helicopter_ref as ref
from oracle import drossel

SEED = 0x1234ABCD5678


def _grids(E, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 3, (E, H, W)).astype(np.uint8)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 5), (3, 67)])
@pytest.mark.parametrize("p", [0.0, 1.0])
def test_restated_rule_is_the_oracles(shape, p):
    """Thresholds 0 (no draw succeeds) and 1 (every draw succeeds) make the step deterministic: the restatement's CA
    equals oracle.drossel.ds_step whatever the rng."""
    assert drossel.choice_threshold(p) == p
    for k in range(4):
        g = _grids(1, *shape, seed=k)[0]
        want = drossel.ds_step(g, p, p, np.random.default_rng(k))
        got = ref.ca_step(g, p, p, SEED, 3, k)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("max_freeze", [0, 2])
def test_host_build_equals_the_restatement(max_freeze):
    E, H, W, off = 3, 6, 9, 5
    thr = np.array([[0.05, 0.4], [0.3, 0.3], [0.033, 0.333]])
    a = ref.make_state(_grids(E, H, W, 1), thr, max_freeze, rng_step=[0, 7, 0xFFFFFFFF])
    b = ref.copy_state(a)
    rng = np.random.default_rng(2)
    ca_steps = 0
    for s in range(12):
        act = rng.integers(-1, 10, E).astype(np.int32)  # -1 and 9 exercise the clamp
        ca_steps += int((a["freeze"] == 0).sum())
        out = np.full(E, -7, np.int32)
        ref.ref_step(a, act, max_freeze, SEED, off)
        ref.host_step(b, act, max_freeze, SEED, off, action_out=out)
        assert np.array_equal(out, act)
        ref.assert_states_equal(a, b, f"step {s}")
    assert ca_steps == (36 if max_freeze == 0 else 12)
    assert (a["steps_elapsed"] == 12).all()


def test_host_random_policy_equals_the_restatement():
    E, H, W, off = 3, 4, 5, 5
    a = ref.make_state(_grids(E, H, W, 3), [0.1, 0.5], 1)
    b = ref.copy_state(a)
    seen = set()
    for s in range(12):
        out = np.zeros(E, np.int32)
        taken = ref.ref_step(a, None, 1, SEED, off, action_seed=9)
        ref.host_step(b, None, 1, SEED, off, action_seed=9, action_out=out)
        assert np.array_equal(out, taken) and ((0 <= out) & (out < 9)).all()
        seen.update(out.tolist())
        ref.assert_states_equal(a, b, f"step {s}")
    assert len(seen) > 3


def test_host_ca_equals_host_ds_step():
    """The env step's CA pass is gca_ds_step in Philox mode on the same grid, rng_step and env_offset."""
    from gymca_amd import _lib

    E, H, W, off = 3, 7, 11, 5
    g = _grids(E, H, W, 4)
    thr = np.array([[0.05, 0.4], [0.3, 0.3], [0.033, 0.333]])
    s = ref.make_state(g, thr, 0, pos=[[0, 0]] * E, rng_step=[3, 4, 5])
    s["buf"][0][:, 0, 0] = 0  # Modify's cell cannot turn FIRE (EMPTY -> EMPTY / TREE): the pass shows unmodified
    gin = s["buf"][0].copy()
    steps = s["rng_step"].copy()
    out, counts = np.zeros_like(gin), np.zeros((E, 3), np.int32)
    _lib.call_cpu("gca_ds_step", gin.ctypes.data, out.ctypes.data, E, H, W, 0, 1, 2, s["thresholds"].ctypes.data, None,
                  None, SEED, steps.ctypes.data, off, counts.ctypes.data, None)
    ref.host_step(s, np.full(E, 4, np.int32), 0, SEED, off)
    assert not s["hit"].any() and (s["parity"] == 1).all()
    assert np.array_equal(s["buf"][1], out) and np.array_equal(s["counts"], counts)


def test_reference_episode_replay(golden):
    """Every step of the reference's seeded 5x5 episode, from the reference's own state before it. Steps whose freeze
    is 0 before the step run the CA, on another random stream here: they are compared on position, freeze and the
    reward of their own grid; the others on grid, reward (bit-equal), position, freeze and hit."""
    from gymca_amd.forest_fire.operators.ca_DrosselSchwabl import choice_threshold

    d = golden("helicopter")
    grids, recs = d["grids"], d["recs"]
    H, W = grids.shape[1:]
    max_freeze = int(0.5 * ((H + W) // 2))
    thr = [choice_threshold(0.033), choice_threshold(0.333)]
    n_ca = 0
    for s in range(len(grids)):
        g0 = d["grid0"] if s == 0 else grids[s - 1]
        pos = (H // 2, W // 2) if s == 0 else (int(recs[s - 1][1]), int(recs[s - 1][2]))
        fz = max_freeze if s == 0 else int(recs[s - 1][3])
        st = ref.make_state(np.asarray(g0)[None], thr, max_freeze, pos=[pos], freeze=fz, rng_step=s)
        ref.host_step(st, np.array([s % 9], np.int32), max_freeze, SEED, 0)
        exp = recs[s]
        got = ref.current_grids(st)[0]
        assert (int(st["pos"][0, 0]), int(st["pos"][0, 1]), int(st["freeze"][0])) == \
            (int(exp[1]), int(exp[2]), int(exp[3])), f"step {s}"
        if fz == 0:
            n_ca += 1
            assert s % 3 == 2
            c = np.array([(got == v).sum() for v in (0, 1, 2)])
            assert np.array_equal(c, st["counts"][0])
            own = np.dot(np.array([0.0, 1.0, -1.0]), c / (H * W))
            assert np.float64(own).view(np.uint64) == st["reward"].view(np.uint64)[0], f"step {s}"
        else:
            assert np.array_equal(got, grids[s]), f"step {s}"
            assert np.float64(exp[0]).view(np.uint64) == st["reward"].view(np.uint64)[0], f"step {s}"
            assert int(st["hit"][0]) == int(exp[4]), f"step {s}"
    assert n_ca <= 16 and len(grids) - n_ca >= 32


def test_host_step_refuses_bad_arguments():
    from gymca_amd import GCAError

    s = ref.make_state(_grids(1, 3, 3), [0.1, 0.1], 1)
    with pytest.raises(GCAError, match="max_freeze"):
        ref.host_step(s, np.zeros(1, np.int32), -1, SEED, 0)
