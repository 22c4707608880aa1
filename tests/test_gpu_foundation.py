"""GPU: the entry points every env is built on -- gca_ds_count_draws / gca_ds_step, gca_count_cells,
gca_fill_categorical, gca_random_actions, gca_philox, gca_reset_where, gca_move_modify -- as raw C-ABI calls on device
tensors against the restatements of tests/_foundation_ref.py (built on oracle.philox and oracle.drossel), at the
shapes where their scans, chunk loops, tails and vector / scalar paths change. Every comparison is exact."""
import numpy as np
import pytest

import _foundation_ref as ref

pytestmark = pytest.mark.gpu

_SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}


def _dev(a, device):
    """A contiguous device copy of a numpy array (unsigned 16 / 32-bit words travel as their signed views)."""
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype)).copy()).to(device)


def _host(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def _call(name, *args):
    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    call(name, *args, dev.stream_ptr())


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------ 1. Drossel-Schwabl
def _device_ds(c, device, uniforms, offsets, seed=0, rng_step=None, env_offset=0):
    import torch

    grids = _dev(c.grids, device)
    out = torch.full_like(grids, 99)
    counts = torch.full((c.E, 3), -12345, dtype=torch.int32, device=device)  # the call overwrites
    thr = _dev(c.thresholds, device)
    _call("gca_ds_step", _ptr(grids), _ptr(out), c.E, c.H, c.W, *c.codes, _ptr(thr), _ptr(uniforms), _ptr(offsets),
          seed, _ptr(rng_step), env_offset, _ptr(counts))
    return _host(out), _host(counts)


@pytest.mark.parametrize("name", list(ref.DS_CASES))
def test_drossel_exact_stream_matches_the_oracle(name, device):
    """The scan across waves and chunks: env e's j-th drawing cell, row-major, reads uniforms[uniform_offset[e] + j] of
    one shared array, the offsets being the exclusive sum of the device's own draw counts."""
    import torch

    c = ref.ds_case(name)
    ref.check_ds_conditions(c)
    grids = _dev(c.grids, device)
    n = torch.full((c.E,), -1, dtype=torch.int32, device=device)
    _call("gca_ds_count_draws", _ptr(grids), c.E, c.H, c.W, *c.codes, _ptr(n))
    n = _host(n)
    assert np.array_equal(n, c.n_draws)
    offsets = (ref.DS_FIRST_OFFSET + np.cumsum(n) - n).astype(np.int64)
    out, counts = _device_ds(c, device, _dev(c.uniforms, device), _dev(offsets, device))
    assert np.array_equal(out, c.out)
    assert np.array_equal(counts, c.counts)


def test_drossel_philox_mode_matches_the_oracle(device):
    c = ref.ds_philox_case()
    d = ref.DS_PHILOX
    out, counts = _device_ds(c, device, None, None, d["seed"], _dev(c.rng_step, device), d["env_offset"])
    assert np.array_equal(out, c.out)
    assert np.array_equal(counts, c.counts)


def test_drossel_dropin_matches_the_oracle_at_40x256(device):
    """Ten chunks of 256 cells through the Python drop-in, seeded like the oracle's generator."""
    from gymca_amd.forest_fire.operators import ForestFire
    from oracle import drossel

    grid = np.random.default_rng(5).choice(3, size=(40, 256), p=[0.3, 0.6, 0.1]).astype(np.int64)
    op, twin = ForestFire(0, 1, 2, backend="hip"), ForestFire(0, 1, 2, backend="hip")
    op.seed(1234)
    twin.seed(1234)
    out, _ = op.update(grid, None, (0.033, 0.333))
    assert np.array_equal(out, drossel.ds_step(grid, 0.033, 0.333, twin.np_random))


# ------------------------------------------------------------------ 2. gca_count_cells
@pytest.mark.parametrize("name", list(ref.COUNT_CASES))
def test_count_cells_matches_numpy(name, device):
    import torch

    ref.check_count_conditions(name)
    g = ref.count_grid(name)
    E, H, W = g.shape
    for shift in (ref.COUNT_SHIFTS if name == "shifted" else (0,)):
        buf = torch.zeros(g.size + 16, dtype=torch.uint8, device=device)
        assert buf.data_ptr() % 16 == 0
        view = buf[shift:shift + g.size]
        view.copy_(_dev(g.reshape(-1), device))
        for triple in ref.COUNT_TRIPLES:
            counts = torch.full((E, 3), -12345, dtype=torch.int32, device=device)  # the call overwrites
            _call("gca_count_cells", view.data_ptr(), E, H, W, *triple, _ptr(counts))
            assert np.array_equal(_host(counts), ref.count_expected(g, triple)), (name, shift, triple)


# ------------------------------------------------------------------ 3. gca_fill_categorical
@pytest.mark.parametrize("case", range(len(ref.FILL_CASES)))
def test_fill_categorical_matches_the_definition(case, device):
    import torch

    ref.check_fill_conditions()
    n, E, off = ref.FILL_CASES[case]
    for nv in ref.FILL_N_VALUES:
        cdf = _dev(ref.fill_cdf(nv), device)
        values = _dev(np.array(ref.FILL_VALUES[:nv], np.uint8), device)
        for seed in ref.SEEDS:
            out = torch.full((E * n + 1,), 0xA5, dtype=torch.uint8, device=device)  # one guard byte behind the batch
            _call("gca_fill_categorical", _ptr(out), n, E, off, seed, _ptr(cdf), _ptr(values), nv)
            got = _host(out)
            assert got[-1] == 0xA5, (nv, seed)
            assert np.array_equal(got[:-1].reshape(E, n), ref.fill_expected(case, nv, seed)), (nv, seed)


# ------------------------------------------------------------------ 4. gca_random_actions
def test_random_actions_match_the_definition(device):
    import torch

    ref.check_action_conditions()
    for E, off, with_step, seed in ref.ACTION_CASES:
        step = _dev(ref.action_rng_step(E), device) if with_step else None
        act = torch.full((E + 1, 2), -7, dtype=torch.int32, device=device)  # a guard row behind the batch
        _call("gca_random_actions", _ptr(act), E, off, seed, _ptr(step))
        got = _host(act)
        assert got[-1].tolist() == [-7, -7]
        assert np.array_equal(got[:-1], ref.action_expected(E, off, with_step, seed)), (E, off, with_step, seed)


# ------------------------------------------------------------------ 5. gca_philox
def test_philox_many_counters_per_launch(device):
    import torch

    for ctr, key, kat in ref.philox_cases():
        out = torch.full((len(ctr) + 1, 4), -1, dtype=torch.int32, device=device)  # a guard row behind the batch
        _call("gca_philox", _ptr(_dev(ctr, device)), key[0], key[1], _ptr(out), len(ctr))
        got = _host(out, np.uint32)
        assert (got[-1] == 0xFFFFFFFF).all()
        assert np.array_equal(got[:-1], ref.philox_expected(ctr, key))
        if kat is not None:
            assert np.array_equal(got[0], kat) and np.array_equal(got[-2], kat)


# ------------------------------------------------------------------ 6. gca_reset_where
def _device_reset(done, s, device, use_dousing0, skip):
    """One call on device copies of the state; returns the state afterwards, plus "done"."""
    E, H, W = s["grid"].shape
    t = {k: _dev(v, device) for k, v in s.items()}
    t["done"] = _dev(done, device)

    def arg(name, group=None):
        return None if (group or name) in skip or name not in t else _ptr(t[name])

    _call("gca_reset_where", _ptr(t["done"]), E, H, W, arg("grid"), arg("grid0", "grid"), arg("age"),
          arg("age0", "age"), arg("dousing"), arg("dousing0", "dousing") if use_dousing0 else None, arg("dous_bits"),
          arg("pos"), arg("pos0", "pos"), arg("accu"), arg("wind_index"), arg("wind_index0", "wind_index"))
    return {k: _host(v, s[k].dtype if k in s else None) for k, v in t.items()}


def _assert_state(got, exp, where):
    for k, v in exp.items():
        assert got[k].dtype == v.dtype, (where, k)
        assert np.array_equal(got[k].view(np.uint8), v.view(np.uint8)), (where, k)  # bit patterns, floats included


@pytest.mark.parametrize("shape", ref.RESET_SHAPES)
def test_reset_where_matches_numpy_where(shape, device):
    """Every array, none / all / mixed done: reset envs take their initial state (dousing0, or zeros with the packed
    bits cleared), live envs keep every byte, done is cleared."""
    E, H, W = shape
    s = ref.reset_state(E, H, W)
    assert ("dous_bits" in s) == (shape == ref.RESET_SHAPES[0])
    for pattern in ("none", "all", "mixed"):
        done = ref.reset_done(E, pattern)
        for use0, skip in ((True, ("dous_bits",)), (False, ())):  # the bits go with the zeroed dousing only
            got = _device_reset(done, s, device, use0, skip)
            _assert_state(got, ref.reset_where(done, s, use0, skip), (pattern, use0))
    done = ref.reset_done(E, "mixed")
    for group in ref.RESET_GROUPS:  # each nullable group passed as NULL once
        got = _device_reset(done, s, device, False, (group,))
        _assert_state(got, ref.reset_where(done, s, False, (group,)), ("null", group))


# ------------------------------------------------------------------ 7. gca_move_modify
@pytest.mark.parametrize("table", range(len(ref.MOVE_TABLES)))
def test_move_modify_more_envs_than_a_workgroup(table, device):
    """E = 300 against the host build's gca_move_modify on the same arrays (held to oracle.windy.move on the CPU)."""
    import torch

    from gymca_amd.forest_fire.operators.move_modify import make_params

    effects, pos, action, grid = ref.move_case(table)
    exp_pos, exp_grid, exp_hit = ref.host_move_modify(effects, pos, action, grid)
    E, H, W = grid.shape
    p = make_params(ref.MOVE_SETS, effects)
    d_pos, d_grid, d_act = _dev(pos, device), _dev(grid, device), _dev(action, device)
    hit = torch.full((E + 1,), 7, dtype=torch.uint8, device=device)
    _call("gca_move_modify", p, _ptr(d_act), _ptr(d_pos), _ptr(d_grid), H, W, _ptr(hit), E)
    assert np.array_equal(_host(d_pos), exp_pos)
    assert np.array_equal(_host(d_grid), exp_grid)
    assert np.array_equal(_host(hit)[:-1], exp_hit) and _host(hit)[-1] == 7
