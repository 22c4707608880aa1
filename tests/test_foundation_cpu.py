"""CPU: the references of tests/_foundation_ref.py, the conditions of the cases they share with
tests/test_gpu_foundation.py, and the host build (libgca_cpu.so) of gca_ds_count_draws / gca_ds_step, gca_count_cells,
gca_philox and gca_move_modify on those cases. Every comparison is exact. No GPU."""
import numpy as np
import pytest

import _foundation_ref as ref


# ------------------------------------------------------------------ the references themselves
def test_fill_reference_equals_the_reset_restatement():
    """For three values the definition is _bulldozer_reset_ref.fill_grid with episode 0."""
    import _bulldozer_reset_ref as rr

    cdf = rr.cdf_of(0.25, 0.5)
    for seed in ref.SEEDS:
        got = ref.fill_categorical(seed, 9, 3, 7 * 11, cdf, rr.CODES)
        for e in range(3):
            assert np.array_equal(got[e].reshape(7, 11), rr.fill_grid(seed, 9 + e, 0, 7, 11, cdf))


def test_fill_and_action_case_conditions():
    ref.check_fill_conditions()
    ref.check_action_conditions()
    assert ref.fill_cdf(3).dtype == np.float32 and ref.fill_cdf(5)[-1] == np.float32(0.6)
    s = ref.action_rng_step(257)
    assert 0 in s and 0xFFFFFFFF in s


def test_random_actions_reference_by_hand():
    """One env spelled out word by word: move = (x.x * 9) >> 32, shoot = the top bit of x.y."""
    from oracle import philox

    seed, off, step = ref.SEEDS[1], 1000, 0xFFFFFFFF
    x = philox.philox4x32_10(np.array([0, off, step, ref.TAG_ACTION]), np.array([seed & 0xFFFFFFFF, seed >> 32]))
    exp = [(int(x[0]) * 9) >> 32, int(x[1]) >> 31]
    assert ref.random_actions(seed, off, 1, [step]).tolist() == [exp]


def test_reset_reference_bit_convention():
    """Cell i of the flat batch is bit i & 15 of word i >> 4: with two envs of 32 cells, env 1 owns words 2 and 3."""
    s = ref.reset_state(2, 2, 16)
    out = ref.reset_where(np.array([0, 1], np.uint8), s, use_dousing0=False)
    assert np.array_equal(out["dous_bits"][:2], s["dous_bits"][:2]) and not out["dous_bits"][2:].any()
    assert s["dous_bits"][:2].all() and np.array_equal(out["grid"][1], s["grid0"][1])
    assert np.array_equal(out["age"][0], s["age"][0]) and not out["dousing"][1].any() and out["accu"][1] == 0
    kept = ref.reset_where(np.array([0, 1], np.uint8), s, skip=ref.RESET_GROUPS)
    assert all(np.array_equal(kept[k], s[k]) for k in s)


# ------------------------------------------------------------------ gca_philox, gca_count_cells (host build)
def test_host_philox_matches_the_oracle():
    from gymca_amd import _lib

    for ctr, key, kat in ref.philox_cases():
        out = np.full_like(ctr, 0xA5A5A5A5)
        _lib.call_cpu("gca_philox", ctr.ctypes.data, key[0], key[1], out.ctypes.data, len(ctr), None)
        assert np.array_equal(out, ref.philox_expected(ctr, key))
        if kat is not None:
            assert np.array_equal(out[0], kat) and np.array_equal(out[-1], kat)


@pytest.mark.parametrize("name", list(ref.COUNT_CASES))
def test_host_count_cells_matches_numpy(name):
    from gymca_amd import _lib

    ref.check_count_conditions(name)
    g = ref.count_grid(name)
    E, H, W = g.shape
    for shift in (ref.COUNT_SHIFTS if name == "shifted" else (0,)):
        buf = np.zeros(g.size + 16, np.uint8)
        view = buf[shift:shift + g.size]
        view[:] = g.reshape(-1)
        for triple in ref.COUNT_TRIPLES:
            counts = np.full((E, 3), -12345, np.int32)  # the call overwrites
            _lib.call_cpu("gca_count_cells", view.ctypes.data, E, H, W, *triple, counts.ctypes.data, None)
            assert np.array_equal(counts, ref.count_expected(g, triple)), (name, shift, triple)


# ------------------------------------------------------------------ Drossel-Schwabl (host build)
def _host_ds(c, uniforms, offsets, seed=0, rng_step=None, env_offset=0):
    from gymca_amd import _lib

    grids = np.ascontiguousarray(c.grids)
    thr = np.ascontiguousarray(c.thresholds)
    out = np.full_like(grids, 99)
    counts = np.full((c.E, 3), -12345, np.int32)
    _lib.call_cpu("gca_ds_step", grids.ctypes.data, out.ctypes.data, c.E, c.H, c.W, *c.codes, thr.ctypes.data,
                  None if uniforms is None else uniforms.ctypes.data, None if offsets is None else offsets.ctypes.data,
                  seed, None if rng_step is None else rng_step.ctypes.data, env_offset, counts.ctypes.data, None)
    return out, counts


@pytest.mark.parametrize("name", list(ref.DS_CASES))
def test_host_drossel_exact_stream_matches_the_oracle(name):
    from gymca_amd import _lib

    c = ref.ds_case(name)
    ref.check_ds_conditions(c)
    grids = np.ascontiguousarray(c.grids)
    n = np.full(c.E, -1, np.int32)
    _lib.call_cpu("gca_ds_count_draws", grids.ctypes.data, c.E, c.H, c.W, *c.codes, n.ctypes.data, None)
    assert np.array_equal(n, c.n_draws)
    offsets = (ref.DS_FIRST_OFFSET + np.cumsum(n) - n).astype(np.int64)  # exclusive sum of the build's own counts
    out, counts = _host_ds(c, np.ascontiguousarray(c.uniforms), offsets)
    assert np.array_equal(out, c.out) and np.array_equal(counts, c.counts)


def test_host_drossel_philox_mode_matches_the_oracle():
    c = ref.ds_philox_case()
    d = ref.DS_PHILOX
    out, counts = _host_ds(c, None, None, d["seed"], c.rng_step, d["env_offset"])
    assert np.array_equal(out, c.out) and np.array_equal(counts, c.counts)


def test_host_drossel_dropin_matches_the_oracle_at_40x256():
    """Ten chunks of 256 cells through the Python drop-in on the host build, seeded like the oracle's generator."""
    from gymca_amd.forest_fire.operators import ForestFire
    from oracle import drossel

    grid = np.random.default_rng(5).choice(3, size=(40, 256), p=[0.3, 0.6, 0.1]).astype(np.int64)
    op, twin = ForestFire(0, 1, 2, backend="cpu"), ForestFire(0, 1, 2, backend="cpu")
    op.seed(1234)
    twin.seed(1234)
    out, _ = op.update(grid, None, (0.033, 0.333))
    assert np.array_equal(out, drossel.ds_step(grid, 0.033, 0.333, twin.np_random))


# ------------------------------------------------------------------ gca_move_modify (host build)
@pytest.mark.parametrize("table", range(len(ref.MOVE_TABLES)))
def test_host_move_modify_matches_the_oracle_move(table):
    """The host build, which the device test compares against, equals oracle.windy.move and the effect table."""
    from oracle.windy import move

    effects, pos, action, grid = ref.move_case(table)
    npos, ngrid, hit = ref.host_move_modify(effects, pos, action, grid)
    exp_grid, exp_hit = grid.copy(), np.zeros(len(pos), np.uint8)
    for e in range(len(pos)):
        r, c = move(pos[e], int(action[e, 0]), ref.MOVE_H, ref.MOVE_W)
        assert (npos[e, 0], npos[e, 1]) == (r, c)
        if action[e, 1] and int(grid[e, r, c]) in effects:
            exp_grid[e, r, c] = effects[int(grid[e, r, c])]
            exp_hit[e] = 1
    assert np.array_equal(ngrid, exp_grid) and np.array_equal(hit, exp_hit)
    assert (npos != pos).any() and 0 < hit.sum() < len(hit) and set(action[:, 0]) == set(range(9))
