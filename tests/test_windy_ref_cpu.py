"""CPU: the references of tests/_windy_ref.py hold before the device is held to them. ref_windy_step against every case
of the committed golden windy.npz (empty != 0 included); the vectorised Philox rolls and masks against
oracle.windy.philox_roll / dir_mask; ref_pre / ref_interpass / ref_post chained over several env steps against
oracle.windy.BulldozerOracle; and the reach conditions every case builder asserts (the march's strip heights, gated
envs, both parities, masked-off neighbours, 3-pass envs)."""
import numpy as np
import pytest

import _windy_ref as wr
from oracle import windy as owindy


def test_ref_windy_step_matches_every_golden_case(golden):
    d = golden("windy")
    n, nonzero_empty = int(d["n"]), 0
    for i in range(n):
        codes = tuple(int(v) for v in d[f"c{i}_values"])
        grid, want = d[f"c{i}_grid"], d[f"c{i}_out"]
        m = owindy.dir_mask(d[f"c{i}_wind"], d[f"c{i}_roll"])
        junk = np.full_like(grid, 0xEE)
        for par in (0, 1):  # the source in either buffer
            bufs = [junk[None], grid[None]] if par else [grid[None], junk[None]]
            c0 = np.array([[5, 6, 7]], np.int32)
            b0, b1, cnt = wr.ref_windy_step(bufs[0], bufs[1], np.array([par], np.uint8), None, 0, [m], codes, c0)
            got, src = (b0, b1) if par else (b1, b0)
            assert np.array_equal(got[0], want), f"case {i}"
            assert np.array_equal(src[0], grid), f"case {i}: the source changed"
            assert np.array_equal(cnt[0] - c0[0], [np.sum(want == c) for c in codes]), f"case {i}"
        nonzero_empty += codes[0] != 0
    assert n >= 32 and nonzero_empty > 0


def test_ref_windy_step_gate_parity_and_null_counts():
    case = wr.case_contract(45, 40, 1, False)
    assert case["want_counts"] is None and case["parity"] is not None
    part = case["steps"] > 1
    assert part.sum() == 5  # steps 2, 3, 2, 3, 2 of CONTRACT_STEPS
    src = np.where((case["parity"] != 0)[:, None, None], case["buf1"], case["buf0"])
    dst = np.where((case["parity"] != 0)[:, None, None], case["want_buf0"], case["want_buf1"])
    for e in np.flatnonzero(part):
        ref = owindy.windy_step(src[e], wr.wind_of_mask(case["masks"][e]), wr.ROLL_HALF)
        assert np.array_equal(dst[e], ref)
    # the source buffer of every env is what it was
    assert np.array_equal(np.where((case["parity"] != 0)[:, None, None], case["want_buf1"], case["want_buf0"]), src)


def test_philox_rolls_and_masks_match_the_oracle_per_env():
    rng = np.random.default_rng(0)
    ids, steps = rng.integers(0, 5000, 40), rng.integers(0, 2**32, 40, dtype=np.uint64)
    steps[0] = 2**32 - 1
    rolls = wr.philox_rolls(0x5EED, ids, steps)
    wind = rng.random((40, 9))
    masks = wr.masks_of(wind, rolls)
    for k in range(40):
        want = owindy.philox_roll(0x5EED, int(ids[k]), int(steps[k]))
        assert np.array_equal(rolls[k].reshape(3, 3), want)
        assert masks[k] == owindy.dir_mask(wind[k], want)
    assert len(set(masks.tolist())) > 20


def test_ref_dirmask_gate_offset_pass_and_strict_ties():
    rng = np.random.default_rng(1)
    E = 30
    wind = rng.random((E, 12))
    rs = rng.integers(0, 2**32, E, dtype=np.uint64).astype(np.uint32)
    steps = rng.integers(0, 4, E).astype(np.int32)
    prev = np.full(E, 0xAA, np.uint8)
    got = wr.ref_dirmask(wind, 12, None, 9, rs, steps, 2, 100, prev)
    for e in range(E):
        want = owindy.dir_mask(wind[e, :9], owindy.philox_roll(9, 100 + e, (int(rs[e]) + 2) & 0xFFFFFFFF))
        assert got[e] == (want if steps[e] > 2 else 0xAA)
    assert np.all(prev == 0xAA) and (steps > 2).any() and (steps <= 2).any()
    # injected rolls: an exact tie roll == wind leaves the bit clear
    roll = rng.random((E, 9))
    tie = rng.random((E, 9)) < 0.3
    roll[tie] = wind[:, :9][tie]
    got = wr.ref_dirmask(wind, 12, roll, 0, None, None, 0, 0, prev)
    for e in range(E):
        for d, idx in enumerate(wr.DIRS):
            assert ((got[e] >> d) & 1) == (0 if tie[e, idx] else int(roll[e, idx] < wind[e, idx]))
    # stride 0: one wind for every env
    got0 = wr.ref_dirmask(wind[0, :9], 0, roll, 0, None, None, 0, 0, prev)
    assert np.array_equal(got0, wr.masks_of(np.repeat(wind[:1, :9], E, 0), roll))


@pytest.mark.parametrize("H,W", [(12, 16), (9, 23)])
def test_chained_pre_interpass_post_match_bulldozer_oracle(H, W):
    """The whole reference step (pre, 3 passes with interpass between them, post) against one BulldozerOracle per env
    (its own wind and global env id), 8 env steps: the current grid, position, hit, reward, done, accu, rng_step."""
    E, P, K = 10, 3, 8
    rng = np.random.default_rng(H)
    p = wr.Params(t_move=[1.1] * 4 + [0.0] + [1.1] * 4, t_shoot=[0.0, 0.8], t_any=0.3, seed=77, env_offset=5)
    grid = rng.choice(np.array(wr.STD_CODES, np.uint8), size=(E, H, W), p=[0.15, 0.75, 0.10])
    grid[3][grid[3] == 25] = 3
    wind = rng.random((E, 9)) * 0.6
    pos = wr.border_positions(E, H, W, rng)
    accu = rng.random(E)
    oracles = [owindy.BulldozerOracle([grid[e]], [pos[e]], wind[e].reshape(3, 3), 1.1, 0.8, 0.3, 77, env_offset=5 + e)
               for e in range(E)]
    for e, o in enumerate(oracles):
        o.accu[0] = accu[e]
    parity = rng.integers(0, 2, E).astype(np.uint8)
    odd = (parity != 0)[:, None, None]
    junk = np.full_like(grid, 0x5A)
    s = dict(buf0=np.where(odd, junk, grid), buf1=np.where(odd, grid, junk), parity=parity, accu=accu,
             steps=np.zeros(E, np.int32), counts=wr.count_cells(grid, wr.STD_CODES), pos=pos, hit=np.zeros(E, np.uint8),
             reward=np.zeros(E), done=np.zeros(E, np.uint8), rng_step=np.zeros(E, np.uint32),
             dir_mask=np.zeros(E, np.uint8))
    seen = set()
    for k in range(K):
        act = np.stack([rng.integers(0, 9, E), rng.integers(0, 2, E)], axis=1).astype(np.int32)
        act[0], act[2] = (4, 0), (4, 1)  # the cheapest actions: env steps without a CA pass
        was_done = s["done"].copy()
        s = wr.ref_env_step(p, P, s, act, wind, 9)
        seen.update(s["steps"].tolist())
        cur = np.where((s["parity"] != 0)[:, None, None], s["buf1"], s["buf0"])
        for e, o in enumerate(oracles):
            r = o.step([act[e]])[0]
            assert np.array_equal(cur[e], o.grids[0]), (k, e)
            assert tuple(s["pos"][e]) == o.pos[0] and s["accu"][e] == o.accu[0] and s["rng_step"][e] == o.rng_step[0]
            assert bool(s["done"][e]) == bool(o.done[0])
            assert (np.isnan(r) and np.isnan(s["reward"][e])) or r == s["reward"][e], (k, e)
            if not was_done[e]:
                assert bool(s["hit"][e]) == bool(o.hit[0])
        assert np.array_equal(s["counts"], wr.count_cells(cur, wr.STD_CODES))
    assert {-1, 0, 1, 2, 3} <= seen, seen


@pytest.mark.parametrize("shape", sorted(wr.MARCH_CASES))
def test_march_cases_reach_the_march(shape):
    sh, rpw, rows, nts = wr.march_reach(*shape)
    assert sh % rpw == 0 and sum(rows) == shape[1]


def test_strip_height_of_the_small_batches():
    """Every other fast-kernel case of the direct tests is a single chunk: the march is reached by case L alone."""
    for E, H, W in [(256, 20, 16), (256, 20, 64), (256, 20, 128), (256, 7, 1024), (9, 45, 64), (7, 45, 128)]:
        _, _, _, nts = wr.march_chunks(E, H, W)
        assert max(nts) == 1, (E, H, W, nts)
    assert wr.strip_height(2048, 128, 128) == 32 and wr.march_chunks(2048, 128, 128)[3] == [4, 4, 4, 4]


def _closed_form(g, m, codes):
    """TREE -> FIRE iff an active direction sees FIRE, FIRE -> EMPTY, else unchanged (the SWAR kernels' rule)."""
    empty, tree, fire = codes
    f = np.pad(g == fire, 1)
    H, W = g.shape
    any_ = np.zeros((H, W), bool)
    for d, idx in enumerate(wr.DIRS):
        if (m >> d) & 1:
            a, b = divmod(int(idx), 3)
            any_ |= f[1 - (a - 1): 1 - (a - 1) + H, 1 - (b - 1): 1 - (b - 1) + W]
    out = g.copy()
    out[(g == tree) & any_] = fire
    out[g == fire] = empty
    return out


def test_closed_form_rule_and_the_thresholds():
    """Where the SWAR kernels' rule is the reference's thresholds: on every grid for codes that satisfy the
    constructor's inequalities, on domino_fill grids for any empty = 0 < tree < fire, and NOT on dense grids of
    (0, 2, 9), (0, 127, 128), (0, 200, 255) -- which is why case C steps those codes' dense grids on the exact kernel
    only."""
    rng = np.random.default_rng(2)
    assert wr.closed_form_is_exact((0, 3, 25)) and wr.closed_form_is_exact((0, 20, 200))
    for codes in [(0, 3, 25), (0, 20, 200)]:
        g = wr.dense_fill(rng, 16, 12, 20, codes)
        for e in range(16):
            m = int(rng.integers(0, 256))
            assert np.array_equal(owindy.windy_step(g[e], wr.wind_of_mask(m), wr.ROLL_HALF, *codes),
                                  _closed_form(g[e], m, codes))
    for codes in [(0, 2, 9), (0, 127, 128), (0, 200, 255)]:
        assert not wr.closed_form_is_exact(codes)
        g = wr.domino_fill(rng, 16, 12, 20, codes)
        d = wr.dense_fill(rng, 16, 12, 20, codes)
        differ = 0
        for e in range(16):
            m = int(rng.integers(0, 256)) | 1
            assert np.array_equal(owindy.windy_step(g[e], wr.wind_of_mask(m), wr.ROLL_HALF, *codes),
                                  _closed_form(g[e], m, codes))
            differ += int(np.sum(owindy.windy_step(d[e], wr.wind_of_mask(255), wr.ROLL_HALF, *codes) !=
                                 _closed_form(d[e], 255, codes)))
        assert differ > 0, codes


def test_step_case_builders_assert_their_conditions():
    for fill in ("dense", "sparse"):
        case = wr.case_all_masks(20, 64, fill)
        assert case["E"] == 256 and np.array_equal(case["masks"], np.arange(256))
        assert np.array_equal(case["want_counts"], wr.count_cells(case["want_buf1"], wr.STD_CODES))
    g = wr.sparse_fill(256, 20, 64)
    fires = {(r, c) for e in range(256) for r, c in zip(*np.nonzero(g[e] == 25))}
    assert {c for _, c in fires} == {0, 3, 4, 15, 16, 63}
    assert {0, 19, 3, 4, 7, 8, 15, 16} <= {r for r, _ in fires}
    wr.case_contract(45, 64, 0, True)
    wr.case_codes(20, 64, (0, 127, 128), "domino")
    wr.case_codes(19, 17, (2, 7, 200), "bytes")
    # a builder whose condition fails raises: no fire, no ignition
    with pytest.raises(AssertionError):
        wr.step_case(np.full((2, 8, 16), 3, np.uint8), [255, 255], wr.STD_CODES)


def test_kernel_and_sequence_cases_reach_three_passes():
    case = wr.case_kernels()
    assert case["E"] == 600 and (case["steps"] == 3).sum() > 0 and (case["done"] != 0).sum() > 0
    for pass_ in (0, 1):  # interpass redraws for envs with n > pass + 1: 3-pass envs at pass 1
        assert (case["steps"] > pass_ + 1).any()
    for parity in (case["parity"], None):  # what test_bulldozer_post_alone needs of the reference
        want = wr.ref_post(case["p"], 2, case["action"], case["steps"], parity, case["buf0"], case["buf1"], case["pos"],
                           case["counts"], case["rng_step"], case["done"], case["hit"], case["reward"])
        assert (want["hit"] == 1).sum() > 50 and np.isnan(want["reward"]).any() and (want["reward"] == 0).any()
        assert (want["hit"] == 9).sum() == (case["steps"] < 0).sum() > 0  # done on entry: hit keeps its sentinel
        assert not np.array_equal(want["buf0"], case["buf0"])
        assert (parity is None) == np.array_equal(want["buf1"], case["buf1"])
    p, P, state, actions, wind = wr.case_sequence(300, 20, 64)
    seen, s = set(), state
    for k in range(2):
        s = wr.ref_env_step(p, P, s, actions[k], wind, 9)
        seen.update(s["steps"].tolist())
    assert P == 3 and {-1, 0, 1, 2, 3} <= seen and 0 < s["done"].sum() < 300
