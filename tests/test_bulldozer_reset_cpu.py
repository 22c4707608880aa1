"""CPU: the per-env reset of the batched ForestFireBulldozer env (gca_bulldozer_reset_where) in the host build of the
C-ABI against its numpy restatement (tests/_bulldozer_reset_ref.py), and the restatement against the definitions it
stands on (gca_fill_categorical's draw through oracle.philox, _seeding.env_integers). No GPU."""
import numpy as np
import pytest

import _bulldozer_reset_ref as ref
from gymca_amd import _seeding
from oracle import philox

SEED = 0x1234ABCD5678
OFF = 5
SHAPES = [(3, 7, 9), (2, 1, 1), (3, 5, 5), (2, 4, 67)]
CDF = ref.cdf_of(0.10, 0.60)  # all three codes appear


def _both(E, H, W, prepare=None, **kw):
    a = ref.make_state(E, H, W, seed=H * W)
    if prepare:
        prepare(a)
    b, before = ref.copy_state(a), ref.copy_state(a)
    sel = ref.ref_reset_where(a, SEED, OFF, CDF, **kw)
    ref.host_reset_where(b, SEED, OFF, CDF, **kw)
    ref.assert_states_equal(a, b, str(kw))
    return a, before, sel


def _assert_untouched(after, before, sel):
    for k in ref.FIELDS:
        if k in ("terminated", "truncated"):
            continue  # written for every env
        x, y = (after[k][:, ~sel], before[k][:, ~sel]) if k == "buf" else (after[k][~sel], before[k][~sel])
        assert np.array_equal(x, y), k
    assert np.array_equal(after["buf"][1], before["buf"][1])  # the other buffer, selected envs included


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("episode", [0, 1, 300])
def test_host_build_equals_the_restatement_partial_mask(shape, episode):
    E, H, W = shape
    mask = np.zeros(E, np.uint8)
    mask[::2] = 1
    a, before, sel = _both(E, H, W, mask=mask, set_episode=episode)
    assert np.array_equal(sel, mask.astype(bool))
    _assert_untouched(a, before, sel)
    assert (a["episode"][sel] == episode).all() and (a["last_length"][sel] == before["steps_elapsed"][sel]).all()
    assert not a["terminated"].any() and not a["truncated"].any()
    for e in np.flatnonzero(sel):
        assert a["counts"][e].tolist() == [int(np.sum(a["buf"][0, e] == v)) for v in ref.CODES]
        fr, fc = ref.fire_cell(SEED, OFF + e, episode, H, W)
        assert a["buf"][0, e, fr, fc] == 25
        assert 0 <= a["pos"][e, 0] < H and 0 <= a["pos"][e, 1] < W
        for name in ("parity", "accu", "done", "hit", "steps_elapsed"):
            assert a[name][e] == 0, name


@pytest.mark.parametrize("shape", SHAPES)
def test_null_mask_selects_the_done_envs_and_increments_the_episode(shape):
    E, H, W = shape

    def prepare(s):
        s["done"][E - 1] = 1

    a, before, sel = _both(E, H, W, prepare)
    assert sel.tolist() == [False] * (E - 1) + [True]
    _assert_untouched(a, before, sel)
    assert a["terminated"].tolist() == [0] * (E - 1) + [1] and not a["truncated"].any()
    assert a["episode"][E - 1] == before["episode"][E - 1] + 1 and a["done"][E - 1] == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_time_limit_hit_and_not_hit(shape):
    E, H, W = shape

    def prepare(s):
        s["steps_elapsed"][:] = [4, 5, 9][:E]
        s["done"][0] = 1  # done below the limit: terminated; env 1 at the limit: truncated

    a, before, sel = _both(E, H, W, prepare, max_steps=5)
    assert sel.tolist() == [True, True, True][:E]
    assert a["terminated"].tolist() == [1, 0, 0][:E] and a["truncated"].tolist() == [0, 1, 1][:E]
    assert a["last_length"].tolist() == [4, 5, 9][:E]
    a, before, sel = _both(E, H, W, prepare, max_steps=6)
    assert sel.tolist() == [True, False, True][:E]
    assert a["truncated"].tolist() == [0, 0, 1][:E]
    _assert_untouched(a, before, sel)
    a, before, sel = _both(E, H, W, prepare, max_steps=0)  # no limit
    assert sel.tolist() == [True, False, False][:E] and not a["truncated"].any()
    # a done env at its limit is terminated, not truncated; a mask does not switch the limit off
    a, before, sel = _both(E, H, W, prepare, mask=np.zeros(E, np.uint8), max_steps=4)
    assert sel.all() and a["terminated"].tolist() == [1, 0, 0][:E] and a["truncated"].tolist() == [0, 1, 1][:E]


def test_wrapping_episode_index():
    def prepare(s):
        s["episode"][:] = [0xFFFFFFFF, 0xFFFFFF, 7]

    a, _, _ = _both(3, 5, 5, prepare, mask=np.ones(3, np.uint8))
    assert a["episode"].tolist() == [0, 0x1000000, 8]


@pytest.mark.parametrize("shape", SHAPES)
def test_episode_zero_grid_is_fill_categorical(shape):
    """Episode 0's grid before the fire cell is planted is gca_fill_categorical's definition (gca.h: out[e][i] =
    values[first j with u < cdf[j]], u = u01_f32 of Philox((i >> 2, env_offset + e, 0, INIT))[i & 3]), evaluated cell by
    cell with oracle.philox; only the fire cell differs after the reset."""
    E, H, W = shape
    a, _, _ = _both(E, H, W, mask=np.ones(E, np.uint8), set_episode=0)
    key = philox.seed_key(SEED)
    for e in range(E):
        want = np.empty(H * W, np.uint8)
        for i in range(H * W):
            x = philox.philox4x32_10(np.array([i >> 2, OFF + e, 0, ref.TAG_INIT], np.uint64), key)
            u = philox.u01_f32(x[i & 3])
            want[i] = ref.CODES[next(j for j in range(3) if j == 2 or u < CDF[j])]
        want = want.reshape(H, W)
        assert np.array_equal(ref.fill_grid(SEED, OFF + e, 0, H, W, CDF), want)
        fr, fc = ref.fire_cell(SEED, OFF + e, 0, H, W)
        diff = np.argwhere(a["buf"][0, e] != want)
        assert all(tuple(d) == (fr, fc) for d in diff) and a["buf"][0, e, fr, fc] == 25


def test_episode_zero_draws_are_resets_own():
    for tag, n in ((1, 200), (2, 64), (3, 7), (4, 4097)):
        assert np.array_equal(_seeding.env_integers_episode(SEED, OFF, 9, tag, 0, max(1, n // 12), 0),
                              _seeding.env_integers(SEED, OFF, 9, tag, 0, max(1, n // 12)))
    a = _seeding.env_integers_episode(SEED, OFF, 64, 1, 0, 1000, 1)
    assert not np.array_equal(a, _seeding.env_integers(SEED, OFF, 64, 1, 0, 1000))
    # the episode's low 24 bits key the draw
    assert np.array_equal(_seeding.env_integers_episode(SEED, OFF, 8, 1, 0, 1000, 0x1000001), a[:8])
    with pytest.raises(ValueError):
        _seeding.env_integers_episode(SEED, OFF, 8, 256, 0, 10, 0)


def test_two_episodes_of_one_env_differ_and_sharding_holds():
    E, H, W = 3, 24, 36
    states = []
    for k in (1, 2):
        a, _, _ = _both(E, H, W, mask=np.ones(E, np.uint8), set_episode=k)
        states.append(a)
    for e in range(E):
        assert not np.array_equal(states[0]["buf"][0, e], states[1]["buf"][0, e])
    # env 1 of a shard at offset OFF is env 0 of a shard at offset OFF + 1
    b = ref.make_state(1, H, W)
    ref.host_reset_where(b, SEED, OFF + 1, CDF, mask=np.ones(1, np.uint8), set_episode=2)
    assert np.array_equal(b["buf"][0, 0], states[1]["buf"][0, 1]) and np.array_equal(b["pos"][0], states[1]["pos"][1])
    # the noise spans more than one value at this size
    assert len({tuple(s["pos"][e]) for s in states for e in range(E)}) > 1


def test_unaligned_env_bases_and_partial_last_quad():
    """H*W = 7*9 = 63: env bases at odd addresses and a 3-cell last quad."""
    a, _, _ = _both(3, 7, 9, mask=np.ones(3, np.uint8))
    for e in range(3):
        assert a["counts"][e].sum() == 63


def test_host_reset_refuses_bad_arguments():
    from gymca_amd import GCAError, _lib

    s = ref.make_state(1, 3, 3)
    with pytest.raises(GCAError, match="set_episode"):
        ref.host_reset_where(s, SEED, 0, CDF, set_episode=-2)
    with pytest.raises(GCAError, match="env_offset"):
        ref.host_reset_where(s, SEED, -1, CDF)
    p = _lib.BulldozerParams()
    with pytest.raises(GCAError, match="null"):
        _lib.call_cpu("gca_bulldozer_reset_where", p, 0, None, 0, -1, 1, 1, None, *([1] * 8), 3, 3, 1, 1, 1, 1, 1, None)
    with pytest.raises(GCAError, match="32768"):
        _lib.call_cpu("gca_bulldozer_reset_where", p, 0, None, 0, -1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 32768, 3, 1, 1, 1,
                      1, 1, None)
