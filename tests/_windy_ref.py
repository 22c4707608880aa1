"""The C contracts of gca_windy_step, gca_windy_dirmask, gca_bulldozer_pre / _interpass / _post (include/gca.h)
restated in numpy on oracle.windy and oracle.philox, and the cases tests/test_gpu_windy_direct.py runs on the device.
No torch, no device: tests/test_windy_ref_cpu.py holds all of it to the committed golden vectors and to
oracle.windy.BulldozerOracle on the CPU.

The per-env functions follow the text of include/gca.h and the reference lines it cites (repeat_ca.py:32-45,
move_modify.py:128-134, bulldozer.py:180-216), not the device code. Every function returns new arrays and leaves its
arguments unchanged, so a test can compare inputs that must not change as well.

Every case builder asserts, from the reference alone, the conditions that make the case worth running (ignitions,
masked-off neighbours that do not ignite, gated envs, both parities, counts that start non-zero, the march's strip
height): a case whose condition fails raises AssertionError, it is never skipped.
"""
import functools
import math

import numpy as np
from scipy.signal import convolve2d

from oracle import windy as owindy
from oracle.philox import philox4x32_10, seed_key, u01_f64

STD_CODES = (0, 3, 25)
DIRS = np.array([0, 1, 2, 3, 5, 6, 7, 8])  # 3x3 row-major index of direction bit d (centre skipped)
ROLL_HALF = np.full((3, 3), 0.5)
ONES3 = np.ones((3, 3), np.int64)


# ===================================================================== gca_windy_step
def wind_of_mask(m):
    """The 3x3 wind (1.0 / 0.0) under which a roll of 0.5 activates exactly the directions of mask m."""
    w = np.zeros(9)
    w[DIRS] = [(int(m) >> d) & 1 for d in range(8)]
    return w.reshape(3, 3)


def ref_windy_step(buf0, buf1, parity, steps, pass_, masks, codes, counts):
    """gca_windy_step: env e takes part iff steps is None or steps[e] > pass_; it reads buf[parity[e]] (buf0 when
    parity is None) and writes oracle.windy.windy_step of it -- the scipy convolve2d formula and the three thresholds
    -- to the other buffer; the new grid's EMPTY / TREE / FIRE counts are added to counts[e]. Every other byte, and
    every counts row of an env that does not take part, is unchanged. Returns new (buf0, buf1, counts)."""
    b = [np.array(buf0, np.uint8), np.array(buf1, np.uint8)]
    counts = None if counts is None else np.array(counts, np.int32)
    for e in range(b[0].shape[0]):
        if steps is not None and steps[e] <= pass_:
            continue
        s = 1 if (parity is not None and parity[e]) else 0
        out = owindy.windy_step(b[s][e], wind_of_mask(masks[e]), ROLL_HALF, *codes)
        b[1 - s][e] = out
        if counts is not None:
            counts[e] += [int(np.sum(out == c)) for c in codes]
    return b[0], b[1], counts


def closed_form_is_exact(codes):
    """Whether TREE -> FIRE iff an active direction sees FIRE, FIRE -> EMPTY, else unchanged equals the thresholds on
    EVERY grid of the three codes: the reference constructor's three inequalities (ca_windy.py:163-173) with
    identity 2048, propagation 8 and 8 neighbours."""
    e, t, f = codes
    i, p, n = owindy.IDENTITY, owindy.PROPAGATION, 8
    return e < t < f and i * e + n * p * f < i * t and n * p * t < p * f and i * t + n * p * f < i * f


def _nb_count(flag):
    return convolve2d(flag.astype(np.int64), ONES3, mode="same") - flag


def assert_step_conditions(src, out, codes, one_cause=False):
    """src, out: (E, H, W) source grids and reference outputs of the envs that took part. Ignitions happen, and some
    TREE next to FIRE stays TREE (its directions are masked off). one_cause: no TREE has two FIRE neighbours."""
    _, tree, fire = codes
    ign = masked = 0
    for g, o in zip(src, out):
        near = (g == tree) & (_nb_count(g == fire) > 0)
        ign += int(np.sum((g == tree) & (o == fire)))
        masked += int(np.sum(near & (o == tree)))
        if one_cause:
            assert int(_nb_count(g == fire)[g != fire].max(initial=0)) <= 1, "a cell with two FIRE neighbours"
    assert ign > 0, "no ignition in the case"
    assert masked > 0, "no TREE next to FIRE that stays TREE"


def dense_fill(rng, E, H, W, codes=STD_CODES, p=(0.2, 0.5, 0.3)):
    return rng.choice(np.array(codes, np.uint8), size=(E, H, W), p=p)


def interesting_rows(H, W):
    """Rows 0 and H - 1 and the rows either side of every boundary a kernel could have at this width: multiples of
    the fast kernel's rows per wave (64 / (W / 16)) and of 16 (the rows kernel's strip and every fast strip height)."""
    rows = {0, H - 1}
    rpw = max(1, 64 // max(1, W // 16))
    for step in {rpw, 4, 8, 16}:
        for b in range(step, H, step):
            rows.update((b - 1, b))
    return sorted(r for r in rows if 0 <= r < H)


def sparse_fill(E, H, W, codes=STD_CODES):
    """All TREE with isolated FIRE cells, any two at Chebyshev distance >= 3, so every ignition has exactly one
    cause: a wrong direction, or a wrap across a lane, row or grid edge, shows as one named cell. The fires sit on
    columns 0, 3, 4, 15, 16, W - 1 (dword, lane and grid edges) and on interesting_rows; env e starts its greedy
    placement at another candidate, so over the envs (and their masks) every candidate is used."""
    _, tree, fire = codes
    cols = sorted({c for c in (0, 3, 4, 15, 16, W - 1) if 0 <= c < W})
    cand = [(r, c) for r in interesting_rows(H, W) for c in cols]
    g = np.full((E, H, W), tree, np.uint8)
    for e in range(E):
        placed = []
        k0 = (e * 5) % len(cand)
        for r, c in cand[k0:] + cand[:k0]:
            if all(max(abs(r - r1), abs(c - c1)) >= 3 for r1, c1 in placed):
                placed.append((r, c))
                g[e, r, c] = fire
    return g


def domino_fill(rng, E, H, W, codes):
    """EMPTY with isolated pairs and singles: a TREE next to a FIRE in any of the 8 directions, two adjacent TREEs, a
    lone FIRE, a lone TREE; pieces at least two EMPTY cells apart. Every TREE then has at most one non-EMPTY neighbour,
    where the closed-form rule equals the thresholds for ANY empty = 0 < tree < fire (a lone active neighbour adds at
    most 8 * fire < 2048 * (fire - tree); a lone TREE neighbour adds 8 * tree < 8 * fire) -- also for codes that fail
    closed_form_is_exact, whose dense grids the SWAR kernels do not step as the thresholds do."""
    empty, tree, fire = codes
    g = np.full((E, H, W), empty, np.uint8)
    kinds = [(tree, fire), (fire, tree), (tree, tree), (fire, None), (tree, None)]
    offs = [(0, 1), (1, 0), (1, 1), (1, -1)]
    for e in range(E):
        # anchors on a 4-cell lattice with a per-env phase: pieces span at most 2 cells, so gaps are >= 2
        pr, pc = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        for r in range(pr, H, 4):
            for c in range(pc, W, 4):
                a, b = kinds[int(rng.integers(0, len(kinds)))]
                dr, dc = offs[int(rng.integers(0, len(offs)))]
                c0 = c + 1 if dc < 0 else c  # keep the piece inside its 2 x 2 lattice cell
                r1, c1 = r + dr, c0 + dc
                if b is not None and not (r1 < H and 0 <= c1 < W and c0 < W):
                    continue
                if c0 >= W:
                    continue
                g[e, r, c0] = a
                if b is not None:
                    g[e, r1, c1] = b
    return g


def step_case(src, masks, codes, parity=None, steps=None, pass_=0, counts0=None, sentinel=None, one_cause=False,
              conditions=True, counts_nonzero=True, cond_envs=None):
    """A gca_windy_step case: src (E, H, W) is laid into buf[parity[e]], `sentinel` (default: a byte pattern that is
    not a fixed point of anything) into the other buffer; the reference result is computed once here. Returns a dict
    with the inputs (buf0, buf1, parity, steps, pass_, masks, codes, counts0) and want_buf0, want_buf1, want_counts."""
    src = np.ascontiguousarray(src, np.uint8)
    E, H, W = src.shape
    if sentinel is None:
        sentinel = ((np.arange(E * H * W, dtype=np.int64) * 7 + 0xA5) % 251 + 4).astype(np.uint8).reshape(E, H, W)
    par = np.zeros(E, np.uint8) if parity is None else np.asarray(parity, np.uint8)
    odd = (par != 0)[:, None, None]
    buf0, buf1 = np.where(odd, sentinel, src), np.where(odd, src, sentinel)
    masks = np.asarray(masks, np.uint8)
    w0, w1, wc = ref_windy_step(buf0, buf1, parity, steps, pass_, masks, codes, counts0)
    part = np.ones(E, bool) if steps is None else np.asarray(steps) > pass_
    out = np.where(odd, w0, w1)
    if conditions:  # (cond_envs: on the first so many envs that take part, where the batch is large)
        assert_step_conditions(src[part][:cond_envs], out[part][:cond_envs], codes, one_cause)
    if steps is not None:
        assert part.any() and (~part).any(), "gated and ungated envs"
        assert np.array_equal(w0[~part], buf0[~part]) and np.array_equal(w1[~part], buf1[~part])
    if parity is not None:
        assert set(np.unique(par[part])) == {0, 1}, "both parities among the envs that take part"
    if counts0 is not None and counts_nonzero:
        assert np.all(np.asarray(counts0) != 0), "counts start non-zero"
    return dict(buf0=buf0, buf1=buf1, parity=None if parity is None else par,
                steps=None if steps is None else np.asarray(steps, np.int32), pass_=pass_, masks=masks, codes=codes,
                counts0=None if counts0 is None else np.asarray(counts0, np.int32), want_buf0=w0, want_buf1=w1,
                want_counts=wc, E=E, H=H, W=W)


@functools.lru_cache(maxsize=None)
def case_all_masks(H, W, fill):
    """Case A: E = 256 with dir_mask[e] = e on grids of (0, 3, 25); fill 'dense' (0.2 / 0.5 / 0.3) or 'sparse'."""
    E = 256
    rng = np.random.default_rng(1000 * H + W)
    src = dense_fill(rng, E, H, W) if fill == "dense" else sparse_fill(E, H, W)
    return step_case(src, np.arange(E), STD_CODES, counts0=np.zeros((E, 3), np.int32), one_cause=fill == "sparse",
                     counts_nonzero=False)


CONTRACT_STEPS = np.array([-1, 0, 1, 2, 3, 1, 2, 3, 2], np.int32)
CONTRACT_PARITY = np.array([1, 0, 0, 1, 1, 1, 0, 0, 1], np.uint8)


@functools.lru_cache(maxsize=None)
def case_contract(H, W, pass_, with_counts, codes=STD_CODES):
    """Case B: E = 9, steps in {-1, 0, 1, 2, 3} against pass_, mixed parity, counts pre-filled (or NULL), the
    destination of every env holding a sentinel."""
    E = 9
    rng = np.random.default_rng(31 * W + pass_)
    src = dense_fill(rng, E, H, W, codes)
    counts0 = rng.integers(1, 1000, (E, 3)).astype(np.int32) if with_counts else None
    return step_case(src, rng.integers(0, 256, E), codes, parity=CONTRACT_PARITY, steps=CONTRACT_STEPS, pass_=pass_,
                     counts0=counts0)


@functools.lru_cache(maxsize=None)
def case_codes(H, W, codes, fill):
    """Case C: 'dense' (codes drawn 0.2 / 0.5 / 0.3), 'domino' (domino_fill) or 'bytes' (cells from all 256 byte
    values plus the three codes, for the exact kernel: 'any u8 cell codes')."""
    E = 64
    rng = np.random.default_rng(sum(codes) + W)
    if fill == "dense":
        src = dense_fill(rng, E, H, W, codes)
    elif fill == "domino":
        src = domino_fill(rng, E, H, W, codes)
    else:
        src = rng.integers(0, 256, (E, H, W)).astype(np.uint8)
        pick = rng.random((E, H, W)) < 0.6
        src[pick] = dense_fill(rng, E, H, W, codes)[pick]
    counts0 = rng.integers(1, 50, (E, 3)).astype(np.int32)
    return step_case(src, rng.integers(0, 256, E), codes, counts0=counts0)


@functools.lru_cache(maxsize=None)
def case_shape(E, H, W, seed=0):
    """Cases D and E: a dense (0, 3, 25) grid of an edge shape, random masks and parity, counts pre-filled. The
    conditions (ignitions, masked-off neighbours) are asserted where the shape has a neighbour at all."""
    rng = np.random.default_rng(7 * H + W + seed)
    src = dense_fill(rng, E, H, W)
    parity = (np.arange(E) % 2).astype(np.uint8)
    counts0 = rng.integers(1, 50, (E, 3)).astype(np.int32)
    return step_case(src, rng.integers(1, 255, E), STD_CODES, parity=parity, counts0=counts0, conditions=H * W >= 256)


# --------------------------------------------------------------------- the strip march of windy_fast_kernel
def strip_height(E, H, W):
    """The strip height SH that gca_windy_step's host code (launch_fast in gca_windy.hip) picks for the SWAR kernel at
    this batch: 32, halved while E*H / SH < 8192, not below the rows one wave covers per step (RPW = 64 / (W / 16))
    and a multiple of it. This MIRRORS the host code on purpose, and is used only to assert that a case reaches the
    kernel's march over several chunks (nT = ceil(strip rows / RPW) >= 2): the ABI gives no way to choose SH, so a
    case can only reach that path through its batch size, and a change of the heuristic must fail the case's
    assertion instead of silently turning it into one more single-chunk test."""
    lpr = W // 16
    assert W % 16 == 0 and 1 <= lpr <= 64 and 64 % lpr == 0 and W not in (256, 512), "not a SWAR-kernel width"
    rpw = 64 // lpr
    rows, sh = E * H, 32
    while sh > rpw and rows // sh < 8192:
        sh >>= 1
    sh = max(sh, rpw)
    return -(-sh // rpw) * rpw


def march_chunks(E, H, W):
    """(SH, RPW, [rows of each strip], [nT of each strip]) for the batch."""
    sh, rpw = strip_height(E, H, W), 64 // (W // 16)
    rows = [min(s + sh, H) - s for s in range(0, H, sh)]
    return sh, rpw, rows, [-(-r // rpw) for r in rows]


MARCH_CASES = {  # (E, H, W): (SH, nT of the first strip, rows of the last strip)
    (1860, 141, 128): (32, 4, 13),
    (1703, 77, 128): (16, 2, 13),
    (3405, 77, 64): (32, 2, 13),
    (2979, 11, 1024): (4, 4, 3),
}


def march_reach(E, H, W):
    """Asserts the reach conditions of case L from strip_height alone (no grid): cheap enough for the CPU suite."""
    sh, rpw, rows, nts = march_chunks(E, H, W)
    want_sh, want_nt, want_last = MARCH_CASES[(E, H, W)]
    assert (sh, nts[0], rows[-1]) == (want_sh, want_nt, want_last), (sh, rpw, rows, nts)
    assert nts[0] >= 2 and len(rows) >= 2
    return sh, rpw, rows, nts


def case_march(E, H, W):
    """Case L: the smallest batches at which windy_fast_kernel marches (nT >= 2). Random masks, mixed parity, one env
    in eight gated off, counts pre-filled."""
    march_reach(E, H, W)
    rng = np.random.default_rng(E + H + W)
    src = dense_fill(rng, E, H, W)
    parity = rng.integers(0, 2, E).astype(np.uint8)
    steps = np.where(rng.random(E) < 0.125, 1, 2).astype(np.int32)
    counts0 = rng.integers(1, 50, (E, 3)).astype(np.int32)
    return step_case(src, rng.integers(0, 256, E), STD_CODES, parity=parity, steps=steps, pass_=1, counts0=counts0,
                     sentinel=np.full((E, H, W), 0x5A, np.uint8), cond_envs=64)


# ===================================================================== gca_windy_dirmask
def philox_rolls(seed, env_ids, steps):
    """oracle.windy.philox_roll for many (env id, step) pairs at once: (n, 9) doubles, centre 0.5."""
    env_ids = np.asarray(env_ids, np.uint64) & np.uint64(0xFFFFFFFF)
    steps = np.asarray(steps, np.uint64) & np.uint64(0xFFFFFFFF)
    n = len(env_ids)
    ctr = np.empty((n, 4, 4), np.uint64)
    ctr[:, :, 0] = np.arange(4, dtype=np.uint64)
    ctr[:, :, 1] = env_ids[:, None]
    ctr[:, :, 2] = steps[:, None]
    ctr[:, :, 3] = owindy.TAG_WINDY_ROLL
    x = philox4x32_10(ctr, seed_key(seed))
    roll = np.full((n, 9), 0.5)
    for j in range(4):
        roll[:, DIRS[2 * j]] = u01_f64(x[:, j, 0], x[:, j, 1])
        roll[:, DIRS[2 * j + 1]] = u01_f64(x[:, j, 2], x[:, j, 3])
    return roll


def masks_of(wind_rows, rolls):
    """oracle.windy.dir_mask per row: bit d set iff roll < wind, strictly."""
    bits = rolls[:, DIRS] < wind_rows[:, DIRS]
    return (bits.astype(np.int64) << np.arange(8)).sum(axis=1).astype(np.uint8)


def wind_rows(wind, wind_stride, E):
    wind = np.asarray(wind, np.float64).ravel()
    return np.stack([wind[e * wind_stride: e * wind_stride + 9] for e in range(E)])


def ref_dirmask(wind, wind_stride, roll, seed, rng_step, steps, pass_, env_offset, prev):
    """gca_windy_dirmask: the masks of the envs with steps is None or steps[e] > pass_, from the injected rolls
    (E, 9), or from Philox at (env_offset + e, rng_step[e] + pass_) (rng_step None: 0); every other entry is prev's."""
    prev = np.array(prev, np.uint8)
    E = len(prev)
    if roll is None:
        rs = np.zeros(E, np.uint64) if rng_step is None else np.asarray(rng_step).astype(np.uint64)
        roll = philox_rolls(seed, env_offset + np.arange(E), rs + np.uint64(pass_))
    m = masks_of(wind_rows(wind, wind_stride, E), np.asarray(roll, np.float64).reshape(E, 9))
    on = np.ones(E, bool) if steps is None else np.asarray(steps) > pass_
    prev[on] = m[on]
    return prev


# ===================================================================== the three per-env bulldozer kernels
class Params:
    """gca_bulldozer_params as plain Python: timings, the Philox seed, codes, the reference's action sets and effects."""

    def __init__(self, t_move, t_shoot, t_any, seed, env_offset=0, codes=STD_CODES, effects=None):
        self.t_move = [float(v) for v in t_move]
        self.t_shoot = [float(v) for v in t_shoot]
        self.t_any = float(t_any)
        self.seed, self.env_offset, self.codes = int(seed), int(env_offset), tuple(codes)
        self.effects = {codes[1]: codes[0]} if effects is None else dict(effects)
        self.sets = dict(up=owindy.UP, down=owindy.DOWN, left=owindy.LEFT, right=owindy.RIGHT)
        assert len(self.t_move) == 9 and len(self.t_shoot) == 2


def _category(v, codes):
    return codes.index(v) if v in codes else -1


def ref_pre(p, action, accu, steps, done, wind, wind_stride, rng_step, dir_mask, counts):
    """gca_bulldozer_pre (repeat_ca.py:32-45): a live env adds (t_move[a0] + t_shoot[a1]) + t_any to accu, and
    (accu, steps) = math.modf of the sum; an env that steps (steps > 0) has its counts zeroed and its pass-0 mask
    drawn at rng_step[e]. An env done on entry gets steps = -1 and nothing else. Returns (accu, steps, dir_mask,
    counts)."""
    accu, steps = np.array(accu, np.float64), np.array(steps, np.int32)
    dir_mask, counts = np.array(dir_mask, np.uint8), np.array(counts, np.int32)
    E = len(accu)
    for e in range(E):
        if done is not None and done[e]:
            steps[e] = -1
            continue
        a0, a1 = int(action[e][0]), int(action[e][1])
        frac, reps = math.modf(accu[e] + ((p.t_move[a0] + p.t_shoot[a1]) + p.t_any))
        accu[e], steps[e] = frac, int(reps)
    go = steps > 0
    if go.any():
        counts[go] = 0
        ids = np.flatnonzero(go)
        rolls = philox_rolls(p.seed, p.env_offset + ids, np.asarray(rng_step)[ids])
        dir_mask[go] = masks_of(wind_rows(wind, wind_stride, E)[ids], rolls)
    return accu, steps, dir_mask, counts


def ref_interpass(p, pass_, steps, parity, wind, wind_stride, rng_step, dir_mask, counts):
    """gca_bulldozer_interpass between passes pass_ and pass_ + 1: envs that stepped in pass_ (steps > pass_) flip
    parity; envs that step again (steps > pass_ + 1) have their counts zeroed and the mask of pass_ + 1 drawn at
    rng_step[e] + pass_ + 1. Returns (parity, dir_mask, counts)."""
    steps = np.asarray(steps)
    parity, dir_mask, counts = np.array(parity, np.uint8), np.array(dir_mask, np.uint8), np.array(counts, np.int32)
    parity[steps > pass_] ^= 1
    go = steps > pass_ + 1
    if go.any():
        counts[go] = 0
        ids = np.flatnonzero(go)
        rolls = philox_rolls(p.seed, p.env_offset + ids, np.asarray(rng_step).astype(np.uint64)[ids] + np.uint64(pass_ + 1))
        dir_mask[go] = masks_of(wind_rows(wind, wind_stride, len(steps))[ids], rolls)
    return parity, dir_mask, counts


def ref_post(p, last_pass, action, steps, parity, buf0, buf1, pos, counts, rng_step, done, hit, reward):
    """gca_bulldozer_post (move_modify.py:128-134, bulldozer.py:180-216): an env done on entry (steps < 0) gets
    reward 0 and nothing else. Every other env: parity flips if it stepped in last_pass; Move; Modify in place on
    buf[parity[e]] (buf0 when parity is None) at the new position, adjusting the counts of the categories involved;
    reward = -(f / (t + f)) (NaN when t + f == 0), done = (f == 0), rng_step += steps. Returns a dict of new arrays."""
    steps = np.asarray(steps)
    out = dict(parity=None if parity is None else np.array(parity, np.uint8), buf0=np.array(buf0, np.uint8),
               buf1=None if buf1 is None else np.array(buf1, np.uint8), pos=np.array(pos, np.int32),
               counts=np.array(counts, np.int32), rng_step=np.array(rng_step, np.uint32), done=np.array(done, np.uint8),
               hit=np.array(hit, np.uint8), reward=np.array(reward, np.float64))
    E, H, W = out["buf0"].shape
    for e in range(E):
        n = int(steps[e])
        if n < 0:
            out["reward"][e] = 0.0
            continue
        if parity is not None and n > last_pass:
            out["parity"][e] ^= 1
        grid = (out["buf1"] if parity is not None and out["parity"][e] else out["buf0"])[e]
        a0, a1 = int(action[e][0]), int(action[e][1])
        r, c = owindy.move(out["pos"][e], a0, H, W)
        out["pos"][e] = (r, c)
        h = 0
        if a1 and int(grid[r, c]) in p.effects:
            v = int(grid[r, c])
            nv = p.effects[v]
            grid[r, c] = nv
            h = 1
            for val, d in ((v, -1), (nv, 1)):
                k = _category(val, p.codes)
                if k >= 0:
                    out["counts"][e, k] += d
        out["hit"][e] = h
        t, f = int(out["counts"][e, 1]), int(out["counts"][e, 2])
        out["reward"][e] = -(f / (t + f)) if t + f > 0 else float("nan")
        out["done"][e] = 1 if f == 0 else 0
        out["rng_step"][e] = (int(out["rng_step"][e]) + n) & 0xFFFFFFFF
    return out


def ref_env_step(p, P, state, action, wind, wind_stride):
    """One env step as batched.py chains the raw calls: pre, then P passes of windy_step with interpass between
    consecutive passes, then post(last_pass = P - 1). state: dict of buf0, buf1, parity, accu, steps, counts, pos,
    hit, reward, done, rng_step, dir_mask; returns the new one."""
    s = dict(state)
    s["accu"], s["steps"], s["dir_mask"], s["counts"] = ref_pre(p, action, s["accu"], s["steps"], s["done"], wind,
                                                               wind_stride, s["rng_step"], s["dir_mask"], s["counts"])
    for pss in range(P):
        s["buf0"], s["buf1"], s["counts"] = ref_windy_step(s["buf0"], s["buf1"], s["parity"], s["steps"], pss,
                                                          s["dir_mask"], p.codes, s["counts"])
        if pss < P - 1:
            s["parity"], s["dir_mask"], s["counts"] = ref_interpass(p, pss, s["steps"], s["parity"], wind, wind_stride,
                                                                   s["rng_step"], s["dir_mask"], s["counts"])
    post = ref_post(p, P - 1, action, s["steps"], s["parity"], s["buf0"], s["buf1"], s["pos"], s["counts"],
                    s["rng_step"], s["done"], s["hit"], s["reward"])
    s.update(post)
    return s


def count_cells(grids, codes):
    return np.stack([[int(np.sum(g == c)) for c in codes] for g in grids]).astype(np.int32)


ALL_ACTIONS = [(m, s) for m in range(9) for s in (0, 1)]  # the 18 in-range actions
KERNEL_TIMINGS = dict(t_move=[0.9, 0.4, 1.1, 0.3, 0.0, 0.7, 1.2, 0.5, 0.8], t_shoot=[0.0, 0.6], t_any=0.55)


def border_positions(E, H, W, rng):
    """Every corner, a cell of every border and interior cells, cycled over the envs."""
    fixed = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)]
    pos = np.stack([rng.integers(0, H, E), rng.integers(0, W, E)], axis=1)
    for e in range(0, E, 2):
        pos[e] = fixed[(e // 2) % len(fixed)]
    return pos.astype(np.int32)


def case_kernels(E=600, H=8, W=64, codes=(1, 7, 200), seed=5):
    """The inputs of the three per-env kernels, each run alone: timings that give 0 to 3 passes, done envs, a non-zero
    accu, per-env rng_step and wind (stride 9), all 18 actions, positions on every border and corner, non-standard
    codes, a grid with a byte that is no code (50), and effects that map TREE -> EMPTY, a non-category byte -> FIRE
    and FIRE -> a non-category byte."""
    rng = np.random.default_rng(seed)
    empty, tree, fire = codes
    p = Params(seed=0xB0117, env_offset=100, codes=codes, effects={tree: empty, 50: fire, fire: 60}, **KERNEL_TIMINGS)
    action = np.array([ALL_ACTIONS[(e * 7 + e // 18) % 18] for e in range(E)], np.int32)
    accu = rng.random(E)
    done = (rng.random(E) < 0.2).astype(np.uint8)
    done[5:7] = 0
    action[5], action[6] = (1, 0), (7, 0)  # live, no Modify: the counts set below decide reward and done
    wind = rng.random((E, 9))
    rng_step = rng.integers(0, 2**32, E, dtype=np.uint64).astype(np.uint32)
    rng_step[:3] = (2**32 - 1, 2**32 - 2, 0)  # the 32-bit wrap of rng_step + pass
    grids = rng.choice(np.array([empty, tree, fire, 50], np.uint8), size=(2, E, H, W), p=[0.2, 0.4, 0.3, 0.1])
    pos = border_positions(E, H, W, rng)
    parity = rng.integers(0, 2, E).astype(np.uint8)
    counts = rng.integers(1, 400, (E, 3)).astype(np.int32)
    counts[5] = (3, 0, 0)   # t + f == 0: the NaN reward
    counts[6] = (3, 9, 0)   # f == 0: done
    dir_mask = rng.integers(0, 256, E).astype(np.uint8)
    steps0 = np.full(E, 77, np.int32)
    _, steps, _, _ = ref_pre(p, action, accu, steps0, done, wind, 9, rng_step, dir_mask, counts)
    assert set(np.unique(steps)) == {-1, 0, 1, 2, 3}, np.unique(steps)
    assert {tuple(a) for a in action[steps >= 0]} == set(ALL_ACTIONS)
    assert accu.min() > 0 and set(np.unique(parity)) == {0, 1}
    return dict(p=p, E=E, H=H, W=W, action=action, accu=accu, done=done, wind=wind, rng_step=rng_step, buf0=grids[0],
                buf1=grids[1], pos=pos, parity=parity, counts=counts, dir_mask=dir_mask, steps0=steps0, steps=steps,
                hit=np.full(E, 9, np.uint8), reward=np.full(E, 123.5))


def case_sequence(E, H, W, seed=11):
    """The initial state and the per-step actions of the whole-sequence test: (0, 3, 25) grids, fires sprinkled (some
    envs with none, so they finish at the first step), one env done on entry, per-env wind, up to 3 passes per step."""
    rng = np.random.default_rng(seed + W)
    p = Params(t_move=[1.1, 1.1, 1.1, 1.1, 0.0, 1.1, 1.1, 1.1, 1.1], t_shoot=[0.0, 0.8], t_any=0.3, seed=0xD02E5,
               env_offset=40)
    grid = rng.choice(np.array(STD_CODES, np.uint8), size=(E, H, W), p=[0.15, 0.8, 0.05])
    grid[::7][grid[::7] == 25] = 3  # envs without fire
    parity = rng.integers(0, 2, E).astype(np.uint8)
    junk = np.full((E, H, W), 0x5A, np.uint8)
    odd = (parity != 0)[:, None, None]
    done = np.zeros(E, np.uint8)
    done[1] = 1
    state = dict(buf0=np.where(odd, junk, grid), buf1=np.where(odd, grid, junk), parity=parity, accu=rng.random(E),
                 steps=np.zeros(E, np.int32), counts=count_cells(grid, STD_CODES), pos=border_positions(E, H, W, rng),
                 hit=np.zeros(E, np.uint8), reward=np.zeros(E), done=done,
                 rng_step=rng.integers(0, 1000, E).astype(np.uint32), dir_mask=np.zeros(E, np.uint8))
    actions = np.stack([rng.integers(0, 9, (6, E)), rng.integers(0, 2, (6, E))], axis=2).astype(np.int32)
    wind = rng.random((E, 9)) * 0.7
    return p, 3, state, actions, wind
