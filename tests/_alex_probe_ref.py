"""Saturated-probability probes of the Alexandridis step and their numpy reference. Test infrastructure only.

The rule burns a TREE iff u < 1 - q, q = prod(1 - clamp01(p_d)) over its burning neighbours, u in [0, 1 - 2^-24]. With
parameters under which every p_d is either >= 1 or <= 2^-25 (q = 0: burns whatever u is; q = 1 exactly: never burns) one
step is a pure integer function of the neighbourhood: shifts and box counts in int64, no float arithmetic, no oracle
and no draw. Each builder starts from make_alex_params(H, 0, 1, 2, winds(), p_tree, seed) and overwrites fields; the
age range holds the single value AGE, so every new fire's age is known.

A probe is a Probe(label, p, case, pred, grow, edge, planes): `pred` the boolean predicate (a TREE burns iff pred),
`edge` / `planes` the slope probe's edge-layout values (E, 4, H, W) and direction factors (E, 8, H, W) (None: flat).
The sweeps (heat ring over T, dousing over T, layers over the classes) share one state and yield one probe per value.
The states are cached and read-only; expected() never writes into them.
"""
import ctypes
from collections import namedtuple
from functools import lru_cache

import numpy as np

from alex_cases import winds
from oracle import edge_slope

BIG = float(2 ** 20)
AGE = 5            # the single value of the age range [age_lo, age_hi)
EMPTY, TREE, FIRE = 0, 1, 2
# direction d = (a, b) of the 3 x 3 block, row-major without the centre: the neighbour of (r, c) is (r + DR, c + DC)
DR = (-1, -1, -1, 0, 0, 1, 1, 1)
DC = (-1, 0, 1, -1, 1, -1, 0, 1)
UNIFORM_VD = (4, 2)  # vegetation / density of the uniform-layer instance outside the layer probe (both factors > 0)

Probe = namedtuple("Probe", "label p case pred grow edge planes")

# (W, R) of the direction, dousing, layer, slope and growth probes; H = 32: two tiles (rows 15 | 16 a tile boundary)
H = 32
WIDTHS = ((256, 1), (256, 6), (512, 7), (1024, 8))
SEED = 11
DIR_SEEDS = (11, 12, 13)  # states of the direction probe (one launch of E = 9 each; coverage is on their union)
DOUS_MODES = ((1.0, 0.0), (1.0, 1.0), (2.0, 1.0))  # (dous_inner, dous_border): D_1, D_2, D_1 + D_2


def heat_plan(mode, W):
    """(R, k) pairs of the heat-ring probe: every R = 1..8 with every k <= R at W = 256 on the uniform and the general
    instance; R in {1, 6, 7, 8} with k in {1, R} elsewhere."""
    if W == 256 and mode in ("uniform", "general"):
        return [(R, k) for R in range(1, 9) for k in range(1, R + 1)]
    return [(R, k) for R in (1, 6, 7, 8) for k in sorted({1, R})]


# ---------------------------------------------------------------------------------------------- numpy helpers
def shift(a, dr, dc):
    """out[..., r, c] = a[..., r + dr, c + dc], 0 outside the grid."""
    out = np.zeros_like(a)
    h, w = a.shape[-2:]
    rs, re = max(0, -dr), min(h, h - dr)
    cs, ce = max(0, -dc), min(w, w - dc)
    out[..., rs:re, cs:ce] = a[..., rs + dr:re + dr, cs + dc:ce + dc]
    return out


def nbr_fire(grid):
    """(8, E, H, W) bool: the neighbour in direction d is FIRE (outside the grid: not)."""
    f = grid == FIRE
    return np.stack([shift(f, DR[d], DC[d]) for d in range(8)])


def box(x, k):
    """(2k+1)^2 box sums of x (..., H, W) with zero padding, int64."""
    x = np.asarray(x, np.int64)
    h, w = x.shape[-2:]
    n = 2 * k + 1
    pad = np.zeros(x.shape[:-2] + (h + n, w + n), np.int64)
    pad[..., k + 1:k + 1 + h, k + 1:k + 1 + w] = x
    s = pad.cumsum(-2).cumsum(-1)
    return s[..., n:, n:] - s[..., :-n, n:] - s[..., n:, :-n] + s[..., :-n, :-n]


def expected(pr):
    """(grid, ages, counts) after one step of probe `pr`: TREE -> FIRE iff pred, FIRE -> EMPTY iff age <= 1, EMPTY ->
    TREE iff grow; FIRE ages one less, new fires AGE, everything else unchanged."""
    g, a = pr.case["grid"], pr.case["age"]
    tree, fire = g == TREE, g == FIRE
    burn = tree & pr.pred
    out = g.copy()
    out[burn] = FIRE
    out[fire & (a <= 1)] = EMPTY
    if pr.grow:
        out[g == EMPTY] = TREE
    age = a.copy()
    age[fire] -= 1
    age[burn] = AGE
    counts = np.stack([(out == c).sum(axis=(1, 2)) for c in (EMPTY, TREE, FIRE)], axis=1).astype(np.int32)
    return out, age, counts


def probed(pr):
    """The cells the probe decides: TREEs with a burning neighbour."""
    return (pr.case["grid"] == TREE) & nbr_fire(pr.case["grid"]).any(axis=0)


# ---------------------------------------------------------------------------------------------- states
def _freeze(case):
    for v in case.values():
        v.setflags(write=False)
    return case


@lru_cache(maxsize=None)
def state(E, h, w, seed, fire_p, dous_p=0.0, sparse_dous=False, uniform=None):
    """grid iid {EMPTY .1, TREE, FIRE fire_p}; FIRE ages -2..5 (both sides of the burn-out test), others -3..3;
    vegetation / density 0..6 (or the `uniform` pair everywhere); dousing iid dous_p, or the sparse field."""
    rng = np.random.default_rng(seed)
    grid = rng.choice([EMPTY, TREE, FIRE], size=(E, h, w), p=[0.1, 0.9 - fire_p, fire_p]).astype(np.uint8)
    age = np.where(grid == FIRE, rng.integers(-2, 6, (E, h, w)), rng.integers(-3, 4, (E, h, w))).astype(np.int16)
    veg = rng.integers(0, 7, (E, h, w)).astype(np.uint8)
    den = rng.integers(0, 7, (E, h, w)).astype(np.uint8)
    if uniform is not None:
        veg[...], den[...] = uniform
    dous = (rng.random((E, h, w)) < dous_p).astype(np.uint8)
    if sparse_dous:
        dous[...] = 0
        rows = (0, 15, 16, h - 1, 7, 24)
        n = 0
        for b in range(256, w + 1, 256):  # columns 254..257, 510..513, ...: both sides of every segment boundary
            for c in (b - 2, b - 1, b, b + 1):
                if c < w:
                    dous[n % E, rows[n % len(rows)], c] = 1
                    n += 1
        for e, r, c in ((0, 0, 5), (1 % E, h - 1, w - 1), (2 % E, 15, 128), (2 % E, 16, 129), (0, 15, 255),
                        (0, 16, 256 % w), (1 % E, 0, 0), (1 % E, 1, 1)):
            dous[e, r % h, c % w] = 1
        for i, r in enumerate((0, 15, 16, h - 1)):  # a few more on the tile / grid edge rows
            for c in (37 + 11 * i, 38 + 11 * i, 150 + 7 * i):
                dous[i % E, r, c % w] = 1
    widx = rng.integers(0, 8, E).astype(np.int32)
    return _freeze(dict(grid=grid, age=age, veg=veg, den=den, dous=dous, widx=widx))


def _params(h, R, p_tree=0.0, seed=1):
    from gymca_amd.forest_fire.operators.ca_alexandridis import make_alex_params

    p, _ = make_alex_params(h, EMPTY, TREE, FIRE, winds(), p_tree, seed)
    p.R = R
    p.age_lo = p.age_hi = AGE
    for k in range(9):
        p.heat_dw[k] = 0.0
    p.dous_inner = p.dous_border = 0.0
    p.heat0 = 1.0
    return p


def _set_winds(p, rows):
    """rows: (n, 8) values per direction (the centre of the 3 x 3 matrix is 0)."""
    p.n_winds = len(rows)
    for i, row in enumerate(rows):
        for d in range(8):
            p.winds[i][d if d < 4 else d + 1] = float(row[d])
        p.winds[i][4] = 0.0


def clone(p):
    q = type(p)()
    ctypes.memmove(ctypes.addressof(q), ctypes.addressof(p), ctypes.sizeof(q))
    return q


def _uniform(p, uniform, vd=UNIFORM_VD):
    if uniform:
        p.vd_uniform = vd[0] | vd[1] << 4
    return vd if uniform else None


# ---------------------------------------------------------------------------------------------- the probes
def direction(h, w, R, seed, uniform=False, grow=False, fire_p=0.3):
    """Env d (0..7) burns a TREE iff its neighbour in direction d is FIRE (wind BIG in that direction only); env 8 iff
    any neighbour is. grow: p_tree = 1.0 (u < 1 always: every EMPTY cell becomes TREE; the GROW instances)."""
    p = _params(h, R, p_tree=1.0 if grow else 0.0, seed=seed)
    _set_winds(p, [[BIG if d == e else 0.0 for d in range(8)] for e in range(8)] + [[BIG] * 8])
    case = dict(state(9, h, w, seed, fire_p, uniform=_uniform(p, uniform)))
    case["widx"] = np.arange(9, dtype=np.int32)
    nb = nbr_fire(case["grid"])
    pred = np.concatenate([nb[d, d][None] for d in range(8)] + [nb[:, 8].any(axis=0)[None]])
    return Probe(f"direction W={w} R={R} grow={grow}", p, case, pred, grow, None, None)


def heat_ring(h, w, R, k, seed, uniform=False, E=4):
    """heat = 0.5 - T + B_k: a probed TREE burns iff B_k >= T, B_k the FIRE count of its (2k+1)^2 box. One probe per
    T = 1 .. max(B_k) + 1 (the maximum over the probed cells: the last T burns nothing)."""
    p0 = _params(h, R, seed=seed)
    _set_winds(p0, [[BIG] * 8] * 8)
    p0.heat_dw[k] = 1.0
    fire_p = max(4.0 / (2 * k + 1) ** 2, 0.04)  # (0.03 left a column of 3 x 32 cells without a probed TREE)
    case = state(E, h, w, seed + 100 * k, fire_p, uniform=_uniform(p0, uniform))
    any_f = nbr_fire(case["grid"]).any(axis=0)
    B = box(case["grid"] == FIRE, k)
    for T in range(1, int(B[any_f & (case["grid"] == TREE)].max()) + 2):
        p = clone(p0)
        p.heat0 = 0.5 - T
        yield Probe(f"heat ring W={w} R={R} k={k} T={T}", p, case, any_f & (B >= T), False, None, None)


def dousing(h, w, R, mode, sparse, seed, uniform=False, E=3):
    """heat = T - 0.5 - (D_1 | D_2 | D_1 + D_2): a probed TREE burns iff that dousing count <= T - 1 (D_1, D_2 the
    3 x 3 and 5 x 5 box counts). One probe per T = 1 .. max + 1. sparse: a handful of doused cells on the segment
    boundaries and the tile / grid edge rows (most wave-rows skip the dousing term; the halo carries the sums)."""
    inner, border = DOUS_MODES[mode]
    p0 = _params(h, R, seed=seed)
    _set_winds(p0, [[BIG] * 8] * 8)
    p0.dous_inner, p0.dous_border = inner, border
    case = state(E, h, w, seed, 0.15, dous_p=0.15, sparse_dous=sparse, uniform=_uniform(p0, uniform))
    any_f = nbr_fire(case["grid"]).any(axis=0)
    D1, D2 = box(case["dous"], 1), box(case["dous"], 2)
    D = (D1, D2, D1 + D2)[mode]
    for T in range(1, int(D[any_f & (case["grid"] == TREE)].max()) + 2):
        p = clone(p0)
        p.heat0 = T - 0.5
        yield Probe(f"dousing W={w} R={R} mode={mode} sparse={sparse} T={T}", p, case, any_f & (D <= T - 1), False,
                    None, None)


def layers(h, w, R, seed, uniform=False, E=6):
    """One class v* of one layer has factor 1, its other classes 0, the other layer 1 throughout: a probed TREE burns
    iff clip(layer, 1, 5) == v*. Both layers, v* = 1..5. uniform: the layer's uniform value sweeps 0..7."""
    for axis in ("veg", "den"):
        for vs in range(1, 6):
            p0 = _params(h, R, seed=seed)
            _set_winds(p0, [[BIG] * 8] * 8)
            for i in range(6):
                hit = 1.0 if i == vs else 0.0
                p0.veg1p[i], p0.den1p[i] = (hit, 1.0) if axis == "veg" else (1.0, hit)
            for u in range(8) if uniform else (None,):
                p = clone(p0)
                vd = None if u is None else ((u, 3) if axis == "veg" else (3, u))
                # (uniform layers: every cell decides alike, half the envs do)
                case = state(E // 2 if uniform else E, h, w, seed, 0.3, uniform=_uniform(p, uniform, vd))
                any_f = nbr_fire(case["grid"]).any(axis=0)
                pred = any_f & (np.clip(case[axis], 1, 5) == vs)
                yield Probe(f"layers W={w} R={R} {axis} v*={vs} uniform={u}", p, case, pred, False, None, None)


def slopes(h, w, R, seed, E=3):
    """Edge values +-2^40 with random signs (1.0 where the edge's neighbour is outside the grid), winds 2^-30: a
    direction with factor 2^40 has p >= 1, the others p <= 2^-27 (q = 1 exactly). A probed TREE burns iff a FIRE
    neighbour lies in a direction whose factor exceeds 1; the grid's border cells have factor 1 in every direction
    (get_slope's zero border) and never burn."""
    p = _params(h, R, seed=seed)
    _set_winds(p, [[2.0 ** -30] * 8] * 8)
    case = state(E, h, w, seed, 0.3)
    rng = np.random.default_rng(seed + 7)
    sign = np.where(rng.random((E, 4, h, w)) < 0.5, -1.0, 1.0).astype(np.float32)
    for k, (dr, dc) in enumerate(edge_slope.OFF):  # no edge where the neighbour is outside the grid
        valid = shift(np.ones((h, w), np.float32), dr, dc)
        sign[:, k] *= valid
    s9 = edge_slope.slope9_from_edge(sign)  # -1 / 0 / +1 per direction, the border and the centre 0
    s8 = np.stack([s9[:, :, :, DR[d] + 1, DC[d] + 1] for d in range(8)], axis=1)
    edge = np.where(sign == 0, np.float32(1), sign * np.float32(2.0 ** 40)).astype(np.float32)
    planes = np.where(s8 > 0, np.float32(2.0 ** 40), np.where(s8 < 0, np.float32(2.0 ** -40), np.float32(1)))
    nb = nbr_fire(case["grid"])
    pred = (nb & (s8 > 0).transpose(1, 0, 2, 3)).any(axis=0)
    return Probe(f"slopes W={w} R={R}", p, case, pred, False, edge, planes.astype(np.float32))


def tiled_probes(h, w, R):
    """One sweep of every probe at one shape (shared with the GPU test of the tiled kernels)."""
    yield direction(h, w, R, SEED + 1)
    yield direction(h, w, R, SEED + 1, grow=True)
    for k in sorted({1, R}):
        yield from heat_ring(h, w, R, k, SEED + 1)
    for mode in range(3):
        yield from dousing(h, w, R, mode, False, SEED + 1)
    yield from layers(h, w, R, SEED + 1)
    yield slopes(h, w, R, SEED + 1)


# ---------------------------------------------------------------------------------------------- coverage conditions
def edge_lane_columns(w):
    """Columns of lanes 0, 1, 62 and 63 (4 cells each) of every 256-column segment."""
    return [s + c for s in range(0, w, 256) for c in (*range(0, 8), *range(248, 256)) if s + c < w]


def both_outcomes(pr):
    """Per column and per row: does the probe hold a probed TREE that must burn, and one that must not? Returns
    (burn_cols, keep_cols, burn_rows, keep_rows) as boolean vectors over the columns / rows."""
    pb = probed(pr)
    b, k = pb & pr.pred, pb & ~pr.pred
    return b.any(axis=(0, 1)), k.any(axis=(0, 1)), b.any(axis=(0, 2)), k.any(axis=(0, 2))
