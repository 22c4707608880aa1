"""The saturated-probability probes of tests/_alex_probe_ref.py on the CPU: for every probe the GPU test runs, the C
oracle (oracle.alex_c.alex_step) equals the numpy reference -- grid, ages and counts -- and its output is the same for
two different rng_step values (the saturation argument: no draw can move a probed cell). The coverage conditions --
conditions on the inputs, computed from the reference alone -- are asserted here, so that the GPU test's shapes, seeds
and densities are known to put both outcomes of every probe in every column the kernels treat differently."""
import numpy as np
import pytest

import _alex_probe_ref as pr
from oracle import alex_c

SEED = pr.SEED


def _oracle_equals_reference(probe):
    E, H, W = probe.case["grid"].shape
    c = probe.case
    planes = probe.planes if probe.planes is not None else np.ones((E, 8, H, W), np.float32)
    want = pr.expected(probe)
    for step in (3, 1000003):
        got = alex_c.alex_step(probe.p, c["grid"], c["age"], c["veg"], c["den"], c["dous"], planes, c["widx"],
                               rng_step=np.full(E, step, np.uint32))
        for name, g, w in zip(("grid", "ages", "counts"), got, want):
            assert np.array_equal(g, w), f"{probe.label} rng_step={step} {name}: {np.argwhere(g != w)[:5]}"
    return int(pr.probed(probe).sum())


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("W,R", pr.WIDTHS)
def test_direction_and_growth_probes(W, R, uniform):
    """Oracle = reference. Coverage: for every direction, every column and every row hold a probed TREE of that
    direction's env that must burn and one that must not -- except that no TREE of the first / last column or row can
    burn from a neighbour outside the grid: there only the cells that must not burn exist (the zero border). One
    env per direction leaves a column 32 cells, too few for every column to hold both: the probe runs on
    len(DIR_SEEDS) states (one launch of E = 9 each) and the condition is on their union."""
    probes = [pr.direction(pr.H, W, R, s, uniform=uniform, grow=grow) for s in pr.DIR_SEEDS for grow in (False, True)]
    for probe in probes:
        _oracle_equals_reference(probe)
    pb = np.concatenate([pr.probed(q) for q in probes[::2]], axis=1)  # the states stacked along the rows
    pred = np.concatenate([q.pred for q in probes[::2]], axis=1)
    fold = lambda x: x.reshape(len(pr.DIR_SEEDS), pr.H, W).any(axis=0)
    for d in range(8):
        burn, keep = fold(pb[d] & pred[d]), fold(pb[d] & ~pred[d])
        cols = np.ones(W, bool)
        rows = np.ones(pr.H, bool)
        if pr.DC[d]:
            cols[0 if pr.DC[d] < 0 else W - 1] = False
        if pr.DR[d]:
            rows[0 if pr.DR[d] < 0 else pr.H - 1] = False
        assert np.array_equal(burn.any(axis=0), cols), (d, np.flatnonzero(burn.any(axis=0) != cols)[:5])
        assert np.array_equal(burn.any(axis=1), rows), d
        assert keep.any(axis=0).all() and keep.any(axis=1).all(), d
    assert fold(pb[8] & pred[8]).any(axis=0).all() and (probe.case["grid"] == pr.EMPTY).any(axis=(0, 1)).all()


HEAT_CASES = (("general", 256), ("uniform", 256), ("flat", 256), ("flat", 512), ("flat", 1024))


@pytest.mark.parametrize("mode,W,R", [(m, W, R) for m, W in HEAT_CASES for R in sorted({R for R, _ in pr.heat_plan(m, W)})])
def test_heat_ring_probes(mode, W, R):
    """Oracle = reference for every (k, T) of the plan at radius R (the reference does not read the layers: the
    uniform-layer states run at W = 256 only). Coverage: for every k and every column, the sweep over T holds a probed
    cell on each side of the threshold, and every T of the sweep but the last burns some cell."""
    ks = [k for r, k in pr.heat_plan(mode, W) if r == R]
    assert ks == (list(range(1, R + 1)) if W == 256 and mode != "flat" else sorted({1, R}))
    for k in ks:
        sweep = list(pr.heat_ring(pr.H, W, R, k, SEED, uniform=mode == "uniform"))
        burn, keep = np.zeros(W, bool), np.zeros(W, bool)
        for probe in sweep:
            _oracle_equals_reference(probe)
            b, kp, _, _ = pr.both_outcomes(probe)
            burn |= b
            keep |= kp
            assert b.any() or probe is sweep[-1], probe.label
        assert burn.all() and keep.all(), (R, k, np.flatnonzero(~(burn & keep))[:5])
        assert len(sweep) >= 4


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("W,R", pr.WIDTHS)
def test_dousing_probes(W, R, sparse):
    """Oracle = reference for the three weight pairs and every T. Coverage, dense field: for every weight pair and
    every column, the sweep holds a probed cell on each side of the threshold. Sparse field: the same in the two
    columns on either side of every segment boundary and in rows 0, 15, 16 and H - 1; and some wave-row (4-cell
    groups of 64 lanes: a row of a 256-column segment) sees no doused cell in its 5 x 5 windows while another does."""
    for mode in range(3):
        burn, keep = np.zeros(W, bool), np.zeros(W, bool)
        brow, krow = np.zeros(pr.H, bool), np.zeros(pr.H, bool)
        for probe in pr.dousing(pr.H, W, R, mode, sparse, SEED):
            _oracle_equals_reference(probe)
            b, kp, br, kr = pr.both_outcomes(probe)
            burn, keep, brow, krow = burn | b, keep | kp, brow | br, krow | kr
        if not sparse:
            assert burn.all() and keep.all() and brow.all() and krow.all(), mode
        else:
            cols = [c for b in range(256, W, 256) for c in (b - 2, b - 1, b, b + 1)]
            assert burn[cols].all() and keep[cols].all(), mode
            rows = [0, 15, 16, pr.H - 1]
            assert brow[rows].all() and krow[rows].all(), mode
    if sparse:
        near = pr.box(probe.case["dous"], 2) > 0
        wave_rows = near.reshape(near.shape[0], pr.H, W // 256, 256).any(axis=-1)
        assert wave_rows.any() and not wave_rows.all()


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("W,R", pr.WIDTHS)
def test_layer_probes(W, R, uniform):
    """Oracle = reference for both layers and every class. Coverage (per-cell layers): for every class of either
    layer, both outcomes occur in every column of lanes 0, 1, 62 and 63 of every segment. Uniform layers: every class
    is hit by some uniform value and missed by another."""
    cols = pr.edge_lane_columns(W)
    hits = {}
    for probe in pr.layers(pr.H, W, R, SEED, uniform=uniform):
        _oracle_equals_reference(probe)
        b, kp, _, _ = pr.both_outcomes(probe)
        if uniform:
            key = probe.label.split(" uniform=")[0]
            hits.setdefault(key, set()).add(bool(b.any()))
        else:
            assert b[cols].all() and kp[cols].all(), (probe.label, np.flatnonzero(~(b & kp))[:5])
    assert all(v == {False, True} for v in hits.values())


@pytest.mark.parametrize("W,R", pr.WIDTHS)
def test_slope_probe(W, R):
    """Oracle (on the direction factors) = reference. Coverage: both outcomes in every column of lanes 0, 1, 62 and 63
    of every segment and in every row -- except the grid's border columns and rows, whose cells have factor 1 in every
    direction and hold only cells that must not burn."""
    probe = pr.slopes(pr.H, W, R, SEED)
    _oracle_equals_reference(probe)
    b, kp, br, kr = pr.both_outcomes(probe)
    cols = np.array(pr.edge_lane_columns(W))
    inner = cols[(cols > 0) & (cols < W - 1)]
    assert b[inner].all() and kp[cols].all()
    assert not b[0] and not b[W - 1] and not br[0] and not br[-1]
    assert br[1:-1].all() and kr.all()
    # the edge values and the direction factors say the same: own factor V (> 0) or 1 / |V|
    own, _ = alex_c.factor_pairs(probe.edge)
    assert np.array_equal(own[:, 1, 1:-1, 1:-1], probe.planes[:, 1, 1:-1, 1:-1])


@pytest.mark.parametrize("H,W,R", [(37, 45, 4), (32, 256, 6)])
def test_tiled_kernel_probe_shapes(H, W, R):
    """The shapes the tiled kernels' probes run (the odd shape: the bounds-checked path and partial draw groups):
    oracle = reference for one sweep of every probe; each probe decides both ways."""
    n = 0
    for probe in pr.tiled_probes(H, W, R):
        n += _oracle_equals_reference(probe)
        pb = pr.probed(probe)
        both = (pb & probe.pred).any() and (pb & ~probe.pred).any()
        assert both or " T=" in probe.label or "uniform" in probe.label, probe.label
    assert n > 10000
