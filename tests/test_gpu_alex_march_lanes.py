"""The flat-terrain marching step's lane-level plumbing (gca_alex_march.hip): burning-neighbour masks held as 64-bit
lane masks (cells of one lane, cells across a lane boundary, lanes 0 and 63 at the grid's border), the vertical sums
rebuilt per row from the fire ring (first and last ring rows of a tile, the tile boundary). The flat step
(edge_slope = NULL, with the layer bytes and with vd = NULL) against the tiled kernel (gca_alex_step_packed) on all-ones
planes: grid, ages and counts bytewise. E = 2, H = 32 (two tiles: one tile boundary, both grid borders), W = 256."""
import numpy as np
import pytest

from alex_cases import make_case
from test_gpu_alex_march import _coalesced, _layers, _run, _with_radius
from test_gpu_edge_slope import params

pytestmark = pytest.mark.gpu

E, H, W = 2, 32, 256
EDGE_COLS = (0, 1, 3, 4, 7, 8, 247, 248, 251, 252, 254, 255)
EDGE_ROWS = (0, 1, 14, 15, 16, 17, 30, 31)
VEG, DEN = 4, 2


def _uniform(case):
    case["veg"][...] = VEG
    case["den"][...] = DEN
    return case


def _edge_case(seed):
    """FIRE only on the lane- and tile-edge columns and rows, TREE everywhere else, no dousing."""
    case = _uniform(make_case(E, H, W, seed, p_tree=0.0, dousing_p=0.0, fire_p=0.0))
    g = np.ones((E, H, W), np.uint8)
    g[np.ix_(range(E), EDGE_ROWS, EDGE_COLS)] = 2
    case["grid"] = g
    rng = np.random.default_rng(seed)
    case["age"] = np.where(g == 2, rng.integers(1, 5, g.shape), 0).astype(np.int16)  # some burn out in a step
    return case


def _dense_case(seed):
    """The bench's mix (0.1 EMPTY, 0.8 TREE, 0.1 FIRE, iid) with a few doused cells."""
    case = _uniform(make_case(E, H, W, seed, p_tree=0.0, dousing_p=0.0, fire_p=0.1))
    d = case["dous"]
    d[0, 5, 17] = d[0, 15, 255] = d[1, 16, 0] = d[1, 31, 130] = 1
    return case


def _check_steps(device, case, R, steps, seed):
    import torch

    p = _with_radius(params(H, 0.0, seed=seed), R)
    p.vd_uniform = VEG | DEN << 4
    ones = _coalesced(device, torch.ones((E, 4, H, W), dtype=torch.float32, device=device))
    vd, bits = _layers(device, case)
    assert bool((vd == p.vd_uniform).all())
    multi = False
    for s in range(steps):
        rs = np.full(E, 5 * s + 3, np.uint32)
        ref = _run(device, "gca_alex_step_packed", p, case, ones, rs, vd, bits)
        # an all-quiet case would pass for nothing
        assert (ref[0] != case["grid"]).any() and (ref[1] != case["age"]).any(), s
        new_fire = (ref[0] == 2) & (case["grid"] == 1)
        multi = multi or bool((new_fire.reshape(E, H, W // 4, 4).sum(-1) >= 2).any())
        for name, layers in (("flat", vd), ("flat + uniform", None)):
            got = _run(device, "gca_alex_step_march", p, case, None, rs, layers, bits)
            for k, what in enumerate(("grid", "ages", "counts")):
                assert np.array_equal(got[k], ref[k]), (name, R, s, what, np.argwhere(got[k] != ref[k])[:5])
        case["grid"], case["age"] = ref[0], ref[1]
    return multi


@pytest.mark.parametrize("R", [2, 6])
def test_fires_at_lane_and_tile_edges(device, R):
    """Case (a): lane 0 / lane 63 borders, every cell-to-lane boundary in both column directions, the first and last
    ring rows of both tiles."""
    _check_steps(device, _edge_case(11 + R), R, 1, seed=31 + R)


@pytest.mark.parametrize("R", [2, 6])
def test_dense_state(device, R):
    """Case (b): lanes with two or more new fires (the second draw block) and the dousing branch taken."""
    case = _dense_case(17 + R)
    assert _check_steps(device, case, R, 1, seed=37 + R), "no lane with two new fires: the case checks less than it says"


@pytest.mark.parametrize("R", [2, 6])
def test_two_steps_in_a_row(device, R):
    """Case (c): case (a) stepped twice; the second launch starts from whatever the first left in LDS."""
    _check_steps(device, _edge_case(23 + R), R, 2, seed=43 + R)
