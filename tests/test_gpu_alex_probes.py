"""Draw-free probes of the Alexandridis kernels (tests/_alex_probe_ref.py): parameters under which every burn
probability is saturated (>= 1) or zero, so that one step is a pure integer function of the neighbourhood and the
expected grid, ages and counts come from a few lines of numpy -- no float arithmetic, no oracle, no draw. A wrong
neighbour, mask byte, lane shift, halo slot, wind pairing or layer byte fails on the first cell it touches, and the
message names the probe (direction / ring / threshold), env, row and column.

The marching step (gca_alex_step_march) runs every probe in its three terrain modes -- edge_slope given ("general":
real slopes from an altitude field, whose factors in [1/1121, 1121] move no saturated or zero probability),
edge_slope = NULL ("flat"), and vd = NULL as well ("uniform") -- at H = 32 (two tiles) and W = 256 / 512 / 1024
(NSEG = 1 / 2 / 4); the fused-frame instances run the direction probe; the tiled kernels (gca_alex_step_packed,
gca_alex_step_es, and gca_alex_step at 37 x 45: the bounds-checked path, partial draw groups) one sweep of each.
tests/test_alex_probes_cpu.py pins the same probes against the C oracle and asserts their coverage conditions."""
import numpy as np
import pytest

import _alex_probe_ref as pr
from test_gpu_alex_march import _coalesced, _layers, _run
from test_gpu_edge_slope import _t, altitude, slopes, step

pytestmark = pytest.mark.gpu

MODES = ("general", "flat", "uniform")
RS = 12345  # any value: no probed cell's outcome depends on a draw


def _diff(probe, got, want):
    for name, g, w in zip(("grid", "ages", "counts"), got, want):
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)
            i = tuple(int(x) for x in at[0])
            return f"{probe.label}: {name} differ at {len(at)} places, first (env, row, col) = {i}: got {g[i]}, want {w[i]}"
    return None


class Runner:
    """Device copies of a probe's state (shared by the probes of a sweep) and one step through the marching kernel."""

    def __init__(self, device, mode, fn="gca_alex_step_march", rgb=None):
        self.device, self.mode, self.fn, self.rgb = device, mode, fn, rgb
        self.key = None

    def _state(self, probe):
        key = (id(probe.case["grid"]), id(probe.case["veg"]), id(probe.case["dous"]), id(probe.edge))
        if key != self.key:
            import torch

            E, H, W = probe.case["grid"].shape
            self.case = {k: np.array(v) for k, v in probe.case.items()}
            self.vd, self.bits = _layers(self.device, self.case)
            self.es = None
            if self.mode == "general":
                if probe.edge is not None:
                    self.es = _t(probe.edge, torch.float32, self.device)
                else:
                    self.es, _ = slopes(self.device, altitude(E, H, W, 5))
            self.key = key
        self.case["widx"] = np.array(probe.case["widx"])

    def check(self, probe):
        self._state(probe)
        E = probe.case["grid"].shape[0]
        got = _run(self.device, self.fn, probe.p, self.case, self.es, np.full(E, RS, np.uint32),
                   None if self.mode == "uniform" else self.vd, self.bits, rgb=self.rgb)
        msg = _diff(probe, got[:3], pr.expected(probe))
        assert msg is None, f"[{self.fn} {self.mode}] {msg}"
        return got


def _frame_args(device, E):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call
    from gymca_amd.forest_fire.bulldozer.observation import make_obs_params

    col = torch.zeros((12, 4), dtype=torch.float32, device=device)
    call("gca_obs_color_table", make_obs_params(0, 1, 2, False, False, 8), dev.ptr(col), dev.stream_ptr())
    return col, torch.as_tensor(np.arange(E, dtype=np.int32) % 2, device=device)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,R", pr.WIDTHS)
def test_direction_and_growth_probe(device, mode, W, R):
    """Env d burns a TREE iff its neighbour in direction d is FIRE; env 8 iff any is; with p_tree = 1 every EMPTY cell
    grows (the GROW instances). Three states of E = 9."""
    run = Runner(device, mode)
    for seed in pr.DIR_SEEDS:
        for grow in (False, True):
            run.check(pr.direction(pr.H, W, R, seed, uniform=mode == "uniform", grow=grow))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("R", [1, 6])
def test_direction_probe_fused_frame(device, mode, R):
    """The fused-frame instances (gca_alex_step_march_rgb, W = 256) make the same decisions, with and without growth,
    and their frame is the frame of the expected grid (the colours of the new kinds and the pre-step dousing)."""
    run = Runner(device, mode, fn="gca_alex_step_march_rgb", rgb=_frame_args(device, 9))
    plain = Runner(device, mode)
    for grow in (False, True):
        probe = pr.direction(pr.H, 256, R, pr.DIR_SEEDS[0], uniform=mode == "uniform", grow=grow)
        frame = run.check(probe)[4]
        assert np.isfinite(frame).all() and (frame >= 0).all()
        plain.check(probe)
        # cells of one kind (and no dousing: the probe has none) in one env share one colour
        out = pr.expected(probe)[0]
        for e in (0, 1, 8):
            for kind in (pr.EMPTY, pr.TREE, pr.FIRE):
                px = frame[e][out[e] == kind]
                assert (px == px[0]).all(), (e, kind)


@pytest.mark.parametrize("mode,W,R", [(m, W, R) for m in MODES for W in (256, 512, 1024)
                                      for R in sorted({R for R, _ in pr.heat_plan(m, W)})])
def test_heat_ring_probe(device, mode, W, R):
    """heat = 0.5 - T + B_k with only ring k weighted: a probed TREE burns iff the FIRE count of its (2k+1)^2 box is
    >= T; T sweeps 1 .. max + 1. Every k <= R at W = 256 (general and uniform), k in {1, R} elsewhere."""
    run = Runner(device, mode)
    for k in [k for r, k in pr.heat_plan(mode, W) if r == R]:
        for probe in pr.heat_ring(pr.H, W, R, k, pr.SEED, uniform=mode == "uniform"):
            run.check(probe)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("W,R", pr.WIDTHS)
def test_dousing_probe(device, mode, sparse, W, R):
    """heat = T - 0.5 - (D_1 | D_2 | D_1 + D_2): a probed TREE burns iff that count of doused cells is <= T - 1. A
    dense field, and a sparse one on the segment boundaries and the tile / grid edge rows (wave-rows that skip the
    dousing term; the halo exchange of the dousing sums)."""
    run = Runner(device, mode)
    for dm in range(3):
        for probe in pr.dousing(pr.H, W, R, dm, sparse, pr.SEED, uniform=mode == "uniform"):
            run.check(probe)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,R", pr.WIDTHS)
def test_layer_probe(device, mode, W, R):
    """One class of one layer has factor 1 and the layer's other classes 0: a probed TREE burns iff its clipped
    vegetation (density) is that class; uniform: p.vd_uniform sweeps the values 0..7."""
    run = Runner(device, mode)
    for probe in pr.layers(pr.H, W, R, pr.SEED, uniform=mode == "uniform"):
        run.check(probe)


@pytest.mark.parametrize("W,R", pr.WIDTHS)
def test_slope_probe(device, W, R):
    """Edge values +-2^40, winds 2^-30: a probed TREE burns iff a FIRE neighbour lies in a direction whose slope factor
    exceeds 1; the grid's border cells (factor 1 whatever their edge values) never burn. The general instance."""
    Runner(device, "general").check(pr.slopes(pr.H, W, R, pr.SEED))


@pytest.mark.parametrize("fn,H,W,R", [("gca_alex_step_packed", 32, 256, 6), ("gca_alex_step_es", 37, 45, 4),
                                      ("gca_alex_step", 37, 45, 4)])
def test_tiled_kernels_run_the_probes(device, fn, H, W, R):
    """One sweep of every probe through the tiled kernels: the packed step, the edge-slope step and the 8-plane step
    (an odd shape: the bounds-checked path and partial draw groups). Slopes: all ones but for the slope probe."""
    import torch

    for probe in pr.tiled_probes(H, W, R):
        E = probe.case["grid"].shape[0]
        case = {k: np.array(v) for k, v in probe.case.items()}
        rs = np.full(E, RS, np.uint32)
        if fn == "gca_alex_step":
            planes = probe.planes if probe.planes is not None else np.ones((E, 8, H, W), np.float32)
            got = step(device, fn, probe.p, case, _t(planes, torch.float32, device), rng_step=rs)
        else:
            edge = probe.edge if probe.edge is not None else np.ones((E, 4, H, W), np.float32)
            es = _t(edge, torch.float32, device)
            if fn == "gca_alex_step_es":
                got = step(device, fn, probe.p, case, es, rng_step=rs)
            else:
                vd, bits = _layers(device, case)
                got = _run(device, fn, probe.p, case, _coalesced(device, es), rs, vd, bits)
        msg = _diff(probe, got[:3], pr.expected(probe))
        assert msg is None, f"[{fn}] {msg}"
