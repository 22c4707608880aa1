"""GPU: gca_windy_step, gca_windy_dirmask and gca_bulldozer_pre / _interpass / _post through raw C-ABI calls on device
tensors, every env compared exactly with the numpy restatement of their contracts in tests/_windy_ref.py (scipy
convolve2d and the thresholds, oracle.philox; held to the golden vectors and to oracle.windy.BulldozerOracle by
tests/test_windy_ref_cpu.py). Never device against device. The cases and the conditions each one asserts are built in
_windy_ref.py; the letters are those of its builders:

  A  all 256 direction masks, dense and one-cause sparse grids, every kernel width, SWAR and exact
  B  the contract: per-env parity, the steps gate, counts accumulating / NULL, untouched bytes
  C  cell codes other than (0, 3, 25), codes with the high bit, empty != 0 and arbitrary bytes on the exact kernel
  D  heights around the strips (H = 1 .. 65)      E  the fallbacks to the exact kernel
  L  the strip march of windy_fast_kernel (nT >= 2), reached only through the batch size
"""
import numpy as np
import pytest

import _windy_ref as wr

pytestmark = pytest.mark.gpu


def _t(x, device):
    import torch

    x = np.ascontiguousarray(x)
    if x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.as_tensor(x).to(device).contiguous()


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a if dtype is None else a.view(dtype)


def _run_step(device, case, force_exact=0, byte_offset=0):
    """One gca_windy_step call on the case's inputs; returns the device's (buf0, buf1, counts). byte_offset: both
    buffers are slices of larger tensors, that many bytes past their (256-B aligned) starts."""
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    E, H, W = case["E"], case["H"], case["W"]
    n = E * H * W
    bufs, keep = [], []
    for b in (case["buf0"], case["buf1"]):
        big = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=device)
        view = big[byte_offset:byte_offset + n]
        view.copy_(_t(b.reshape(-1), device))
        assert view.data_ptr() % 16 == byte_offset % 16
        bufs.append(view)
        keep.append(big)
    # every operand stays referenced until the kernel has run (a temporary's memory may be reused at once)
    par = None if case["parity"] is None else _t(case["parity"], device)
    steps = None if case["steps"] is None else _t(case["steps"], device)
    masks = _t(case["masks"], device)
    counts = None if case["counts0"] is None else _t(case["counts0"], device)
    call("gca_windy_step", dev.ptr(bufs[0]), dev.ptr(bufs[1]), dev.ptr(par), dev.ptr(steps), case["pass_"],
         dev.ptr(masks), E, H, W, *case["codes"], force_exact, dev.ptr(counts), dev.stream_ptr())
    torch.cuda.synchronize(device)
    for big in keep:  # nothing outside the slices was written
        assert bool((big[:byte_offset] == 0xEE).all()) and bool((big[byte_offset + n:] == 0xEE).all())
    return (_np(bufs[0]).reshape(E, H, W), _np(bufs[1]).reshape(E, H, W), None if counts is None else _np(counts))


def _name_cells(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} cells differ, first (env, row, col) {bad[:6].tolist()}"


def _check_step(device, case, force_exact=0, byte_offset=0):
    b0, b1, cnt = _run_step(device, case, force_exact, byte_offset)
    assert np.array_equal(b0, case["want_buf0"]), "buf0: " + _name_cells(b0, case["want_buf0"])
    assert np.array_equal(b1, case["want_buf1"]), "buf1: " + _name_cells(b1, case["want_buf1"])
    if case["want_counts"] is None:
        assert cnt is None
    else:
        assert np.array_equal(cnt, case["want_counts"]), np.argwhere(cnt != case["want_counts"])[:6].tolist()


# ===================================================================== gca_windy_step
SIZES_A = [(20, 16), (20, 32), (20, 64), (20, 128), (7, 1024), (20, 256), (20, 512)]


@pytest.mark.parametrize("force_exact", [0, 1])
@pytest.mark.parametrize("fill", ["dense", "sparse"])
@pytest.mark.parametrize("H,W", SIZES_A)
def test_a_all_256_masks(device, H, W, fill, force_exact):
    _check_step(device, wr.case_all_masks(H, W, fill), force_exact)


@pytest.mark.parametrize("with_counts", [True, False])
@pytest.mark.parametrize("pass_", [0, 1, 2])
@pytest.mark.parametrize("H,W", [(45, 64), (45, 256), (45, 512), (45, 40)])
def test_b_contract_parity_gate_counts(device, H, W, pass_, with_counts):
    _check_step(device, wr.case_contract(H, W, pass_, with_counts))


@pytest.mark.parametrize("H,W,force_exact", [(20, 64, 0), (20, 256, 0), (20, 512, 0), (20, 64, 1)])
@pytest.mark.parametrize("codes", [(0, 2, 9), (0, 127, 128), (0, 200, 255), (0, 20, 200)])
def test_c_codes_with_empty_zero(device, codes, H, W, force_exact):
    """Codes with the high bit and codes one apart on the byte compares of all three kernels. Grids of domino_fill,
    on which the SWAR kernels' closed-form rule is the thresholds for any empty = 0 < tree < fire; (0, 20, 200), which
    satisfies the reference constructor's inequalities, also on a dense grid."""
    _check_step(device, wr.case_codes(H, W, codes, "domino"), force_exact)
    if wr.closed_form_is_exact(codes):
        _check_step(device, wr.case_codes(H, W, codes, "dense"), force_exact)


@pytest.mark.parametrize("H,W", [(20, 64), (19, 17)])
@pytest.mark.parametrize("codes,fill", [((1, 3, 25), "bytes"), ((2, 7, 200), "bytes"), ((0, 2, 9), "dense"),
                                        ((0, 127, 128), "dense"), ((0, 200, 255), "dense"), ((0, 2, 9), "bytes")])
def test_c_exact_kernel_any_bytes_any_codes(device, codes, fill, H, W):
    """The exact kernel is the thresholds themselves: empty != 0 with cells from all 256 byte values, and dense grids
    of the codes on which the closed-form rule is not the thresholds."""
    _check_step(device, wr.case_codes(H, W, codes, fill), 1)
    if codes[0] != 0:
        _check_step(device, wr.case_codes(H, W, codes, fill), 0)  # empty != 0 never takes a SWAR kernel


HEIGHTS = [(H, W) for W in (256, 512) for H in (1, 2, 15, 16, 17, 63, 64, 65)] + \
          [(H, W) for W in (64, 1024) for H in (1, 2, 3, 17)]


@pytest.mark.parametrize("H,W", HEIGHTS)
def test_d_heights(device, H, W):
    _check_step(device, wr.case_shape(5, H, W))


@pytest.mark.parametrize("H,W,byte_offset", [(9, 17, 0), (9, 48, 0), (5, 2048, 0), (9, 64, 4)])
def test_e_fallbacks_to_the_exact_kernel(device, H, W, byte_offset):
    _check_step(device, wr.case_shape(3, H, W, seed=1), 0, byte_offset)


@pytest.mark.parametrize("E,H,W", sorted(wr.MARCH_CASES))
def test_l_strip_march(device, E, H, W):
    _check_step(device, wr.case_march(E, H, W))


# ===================================================================== gca_windy_dirmask
DM_E, DM_OFFSET, DM_SEED = 600, 100, 0x5EED0123456789


def _dirmask_inputs(wind_stride):
    rng = np.random.default_rng(wind_stride)
    wind = rng.random(max(wind_stride, 1) * (DM_E - 1) + 9) if wind_stride else rng.random(9)
    rs = rng.integers(0, 2**32, DM_E, dtype=np.uint64).astype(np.uint32)
    rs[:2] = (2**32 - 1, 2**32 - 2)
    assert len(set(rs.tolist())) > DM_E - 5
    steps = rng.integers(-1, 4, DM_E).astype(np.int32)
    return wind, rs, steps


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("pass_", [0, 2])
@pytest.mark.parametrize("wind_stride", [0, 9, 12])
def test_dirmask_philox_per_env_step_pass_and_gate(device, wind_stride, pass_, gated):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    wind, rs, steps = _dirmask_inputs(wind_stride)
    steps = steps if gated else None
    prev = np.full(DM_E, 0xA5, np.uint8)
    want = wr.ref_dirmask(wind, wind_stride, None, DM_SEED, rs, steps, pass_, DM_OFFSET, prev)
    if gated:
        assert (steps > pass_).any() and (steps <= pass_).any() and np.all(want[steps <= pass_] == 0xA5)
    w_d, r_d, m_d = _t(wind, device), _t(rs, device), _t(prev, device)
    s_d = None if steps is None else _t(steps, device)
    call("gca_windy_dirmask", dev.ptr(w_d), wind_stride, None, DM_SEED, dev.ptr(r_d), dev.ptr(s_d), pass_, DM_OFFSET,
         dev.ptr(m_d), DM_E, dev.stream_ptr())
    torch.cuda.synchronize(device)
    got = _np(m_d)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8].tolist()
    assert np.array_equal(_np(r_d, np.uint32), rs) and np.array_equal(_np(w_d), wind)
    if wind_stride == 0:  # rng_step = NULL draws step `pass_` for every env
        call("gca_windy_dirmask", dev.ptr(w_d), 0, None, DM_SEED, None, dev.ptr(s_d), pass_, DM_OFFSET, dev.ptr(m_d),
             DM_E, dev.stream_ptr())
        torch.cuda.synchronize(device)
        assert np.array_equal(_np(m_d), wr.ref_dirmask(wind, 0, None, DM_SEED, None, steps, pass_, DM_OFFSET, want))


@pytest.mark.parametrize("wind_stride", [0, 9, 12])
def test_dirmask_injected_rolls_and_strict_ties(device, wind_stride):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    wind, _, steps = _dirmask_inputs(wind_stride)
    rng = np.random.default_rng(5)
    roll = rng.random((DM_E, 9))
    rows = wr.wind_rows(wind, wind_stride, DM_E)
    tie = rng.random((DM_E, 9)) < 0.3
    roll[tie] = rows[tie]
    prev = np.full(DM_E, 0x5A, np.uint8)
    want = wr.ref_dirmask(wind, wind_stride, roll, DM_SEED, None, steps, 1, DM_OFFSET, prev)
    on = steps > 1
    for d, idx in enumerate(wr.DIRS):  # roll < wind is strict: a tie leaves the bit clear
        assert np.all(((want[on] >> d) & 1)[tie[on][:, idx]] == 0) and tie[on][:, idx].any()
    w_d, ro_d, s_d, m_d = _t(wind, device), _t(roll, device), _t(steps, device), _t(prev, device)
    call("gca_windy_dirmask", dev.ptr(w_d), wind_stride, dev.ptr(ro_d), DM_SEED, None, dev.ptr(s_d), 1, DM_OFFSET,
         dev.ptr(m_d), DM_E, dev.stream_ptr())
    torch.cuda.synchronize(device)
    got = _np(m_d)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8].tolist()


# ===================================================================== the three per-env kernels, each alone
def _c_params(p):
    from gymca_amd.forest_fire.operators.move_modify import make_params

    c = make_params(p.sets, p.effects)
    for k in range(9):
        c.t_move[k] = p.t_move[k]
    c.t_shoot[0], c.t_shoot[1], c.t_any = p.t_shoot[0], p.t_shoot[1], p.t_any
    c.seed, c.env_offset = p.seed, p.env_offset
    c.empty, c.tree, c.fire = p.codes
    return c


def _same(got, want):
    return got.dtype == want.dtype and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def test_bulldozer_pre_alone(device):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    k = wr.case_kernels()
    p, E = k["p"], k["E"]
    want = wr.ref_pre(p, k["action"], k["accu"], k["steps0"], k["done"], k["wind"], 9, k["rng_step"], k["dir_mask"],
                      k["counts"])
    cp = _c_params(p)
    d = {n: _t(k[n], device) for n in ("action", "accu", "steps0", "done", "wind", "rng_step", "dir_mask", "counts")}
    call("gca_bulldozer_pre", cp, dev.ptr(d["action"]), dev.ptr(d["accu"]), dev.ptr(d["steps0"]), dev.ptr(d["done"]),
         dev.ptr(d["wind"]), 9, dev.ptr(d["rng_step"]), dev.ptr(d["dir_mask"]), dev.ptr(d["counts"]), E,
         dev.stream_ptr())
    torch.cuda.synchronize(device)
    for name, w in zip(("accu", "steps0", "dir_mask", "counts"), want):
        assert _same(_np(d[name]), w), (name, np.argwhere(_np(d[name]) != w)[:6].tolist())
    for name in ("action", "done", "wind"):
        assert _same(_np(d[name]), k[name]), name
    assert np.array_equal(_np(d["rng_step"], np.uint32), k["rng_step"])
    # done = NULL: every env is live
    d2 = {n: _t(k[n], device) for n in ("accu", "steps0", "dir_mask", "counts")}
    want = wr.ref_pre(p, k["action"], k["accu"], k["steps0"], None, k["wind"], 9, k["rng_step"], k["dir_mask"],
                      k["counts"])
    call("gca_bulldozer_pre", cp, dev.ptr(d["action"]), dev.ptr(d2["accu"]), dev.ptr(d2["steps0"]), None,
         dev.ptr(d["wind"]), 9, dev.ptr(d["rng_step"]), dev.ptr(d2["dir_mask"]), dev.ptr(d2["counts"]), E,
         dev.stream_ptr())
    torch.cuda.synchronize(device)
    for name, w in zip(("accu", "steps0", "dir_mask", "counts"), want):
        assert _same(_np(d2[name]), w), ("done = NULL", name)


@pytest.mark.parametrize("pass_", [0, 1])
def test_bulldozer_interpass_alone(device, pass_):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    k = wr.case_kernels()
    p, E = k["p"], k["E"]
    assert (k["steps"] > pass_ + 1).any() and (k["steps"] == pass_ + 1).any() and (k["steps"] <= pass_).any()
    want = wr.ref_interpass(p, pass_, k["steps"], k["parity"], k["wind"], 9, k["rng_step"], k["dir_mask"], k["counts"])
    cp = _c_params(p)
    d = {n: _t(k[n], device) for n in ("steps", "parity", "wind", "rng_step", "dir_mask", "counts")}
    call("gca_bulldozer_interpass", cp, pass_, dev.ptr(d["steps"]), dev.ptr(d["parity"]), dev.ptr(d["wind"]), 9,
         dev.ptr(d["rng_step"]), dev.ptr(d["dir_mask"]), dev.ptr(d["counts"]), E, dev.stream_ptr())
    torch.cuda.synchronize(device)
    for name, w in zip(("parity", "dir_mask", "counts"), want):
        assert _same(_np(d[name]), w), (name, np.argwhere(_np(d[name]) != w)[:6].tolist())
    assert _same(_np(d["steps"]), k["steps"]) and _same(_np(d["wind"]), k["wind"])
    assert np.array_equal(_np(d["rng_step"], np.uint32), k["rng_step"])


POST_OUT = ("parity", "buf0", "buf1", "pos", "counts", "rng_step", "done", "hit", "reward")


@pytest.mark.parametrize("with_parity", [True, False])
def test_bulldozer_post_alone(device, with_parity):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    k = wr.case_kernels()
    p, E, H, W = k["p"], k["E"], k["H"], k["W"]
    parity = k["parity"] if with_parity else None
    want = wr.ref_post(p, 2, k["action"], k["steps"], parity, k["buf0"], k["buf1"], k["pos"], k["counts"],
                       k["rng_step"], k["done"], k["hit"], k["reward"])
    assert want["hit"].tolist().count(1) > 50 and np.isnan(want["reward"]).any() and (want["reward"] == 0).any()
    assert not np.array_equal(want["buf0"], k["buf0"]) and with_parity != np.array_equal(want["buf1"], k["buf1"])
    cp = _c_params(p)
    d = {n: _t(k[n], device) for n in POST_OUT + ("action", "steps")}
    call("gca_bulldozer_post", cp, 2, dev.ptr(d["action"]), dev.ptr(d["steps"]),
         dev.ptr(d["parity"]) if with_parity else None, dev.ptr(d["buf0"]), dev.ptr(d["buf1"]), H, W, dev.ptr(d["pos"]),
         dev.ptr(d["counts"]), dev.ptr(d["rng_step"]), dev.ptr(d["done"]), dev.ptr(d["hit"]), dev.ptr(d["reward"]), E,
         dev.stream_ptr())
    torch.cuda.synchronize(device)
    for name in POST_OUT:
        w = k["parity"] if (name == "parity" and not with_parity) else want[name]
        got = _np(d[name], np.uint32) if name == "rng_step" else _np(d[name])
        assert _same(got, w), (name, np.argwhere(got != w)[:6].tolist())
    assert _same(_np(d["action"]), k["action"]) and _same(_np(d["steps"]), k["steps"])


# ===================================================================== the whole three-kernel sequence
SEQ_STATE = ("buf0", "buf1", "parity", "accu", "steps", "counts", "pos", "hit", "reward", "done", "rng_step")


@pytest.mark.parametrize("H,W", [(20, 64), (20, 256)])
def test_three_kernel_sequence_against_the_reference(device, H, W):
    """pre, the passes (windy_step, interpass between consecutive passes) and post as batched.py chains them, through
    the raw ABI: E = 300, 6 env steps of up to 3 passes, every state array compared after every step."""
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    E = 300
    p, P, ref, actions, wind = wr.case_sequence(E, H, W)
    cp = _c_params(p)
    d = {n: _t(ref[n], device) for n in SEQ_STATE + ("dir_mask",)}
    w_d = _t(wind, device)
    st = dev.stream_ptr()
    seen = set()
    for k in range(len(actions)):
        ref = wr.ref_env_step(p, P, ref, actions[k], wind, 9)
        a_d = _t(actions[k], device)
        call("gca_bulldozer_pre", cp, dev.ptr(a_d), dev.ptr(d["accu"]), dev.ptr(d["steps"]), dev.ptr(d["done"]),
             dev.ptr(w_d), 9, dev.ptr(d["rng_step"]), dev.ptr(d["dir_mask"]), dev.ptr(d["counts"]), E, st)
        for pss in range(P):
            call("gca_windy_step", dev.ptr(d["buf0"]), dev.ptr(d["buf1"]), dev.ptr(d["parity"]), dev.ptr(d["steps"]),
                 pss, dev.ptr(d["dir_mask"]), E, H, W, *p.codes, 0, dev.ptr(d["counts"]), st)
            if pss < P - 1:
                call("gca_bulldozer_interpass", cp, pss, dev.ptr(d["steps"]), dev.ptr(d["parity"]), dev.ptr(w_d), 9,
                     dev.ptr(d["rng_step"]), dev.ptr(d["dir_mask"]), dev.ptr(d["counts"]), E, st)
        call("gca_bulldozer_post", cp, P - 1, dev.ptr(a_d), dev.ptr(d["steps"]), dev.ptr(d["parity"]),
             dev.ptr(d["buf0"]), dev.ptr(d["buf1"]), H, W, dev.ptr(d["pos"]), dev.ptr(d["counts"]),
             dev.ptr(d["rng_step"]), dev.ptr(d["done"]), dev.ptr(d["hit"]), dev.ptr(d["reward"]), E, st)
        torch.cuda.synchronize(device)
        for name in SEQ_STATE:
            got = _np(d[name], np.uint32) if name == "rng_step" else _np(d[name])
            assert _same(got, ref[name]), (f"step {k}", name, np.argwhere(got != ref[name])[:6].tolist())
        seen.update(ref["steps"].tolist())
    assert {-1, 0, 1, 2, 3} <= seen and 0 < ref["done"].sum() < E and ref["counts"][:, 2].max() > 0
