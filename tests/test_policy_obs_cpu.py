"""CPU: the policy observation of the batched envs (gca_policy_observation) in the host build of the C-ABI against its
numpy restatement (tests/_policy_obs_ref.py), bit for bit, and the restatement against torch's avg_pool2d of the
one-hot planes. No GPU."""
import numpy as np
import pytest

import _policy_obs_ref as ref

SHAPES = ref.SHAPES


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(buf, parity, pos, codes, r, B, **kw):
    cur = buf[0] if parity is None else ref.current(buf, parity)
    want_l, want_c = ref.ref(cur, pos, codes, r, B)
    got_l, got_c = ref.host_observe(buf, parity, pos, codes, r, B, **kw)
    assert _same_bits(got_l, want_l), "local"
    assert _same_bits(got_c, want_c), "coarse"
    return want_l, want_c


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_build_equals_the_restatement(shape, rot):
    E, H, W, B, r = shape
    buf, parity, pos = ref.make_case(E, H, W, B, rot=rot)
    assert 0 < parity.sum() < E
    local, coarse = _check(buf, parity, pos, ref.CODES, r, B)
    # env 0's first block is all FIRE, the last env's last block all TREE: exactly 1.0 where the block fits
    fit0 = min(B, H) * min(B, W) / (B * B)
    assert coarse[0, 1, 0, 0] == np.float32(fit0) and coarse[0, 0, 0, 0] == 0.0
    hl, wl = H - (coarse.shape[2] - 1) * B, W - (coarse.shape[3] - 1) * B
    assert coarse[E - 1, 0, -1, -1] == np.float32(hl * wl / (B * B)) and coarse[E - 1, 1, -1, -1] == 0.0
    if H >= B and W >= B:
        assert coarse[0, 1, 0, 0] == 1.0
    # the window's centre is the agent's own cell; a corner position pads two sides with class 3
    cur = ref.current(buf, parity)
    for e in range(E):
        v = cur[e, pos[e, 0], pos[e, 1]]
        assert local[e, r, r] == (1 if v == 3 else 2 if v == 25 else 0)
        if r and tuple(pos[e]) == (0, 0):
            assert (local[e, :r] == 3).all() and (local[e, :, :r] == 3).all()
        if r and tuple(pos[e]) == (H - 1, W - 1):
            assert (local[e, r + 1:] == 3).all() and (local[e, :, r + 1:] == 3).all()
    assert (local[cur[np.arange(E), pos[:, 0], pos[:, 1]] == ref.OTHER][:, r, r] == 0).all()


def test_every_corner_and_the_centre_are_covered():
    """The two rotations of the positions give each shape (0, 0), (H - 1, W - 1) and the centre."""
    for E, H, W, _, _ in SHAPES:
        seen = {tuple(p) for rot in (0, 1) for p in ref.positions(E, H, W, rot)}
        assert seen == {(0, 0), (H - 1, W - 1), (H // 2, W // 2)}


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[0]])
def test_helicopter_codes(shape):
    E, H, W, B, r = shape
    buf, parity, pos = ref.make_case(E, H, W, B, codes=ref.HELI_CODES, seed=3)
    _check(buf, parity, pos, ref.HELI_CODES, r, B)


@pytest.mark.parametrize("shape", SHAPES)
def test_null_parity_reads_buf0(shape):
    E, H, W, B, r = shape
    buf, _, pos = ref.make_case(E, H, W, B, seed=5, rot=2)
    _check(buf, None, pos, ref.CODES, r, B)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_form_is_validated_and_otherwise_ignored(form):
    E, H, W, B, r = SHAPES[0]
    buf, parity, pos = ref.make_case(E, H, W, B, seed=7)
    _check(buf, parity, pos, ref.CODES, r, B, form=form)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]])
def test_a_null_output_is_skipped(shape):
    E, H, W, B, r = shape
    buf, parity, pos = ref.make_case(E, H, W, B, seed=9)
    want_l, want_c = ref.ref(ref.current(buf, parity), pos, ref.CODES, r, B)
    lo, co = ref.host_observe(buf, parity, pos, ref.CODES, r, B, coarse=False)
    assert co is None and _same_bits(lo, want_l)
    lo, co = ref.host_observe(buf, parity, pos, ref.CODES, r, B, local=False)
    assert lo is None and _same_bits(co, want_c)


def test_positions_outside_the_grid_give_class_3_and_no_fault():
    """A position outside the grid is not an error of the call: the window is class 3 wherever it misses the grid
    (host build only; the device's window part has the guarded load as its only load)."""
    E, H, W, B, r = 6, 7, 9, 4, 2
    buf, _, _ = ref.make_case(E, H, W, B, seed=11)
    parity = np.zeros(E, np.uint8)
    far = np.iinfo(np.int32)
    pos = np.array([[-100, 4], [3, 1000], [far.min, far.min], [far.max, far.max], [-1, -1], [H, W]], np.int32)
    lo, co = ref.host_observe(buf, parity, pos, ref.CODES, r, B)
    assert (lo[:4] == 3).all()
    cls = lambda v: 1 if v == 3 else 2 if v == 25 else 0
    # (-1, -1): the window's last row / column pair (rows 0 .. 1, columns 0 .. 1) is inside; (H, W): the first pair
    assert (lo[4, :r + 1] == 3).all() and (lo[4, :, :r + 1] == 3).all()
    assert lo[4, r + 1, r + 1] == cls(buf[0, 4, 0, 0]) and lo[4, 2 * r, 2 * r] == cls(buf[0, 4, 1, 1])
    assert (lo[5, 2:] == 3).all() and (lo[5, :, 2:] == 3).all()
    assert lo[5, 0, 0] == cls(buf[0, 5, H - 2, W - 2]) and lo[5, 1, 1] == cls(buf[0, 5, H - 1, W - 1])
    assert _same_bits(co, ref.ref(buf[0], np.zeros((E, 2), np.int32), ref.CODES, r, B)[1])


def test_argument_errors():
    from gymca_amd import _lib

    E, H, W, B, r = SHAPES[2]
    buf, parity, pos = ref.make_case(E, H, W, B)
    lo, co = np.zeros((E, 2 * r + 1, 2 * r + 1), np.uint8), np.zeros((E, 2, 2, 3), np.float32)
    p = lambda x: x.ctypes.data

    def call(E=E, H=H, W=W, r=r, B=B, form=0, lo=p(lo), co=p(co), b0=p(buf[0]), codes=ref.CODES):
        _lib.call_cpu("gca_policy_observation", b0, p(buf[1]), p(parity), p(pos), E, H, W, *codes, r, B, form, lo, co,
                      None)

    call()
    for kw in (dict(E=0), dict(H=0), dict(W=-1)):
        with pytest.raises(_lib.GCAError, match="E, H, W must be positive"):
            call(**kw)
    with pytest.raises(_lib.GCAError, match="grid too large"):
        call(H=32768, W=32768)
    for bad in (-1, 32):
        with pytest.raises(_lib.GCAError, match=r"radius in \[0, 31\]"):
            call(r=bad)
    for bad in (0, 3, 12, 128, -8):
        with pytest.raises(_lib.GCAError, match="power of two"):
            call(B=bad)
    for bad in (-1, 3):
        with pytest.raises(_lib.GCAError, match="form 0"):
            call(form=bad)
    # the rows form on shapes it does not cover: (7, 9); B = 4; H % B != 0
    for kw in (dict(B=8), dict(H=32, W=256, B=4), dict(H=24, W=256, B=16), dict(H=32, W=128, B=16),
               dict(H=64, W=512, B=64)):
        with pytest.raises(_lib.GCAError, match="form 2"):
            call(form=2, **kw)
    with pytest.raises(_lib.GCAError, match="local_out or coarse_out"):
        call(lo=None, co=None)
    with pytest.raises(_lib.GCAError, match="buf0"):
        call(b0=None)
    with pytest.raises(_lib.GCAError, match="u8"):
        call(codes=(0, 3, 256))


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] % s[3] == 0 and s[2] % s[3] == 0])
def test_restatement_equals_avg_pool2d_on_dividing_shapes(shape):
    import torch
    import torch.nn.functional as F

    E, H, W, B, r = shape
    buf, parity, pos = ref.make_case(E, H, W, B, seed=13)
    cur = ref.current(buf, parity)
    _, coarse = ref.ref(cur, pos, ref.CODES, r, B)
    g = torch.as_tensor(cur)
    planes = torch.stack([(g == 3), (g == 25)], dim=1).float()
    assert _same_bits(F.avg_pool2d(planes, B).numpy(), coarse)
