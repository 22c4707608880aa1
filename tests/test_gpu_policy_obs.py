"""GPU: the policy observation of the batched envs (gca_policy_observation, env.observe) against its numpy
restatement (tests/_policy_obs_ref.py) and the host build, the two forms of the kernel against each other, and
observe() through both batched envs (steps that flip parity, reset_where, rollout, given outputs, rebinding, a captured
step + observe). Bit for bit throughout; every case is a few envs of at most 64 x 512 cells."""
import numpy as np
import pytest

import _policy_obs_ref as ref

pytestmark = pytest.mark.gpu

# the shapes that decide the rows form: both widths x every block at two block-rows and at one (E = 3)
ROWS = [(3, k * B, W, B, r) for W in (256, 512) for B, r in ((8, 3), (16, 16), (32, 31)) for k in (2, 1)]


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _device_observe(device, buf, parity, pos, codes, r, B, form=0, local=True, coarse=True):
    """gca_policy_observation of the device build on host arrays -> (local, coarse) numpy (None for a skipped part)."""
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    _, E, H, W = buf.shape
    S, Hc, Wc = 2 * r + 1, -(-H // B), -(-W // B)
    b = dev.to_device(buf, torch.uint8, device)
    par = None if parity is None else dev.to_device(parity, torch.uint8, device)
    p = dev.to_device(pos, torch.int32, device)
    lo = torch.full((E, S, S), 0xAA, dtype=torch.uint8, device=device) if local else None
    co = torch.full((E, 2, Hc, Wc), -1.0, dtype=torch.float32, device=device) if coarse else None
    call("gca_policy_observation", dev.ptr(b[0]), None if par is None else dev.ptr(b[1]), dev.ptr(par), dev.ptr(p), E, H,
         W, *codes, r, B, form, dev.ptr(lo), dev.ptr(co), dev.stream_ptr(device))
    return (None if lo is None else lo.cpu().numpy()), (None if co is None else co.cpu().numpy())


def _want(buf, parity, pos, codes, r, B):
    return ref.ref(buf[0] if parity is None else ref.current(buf, parity), pos, codes, r, B)


@pytest.mark.parametrize("rot", [0, 1])
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_device_equals_restatement_and_host_build(device, shape, rot):
    E, H, W, B, r = shape
    buf, parity, pos = ref.make_case(E, H, W, B, rot=rot)
    want = _want(buf, parity, pos, ref.CODES, r, B)
    host = ref.host_observe(buf, parity, pos, ref.CODES, r, B)
    got = _device_observe(device, buf, parity, pos, ref.CODES, r, B)
    for g, h, w, what in zip(got, host, want, ("local", "coarse")):
        assert _same_bits(g, w) and _same_bits(h, w), what


@pytest.mark.parametrize("shape", [ref.SHAPES[0], ref.SHAPES[3]])
def test_null_parity_null_outputs_and_helicopter_codes(device, shape):
    E, H, W, B, r = shape
    buf, parity, pos = ref.make_case(E, H, W, B, codes=ref.HELI_CODES, seed=3, rot=2)
    want = _want(buf, None, pos, ref.HELI_CODES, r, B)
    got = _device_observe(device, buf, None, pos, ref.HELI_CODES, r, B)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    want = _want(buf, parity, pos, ref.HELI_CODES, r, B)
    lo, co = _device_observe(device, buf, parity, pos, ref.HELI_CODES, r, B, coarse=False)
    assert co is None and _same_bits(lo, want[0])
    lo, co = _device_observe(device, buf, parity, pos, ref.HELI_CODES, r, B, local=False)
    assert lo is None and _same_bits(co, want[1])


def _rows_case(E, H, W, B):
    """make_case (a fourth code, env 0's first block all FIRE, the last env's last block all TREE) plus, in env 1, a
    block with FIRE in its first and last column only and one with TREE in its first and last column only: the two ends
    of the cross-lane sum."""
    buf, parity, pos = ref.make_case(E, H, W, B, seed=21)
    g = buf[parity[1], 1]
    Hc, Wc = H // B, W // B
    g[:B, B:2 * B] = ref.OTHER
    g[:B, B], g[:B, 2 * B - 1] = 25, 25
    r0, c0 = (Hc - 1) * B, (Wc - 2) * B
    g[r0:, c0:c0 + B] = 0
    g[r0:, c0], g[r0:, c0 + B - 1] = 3, 3
    return buf, parity, pos


@pytest.mark.parametrize("shape", ROWS)
def test_rows_form_equals_generic_form_and_restatement(device, shape):
    E, H, W, B, r = shape
    buf, parity, pos = _rows_case(E, H, W, B)
    want = _want(buf, parity, pos, ref.CODES, r, B)
    Hc, Wc = H // B, W // B
    # what the special blocks must give (B = 32: per-byte sums of 32, the largest)
    assert want[1][0, 1, 0, 0] == 1.0 and want[1][0, 0, 0, 0] == 0.0
    assert want[1][E - 1, 0, -1, -1] == 1.0 and want[1][E - 1, 1, -1, -1] == 0.0
    assert want[1][1, 1, 0, 1] == np.float32(2.0 / B) and want[1][1, 0, 0, 1] == 0.0
    assert want[1][1, 0, Hc - 1, Wc - 2] == np.float32(2.0 / B) and want[1][1, 1, Hc - 1, Wc - 2] == 0.0
    assert (ref.current(buf, parity) == ref.OTHER).any()
    for form in (1, 2, 0):
        got = _device_observe(device, buf, parity, pos, ref.CODES, r, B, form=form)
        assert _same_bits(got[0], want[0]), ("local", form)
        assert _same_bits(got[1], want[1]), ("coarse", form)


def test_rows_form_is_refused_where_it_does_not_apply(device):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd import _lib

    b = torch.zeros((2, 1, 64, 512), dtype=torch.uint8, device=device)
    par = torch.zeros(1, dtype=torch.uint8, device=device)
    pos = torch.zeros((1, 2), dtype=torch.int32, device=device)
    lo = torch.full((1, 3, 3), 9, dtype=torch.uint8, device=device)
    co = torch.full((1, 2, 64, 64), 9.0, dtype=torch.float32, device=device)

    def call(H, W, B, form=2, lo_=lo, co_=co):
        _lib.call("gca_policy_observation", dev.ptr(b[0]), dev.ptr(b[1]), dev.ptr(par), dev.ptr(pos), 1, H, W,
                  *ref.CODES, 1, B, form, dev.ptr(lo_), dev.ptr(co_), dev.stream_ptr(device))

    for H, W, B in ((7, 9, 4), (7, 9, 8), (32, 256, 4), (24, 256, 16), (40, 512, 32), (64, 512, 64), (32, 128, 16)):
        with pytest.raises(_lib.GCAError, match="form 2"):
            call(H, W, B)
    with pytest.raises(_lib.GCAError, match="local_out or coarse_out"):
        call(32, 256, 16, 0, None, None)
    with pytest.raises(_lib.GCAError, match="radius|power of two"):
        call(32, 256, 3, 0)
    torch.cuda.synchronize(device)
    assert (lo == 9).all() and (co == 9.0).all()  # refused before any launch


# ------------------------------------------------------------------ through the envs
def _check_env(env, codes, **kw):
    """env.observe(**kw) against the restatement of env.grids() / env.pos."""
    local, coarse = env.observe(**kw)
    r, B = kw.get("radius", 16), kw.get("block", 16)
    want = ref.ref(env.grids().cpu().numpy(), env.pos.cpu().numpy(), codes, r, B)
    assert _same_bits(local.cpu().numpy(), want[0]), "local"
    assert _same_bits(coarse.cpu().numpy(), want[1]), "coarse"


def _bulldozer(E, H, W, device, **kw):
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv

    # t_move + t_shoot close to one time unit: a CA step (and a parity flip) on most env steps
    env = BatchedForestFireBulldozerEnv(E, H, W, device=device, seed=17, materialize_obs=False, t_move=0.4, t_shoot=0.3,
                                        p_tree=0.6, p_empty=0.1, **kw)
    env.reset(seed=5)
    return env


def _helicopter(E, H, W, device):
    from gymca_amd.forest_fire.helicopter.batched import BatchedForestFireHelicopterEnv

    env = BatchedForestFireHelicopterEnv(E, H, W, device=device, seed=17, freeze=1, materialize_obs=False)
    env.reset(seed=5)
    return env


@pytest.mark.parametrize("shape", [(3, 32, 256), (2, 16, 512)])
def test_bulldozer_env_observe(device, shape):
    import torch

    E, H, W = shape
    env = _bulldozer(E, H, W, device)
    rng = np.random.default_rng(4)
    _check_env(env, ref.CODES)
    flipped = torch.zeros(E, dtype=torch.bool, device=device)
    for k in range(6):
        act = np.stack([rng.integers(0, 9, E), rng.integers(0, 2, E)], axis=1).astype(np.int32)
        env.step(act)
        flipped |= env.parity.bool()
        _check_env(env, ref.CODES)
        _check_env(env, ref.CODES, radius=3, block=8, form=1)
    assert flipped.any() and (env.steps_elapsed > 0).all()
    mask = np.zeros(E, np.uint8)
    mask[::2] = 1
    env.reset_where(mask)
    _check_env(env, ref.CODES)
    acts = torch.as_tensor(np.stack([rng.integers(0, 9, (5, E)), rng.integers(0, 2, (5, E))], axis=2).astype(np.int32),
                           device=device)
    env.rollout(acts)
    _check_env(env, ref.CODES)
    _check_env(env, ref.CODES, radius=0, block=64)


@pytest.mark.parametrize("shape,block", [((4, 42, 42), 8), ((3, 40, 256), 8), ((3, 40, 256), 16)])
def test_helicopter_env_observe(device, shape, block):
    import torch

    E, H, W = shape
    env = _helicopter(E, H, W, device)
    rng = np.random.default_rng(6)
    _check_env(env, ref.HELI_CODES, block=block)
    flipped = torch.zeros(E, dtype=torch.bool, device=device)
    for k in range(5):
        env.step(rng.integers(0, 9, E).astype(np.int32))
        flipped |= env.parity.bool()
        _check_env(env, ref.HELI_CODES, block=block)
    assert flipped.any()
    env.rollout(torch.as_tensor(rng.integers(0, 9, (4, E)).astype(np.int32), device=device))
    _check_env(env, ref.HELI_CODES, block=block, radius=5)


def test_given_outputs_are_written_in_place_and_checked(device):
    import torch

    E, H, W = 3, 32, 256
    env = _bulldozer(E, H, W, device)
    lo = torch.zeros((E, 33, 33), dtype=torch.uint8, device=device)
    co = torch.zeros((E, 2, 2, 16), dtype=torch.float32, device=device)
    a, b = env.observe(local_out=lo, coarse_out=co)
    assert a is lo and b is co
    fresh = env.observe()
    assert fresh[0] is not lo and torch.equal(fresh[0], lo) and torch.equal(fresh[1], co)
    assert lo.dtype is torch.uint8 and tuple(fresh[0].shape) == (E, 33, 33) and tuple(fresh[1].shape) == (E, 2, 2, 16)
    for bad in (lo.int(), lo[:, :32], lo.cpu(), torch.zeros((E, 33, 66), dtype=torch.uint8, device=device)[:, :, ::2], np.zeros((E, 33, 33))):
        with pytest.raises(ValueError, match="local_out"):
            env.observe(local_out=bad, coarse_out=co)
    for bad in (co.double(), co[:, :1], co.cpu(), torch.zeros((E, 2, 16, 2), device=device)):
        with pytest.raises(ValueError, match="coarse_out"):
            env.observe(local_out=lo, coarse_out=bad)
    for kw in (dict(radius=32), dict(radius=-1), dict(block=12), dict(block=128), dict(form=3)):
        with pytest.raises(ValueError, match="observe"):
            env.observe(**kw)
    from gymca_amd import _lib

    with pytest.raises(_lib.GCAError, match="form 2"):
        env.observe(block=4, form=2)


def test_observe_rebinds_after_a_state_tensor_is_replaced(device):
    import torch

    env = _helicopter(4, 42, 42, device)
    env.observe(block=8)
    assert env._observe_calls
    old = env.buf
    env.buf = env.buf.clone()
    assert not env._observe_calls
    old.fill_(2)  # the tensor the first call bound: all FIRE now
    env.step(np.zeros(4, np.int32))
    _check_env(env, ref.HELI_CODES, block=8)
    env.pos = env.pos.clone()
    env.parity = env.parity.clone()
    _check_env(env, ref.HELI_CODES, block=8)
    env.observe(block=8, radius=2)
    assert len(env._observe_calls) == 2
    env.rebind()
    assert not env._observe_calls


def test_captured_step_and_observe_replays_as_eager(device):
    import torch

    from gymca_amd.graph import StepGraph

    E, H, W = 3, 32, 256
    a, b = _bulldozer(E, H, W, device), _bulldozer(E, H, W, device)
    act = torch.as_tensor(np.stack([np.full(E, 5), np.ones(E)], axis=1).astype(np.int32), device=device)
    outs = [(torch.zeros((E, 33, 33), dtype=torch.uint8, device=device),
             torch.zeros((E, 2, 2, 16), dtype=torch.float32, device=device)) for _ in range(2)]

    def loop(env, out):
        env.step(act)
        env.observe(local_out=out[0], coarse_out=out[1])

    graph = StepGraph(lambda: loop(a, outs[0]), n_steps=1, device=device, warmup=1)  # one warm-up + the capture
    loop(b, outs[1])
    torch.cuda.synchronize(device)
    before = (torch.cuda.memory_allocated(device), torch.cuda.memory_stats(device)["allocation.all.allocated"])
    for _ in range(4):
        graph.replay()
    torch.cuda.synchronize(device)
    assert before == (torch.cuda.memory_allocated(device), torch.cuda.memory_stats(device)["allocation.all.allocated"])
    for _ in range(4):
        loop(b, outs[1])
    for name in ("buf", "parity", "pos", "counts", "reward", "steps_elapsed"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want = ref.ref(a.grids().cpu().numpy(), a.pos.cpu().numpy(), ref.CODES, 16, 16)
    assert _same_bits(outs[0][0].cpu().numpy(), want[0]) and _same_bits(outs[0][1].cpu().numpy(), want[1])
