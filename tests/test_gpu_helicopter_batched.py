"""GPU: BatchedForestFireHelicopterEnv / gca_helicopter_step against the host build of the same entry point
(itself pinned to the numpy restatement, the oracle's rule and the reference's episode in
test_helicopter_batched_cpu.py), the existing device gca_ds_step, its own one-workgroup form, sharding, graph replay
and the bound-tensor guard."""
import numpy as np
import pytest

import _helicopter_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678
THR = np.array([0.05, 0.4])


def _grids(E, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 3, (E, H, W)).astype(np.uint8)


def _env(device, grids, max_freeze, env_offset=0, pos=None, thr=THR, **kw):
    import torch

    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv

    E, H, W = grids.shape
    env = BatchedForestFireHelicopterEnv(E, H, W, device=device, seed=SEED, env_offset=env_offset, freeze=max_freeze,
                                         materialize_obs=False, **kw)
    env.reset(grids=grids, positions=pos)
    env.thresholds.copy_(torch.as_tensor(np.broadcast_to(thr, (E, 2)).copy(), device=device))
    return env


def _state(env):
    """The env's device state as host arrays in _helicopter_ref's layout."""
    s = {k: getattr(env, k).cpu().numpy() for k in ref.STATE_KEYS}
    s["rng_step"] = s["rng_step"].view(np.uint32)
    return s


def _raw_step(env, action, meet):
    """gca_helicopter_step on the env's tensors with the caller's `meet` (None: one workgroup per env)."""
    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    call("gca_helicopter_step", 0, 1, 2, env.max_freeze, SEED, env.env_offset, dev.ptr(action), 0, None,
         dev.ptr(env.thresholds), dev.ptr(env.freeze), dev.ptr(env.rng_step), dev.ptr(env.parity),
         dev.ptr(env.buf[0]), dev.ptr(env.buf[1]), env.nrows, env.ncols, dev.ptr(env.pos), dev.ptr(env.counts),
         dev.ptr(env.hit), dev.ptr(env.reward), dev.ptr(env.steps_elapsed), dev.ptr(meet), env.num_envs,
         dev.stream_ptr(env.device))


CORNER_MOVES = (0, 2, 6, 8)  # up-left, up-right, down-left, down-right


@pytest.mark.parametrize("shape,max_freeze", [((3, 1, 1), 0), ((4, 5, 5), 0), ((3, 3, 67), 0), ((2, 37, 64), 0),
                                              ((3, 40, 256), 0), ((2, 33, 512), 0), ((4, 5, 5), 2),
                                              ((3, 40, 256), 2)])
def test_device_step_equals_host_build(device, shape, max_freeze):
    """6 steps: steps 0-3 start every env diagonally next to corner k and move into it, steps 4 and 5 pass the
    out-of-range actions -1 and 9 (clamped to 0 and 8). Every state tensor is compared exactly after every step."""
    import torch

    E, H, W = shape
    g = _grids(E, H, W, seed=H * W)
    env = _env(device, g, max_freeze)
    host = ref.make_state(g, THR, max_freeze)
    ref.assert_states_equal(_state(env), host, "reset")
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    hits = 0
    for k in range(6):
        if k < 4:
            r, c = corners[k]
            start = (min(max(r + (1 if r == 0 else -1), 0), H - 1), min(max(c + (1 if c == 0 else -1), 0), W - 1))
            host["pos"][:] = start
            env.pos.copy_(torch.as_tensor(host["pos"], device=device))
            act = np.full(E, CORNER_MOVES[k], np.int32)
        else:
            act = np.full(E, -1 if k == 4 else 9, np.int32)
        env.step(act)
        ref.host_step(host, act, max_freeze, SEED, 0)
        if k < 4:
            assert (host["pos"] == corners[k]).all()
        ref.assert_states_equal(_state(env), host, f"step {k}")
        hits += int(host["hit"].sum())
    assert (host["steps_elapsed"] == 6).all()
    assert not env._meet.any().item()


@pytest.mark.parametrize("shape", [(3, 40, 256), (3, 3, 67)])
def test_ca_pass_equals_device_ds_step(device, shape):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    E, H, W = shape
    g = _grids(E, H, W, seed=5)
    g[:, H // 2, W // 2] = 0  # Modify's cell stays EMPTY / TREE through the CA: the pass shows unmodified
    env = _env(device, g, 0, env_offset=5)
    env.set_state(rng_step=[3, 4, 5])
    gin = env.buf[0].clone()
    out = torch.zeros_like(gin)
    counts = torch.zeros((E, 3), dtype=torch.int32, device=device)
    call("gca_ds_step", dev.ptr(gin), dev.ptr(out), E, H, W, 0, 1, 2, dev.ptr(env.thresholds), None, None, SEED,
         dev.ptr(env.rng_step), 5, dev.ptr(counts), dev.stream_ptr(device))
    env.step(np.full(E, 4, np.int32))
    assert not env.hit.any().item() and env.parity.all().item()
    assert torch.equal(env.buf[1], out) and torch.equal(env.counts, counts)
    assert not torch.equal(out, gin)


@pytest.mark.parametrize("shape", [(3, 40, 256), (2, 33, 512)])
def test_parts_equal_one_workgroup(device, shape):
    """The env's rows over several workgroups (with `meet`) against one workgroup per env (without), CA steps and
    countdown steps alike; helicopters on a strip boundary (rows 15 / 16), on the parts' boundary (rows 31 / 32, the
    start of the last, partial strip) and in the last strip; a TREE under the helicopter ignited from the next strip
    gives a certain hit in step 0."""
    import torch

    E, H, W = shape
    g = _grids(E, H, W, seed=9)
    pos = np.array([[16, 255 % W], [31, W - 1], [H - 2, 0]][:E], np.int32)
    g[0, 15, pos[0, 1]], g[0, 16, pos[0, 1]] = 1, 2  # env 0 moves up onto a TREE whose neighbour below burns
    g[1, 31, W - 1], g[1, 32, W - 1] = 2, 1          # env 1 moves down onto a TREE whose neighbour above burns
    moves = np.array([1, 7, 7][:E], np.int32)
    a, b = _env(device, g, 1, pos=pos), _env(device, g, 1, pos=pos)
    a.set_state(freeze=0)
    b.set_state(freeze=0)
    meet = torch.zeros(E, dtype=torch.int64, device=device)
    for k in range(6):
        act = torch.as_tensor(moves if k % 2 == 0 else 8 - moves, device=device)
        _raw_step(a, act, meet)
        _raw_step(b, act, None)
        sa, sb = _state(a), _state(b)
        ref.assert_states_equal(sa, sb, f"step {k}")
        if k == 0:
            assert sa["hit"][0] == 1 and sa["hit"][1] == 1 and (sa["parity"] == 1).all()
        assert not meet.any().item()
    host = ref.make_state(g, THR, 1, pos=pos, freeze=0)
    for k in range(6):
        ref.host_step(host, moves if k % 2 == 0 else 8 - moves, 1, SEED, 0)
    ref.assert_states_equal(_state(a), host, "host build")


def test_step_random_equals_sample_then_step(device):
    import torch

    g = _grids(5, 9, 13, seed=3)
    a, b = _env(device, g, 1), _env(device, g, 1)
    out = torch.full((5,), -7, dtype=torch.int32, device=device)
    seen = set()
    for k in range(5):
        a.step_random(seed=11, action_out=out)
        acts = b.sample_actions(tag=11)
        assert torch.equal(acts, out)
        b.step(acts)
        ref.assert_states_equal(_state(a), _state(b), f"step {k}")
        seen.update(out.cpu().numpy().tolist())
    assert seen <= set(range(9)) and len(seen) > 3


def test_sharded_envs_equal_the_unsharded(device):
    """Envs [4, 6) of an E = 8 env equal an E = 2 env with env_offset = 4: reset and 5 steps."""
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv

    kw = dict(device=device, seed=SEED, freeze=1, materialize_obs=False)
    full = BatchedForestFireHelicopterEnv(8, 12, 20, **kw)
    part = BatchedForestFireHelicopterEnv(2, 12, 20, env_offset=4, **kw)
    full.reset()
    part.reset()
    rng = np.random.default_rng(1)
    for k in range(5):
        act = rng.integers(0, 9, 8).astype(np.int32)
        full.step(act)
        part.step(act[4:6])
        sf, sp = _state(full), _state(part)
        for key in ref.STATE_KEYS:
            x = sf[key][:, 4:6] if key == "buf" else sf[key][4:6]
            assert np.array_equal(x, sp[key]), f"step {k}: {key}"
    g = sf["buf"][0]
    assert len(np.unique(g)) == 3 and not np.array_equal(g[4], g[5])


def test_graph_replay_equals_eager(device):
    """3 step calls captured on one stream (a linear graph) and replayed once against 3 eager steps."""
    import torch

    g = _grids(4, 40, 256, seed=7)
    eager, graphed = _env(device, g, 1), _env(device, g, 1)
    act = torch.as_tensor(np.array([0, 5, 7, 8], np.int32), device=device)
    for _ in range(3):
        eager.step(act)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(3):
            graphed.step(act)
    ref.assert_states_equal(_state(graphed), ref.make_state(g, THR, 1), "capture runs nothing")
    graph.replay()
    torch.cuda.synchronize(device)
    ref.assert_states_equal(_state(graphed), _state(eager), "replay")


def test_bound_tensor_guard(device):
    import torch

    g = _grids(2, 5, 7, seed=2)
    env, twin = _env(device, g, 0), _env(device, g, 0)
    act = np.array([4, 4], np.int32)
    env.step(act)
    twin.step(act)
    with pytest.raises(ValueError):
        env.pos = torch.zeros((2, 2), dtype=torch.int64, device=device)
    with pytest.raises(ValueError):
        env.freeze = torch.zeros(3, dtype=torch.int32, device=device)
    with pytest.raises(ValueError):
        env.buf = torch.zeros((2, 2, 5, 7), dtype=torch.uint8)  # a host tensor
    new_pos = torch.tensor([[0, 0], [4, 6]], dtype=torch.int32, device=device)
    env.pos = new_pos
    twin.pos.copy_(new_pos)
    obs, reward, terminated, truncated, info = env.step(act)
    twin.step(act)
    assert obs[1]["position"] is new_pos and torch.equal(new_pos.cpu(), torch.tensor([[0, 0], [4, 6]], dtype=torch.int32))
    ref.assert_states_equal(_state(env), _state(twin), "rebound")
    assert not terminated.any().item() and not truncated.any().item() and info["hit"] is env.hit
