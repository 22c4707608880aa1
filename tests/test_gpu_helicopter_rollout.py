"""GPU: BatchedForestFireHelicopterEnv.rollout / gca_helicopter_rollout (K env steps in one launch, the grid resident
in LDS) against K step calls of the same env class, and against the host build's step: every state tensor, both planes
of buf included, and the per-step records, exactly (rewards as bits)."""
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


def _step_k(env, actions):
    """K step calls; the per-step reward / hit clones as (K, E) host arrays."""
    rew, hit = [], []
    for k in range(len(actions)):
        env.step(actions[k])
        rew.append(env.reward.clone())
        hit.append(env.hit.clone())
    E = env.num_envs
    return (np.stack([r.cpu().numpy() for r in rew]) if rew else np.zeros((0, E)),
            np.stack([h.cpu().numpy() for h in hit]) if hit else np.zeros((0, E), np.uint8))


def _assert_records(got_r, got_h, want_r, want_h, where):
    assert np.array_equal(got_r.cpu().numpy().view(np.uint64), want_r.view(np.uint64)), f"{where}: reward_out"
    assert np.array_equal(got_h.cpu().numpy(), want_h), f"{where}: hit_out"


def _corner_positions(E, H, W):
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    return np.array([corners[e % 4] for e in range(E)], np.int32)


CASES = [((3, 1, 1), 0, 4), ((4, 5, 5), 0, 7), ((4, 5, 5), 2, 7), ((3, 3, 67), 0, 5), ((2, 42, 42), None, 45),
         ((3, 40, 256), 0, 4), ((3, 40, 256), 2, 7), ((2, 33, 512), 1, 5)]


@pytest.mark.parametrize("shape,max_freeze,K", CASES)
def test_rollout_equals_k_steps(device, shape, max_freeze, K):
    """Actions from [-1, 10) (the clamp); the envs start in the grid's corners, so the first moves run into the
    edges. (2, 42, 42) with the default freeze 21 spans two CA passes and 43 countdown steps."""
    import torch

    E, H, W = shape
    g = _grids(E, H, W, seed=H * W + K)
    pos = _corner_positions(E, H, W)
    a, b = _env(device, g, max_freeze, pos=pos), _env(device, g, max_freeze, pos=pos)
    if max_freeze is None:
        assert a.max_freeze == 21
    actions = np.random.default_rng(K).integers(-1, 10, (K, E)).astype(np.int32)
    want_r, want_h = _step_k(a, actions)
    act_o = torch.full((K, E), -7, dtype=torch.int32, device=device)
    rew_o, hit_o = b.rollout(torch.as_tensor(actions, device=device), action_out=act_o)
    sa, sb = _state(a), _state(b)
    ref.assert_states_equal(sb, sa, "rollout vs K steps")
    _assert_records(rew_o, hit_o, want_r, want_h, "rollout")
    assert np.array_equal(act_o.cpu().numpy(), actions)
    assert b.reward is not rew_o and torch.equal(b.reward, rew_o[-1]) and torch.equal(b.hit, hit_o[-1])
    assert (sb["steps_elapsed"] == K).all()
    if max_freeze is None:  # CA passes at steps 21 and 43 (0-based), one countdown step after the second
        assert (sb["parity"] == 0).all() and (sb["freeze"] == 20).all()
    if (H, W) in ((5, 5), (42, 42)):
        host = ref.make_state(g, THR, a.max_freeze, pos=pos)
        for k in range(K):
            ref.host_step(host, actions[k], a.max_freeze, SEED, 0)
        ref.assert_states_equal(sb, host, "rollout vs K host steps")
    assert not a._meet.any().item() and not b._meet.any().item()


def test_hits_really_happen(device):
    """Env 0 moves up onto a TREE whose neighbour burns, on a CA step (k = 1: the TREE ignites and Modify puts it out);
    env 1 sits on a FIRE cell during a countdown step (k = 0). Thresholds 0: nothing else ignites or grows."""
    import torch

    E, H, W, K = 2, 8, 12, 3
    g = np.zeros((E, H, W), np.uint8)
    g[0, 3, 5], g[0, 3, 6] = 1, 2               # TREE at (3, 5), FIRE right of it
    g[1, 4, 7], g[1, 0, 0], g[1, 4, 5] = 1, 1, 2  # two TREEs away from the FIRE under the helicopter
    pos = np.array([[5, 5], [4, 5]], np.int32)
    zero = np.array([0.0, 0.0])
    actions = np.array([[1, 4], [1, 4], [4, 4]], np.int32)  # env 0: up, up, stay; env 1 stays
    a, b = _env(device, g, 2, pos=pos, thr=zero), _env(device, g, 2, pos=pos, thr=zero)
    for env in (a, b):
        # env 0 runs the CA at k = 1, env 1 at k = 2
        env.set_state(freeze=torch.tensor([1, 2], dtype=torch.int32, device=device))
    counts0 = a.counts.cpu().numpy().copy()
    assert counts0.tolist() == [[H * W - 2, 1, 1], [H * W - 3, 2, 1]]
    want_r, want_h = _step_k(a, actions)
    rew_o, hit_o = b.rollout(torch.as_tensor(actions, device=device))
    ref.assert_states_equal(_state(b), _state(a), "rollout vs K steps")
    _assert_records(rew_o, hit_o, want_r, want_h, "rollout")
    hits = hit_o.cpu().numpy()
    assert hits.tolist() == [[0, 1], [1, 0], [0, 0]] and hits.sum() > 0
    counts = b.counts.cpu().numpy()
    # env 0: the FIRE burnt out, the ignited TREE was put out: all EMPTY; env 1: its FIRE became EMPTY in place
    assert counts.tolist() == [[H * W, 0, 0], [H * W - 2, 2, 0]]
    assert b.parity.cpu().numpy().tolist() == [1, 1]
    assert not a._meet.any().item() and not b._meet.any().item()


def test_random_policy_equals_step_random(device):
    import torch

    E, K = 5, 6
    g = _grids(E, 9, 13, seed=3)
    a, b = _env(device, g, 1), _env(device, g, 1)
    out = torch.full((E,), -7, dtype=torch.int32, device=device)
    taken, rew, hit = [], [], []
    for k in range(K):
        a.step_random(seed=11, action_out=out)
        taken.append(out.cpu().numpy().copy())
        rew.append(a.reward.cpu().numpy().copy())
        hit.append(a.hit.cpu().numpy().copy())
    act_o = torch.full((K, E), -7, dtype=torch.int32, device=device)
    rew_o, hit_o = b.rollout(K=K, seed=11, action_out=act_o)
    ref.assert_states_equal(_state(b), _state(a), "random rollout")
    _assert_records(rew_o, hit_o, np.stack(rew), np.stack(hit), "random rollout")
    acts = act_o.cpu().numpy()
    assert np.array_equal(acts, np.stack(taken))
    assert ((0 <= acts) & (acts < 9)).all() and len(np.unique(acts)) > 3
    assert not b._meet.any().item()


def test_state_carries_across_launches(device):
    """rollout of 3, step, rollout of 4 against 8 steps, freeze 1. The envs start staggered (freeze 1, 0, 1) and take one
    step before the comparison begins: env 1 has then run one CA pass, so it enters both rollouts on the odd plane with
    its countdown running (parity 1, freeze 1), while envs 0 and 2 enter them on the even plane at freeze 0."""
    import torch

    E, H, W = 3, 40, 256
    g = _grids(E, H, W, seed=11)
    a, b = _env(device, g, 1), _env(device, g, 1)
    for env in (a, b):
        env.set_state(freeze=[1, 0, 1])
        env.step(np.full(E, 4, np.int32))
    actions = np.random.default_rng(5).integers(-1, 10, (8, E)).astype(np.int32)
    want_r, want_h = _step_k(a, actions)

    def entering():
        parity, freeze = b.parity.cpu().numpy(), b.freeze.cpu().numpy()
        assert ((parity == 1) & (freeze == 1)).any() and (parity == 0).any(), (parity, freeze)

    entering()
    r0, h0 = b.rollout(actions[:3])  # a numpy (K, E) array is converted
    b.step(actions[3])
    r3, h3 = b.reward.clone(), b.hit.clone()
    entering()
    r4, h4 = b.rollout(torch.as_tensor(actions[4:], device=device))
    ref.assert_states_equal(_state(b), _state(a), "3 + 1 + 4 vs 8 steps")
    _assert_records(torch.cat([r0, r3[None], r4]), torch.cat([h0, h3[None], h4]), want_r, want_h, "3 + 1 + 4")
    assert not b._meet.any().item()


def test_sharded_rollout_equals_the_unsharded(device):
    """Envs [4, 6) of an E = 8 env equal an E = 2 env with env_offset = 4: reset and a rollout of 5."""
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv

    kw = dict(device=device, seed=SEED, freeze=1, materialize_obs=False)
    full = BatchedForestFireHelicopterEnv(8, 12, 20, **kw)
    part = BatchedForestFireHelicopterEnv(2, 12, 20, env_offset=4, **kw)
    full.reset()
    part.reset()
    actions = np.random.default_rng(1).integers(0, 9, (5, 8)).astype(np.int32)
    rf, hf = full.rollout(actions)
    rp, hp = part.rollout(np.ascontiguousarray(actions[:, 4:6]))
    sf, sp = _state(full), _state(part)
    for key in ref.STATE_KEYS:
        x = sf[key][:, 4:6] if key == "buf" else sf[key][4:6]
        if key == "reward":
            x, y = x.view(np.uint64), sp[key].view(np.uint64)
        else:
            y = sp[key]
        assert np.array_equal(x, y), key
    _assert_records(rp, hp, rf.cpu().numpy()[:, 4:6].copy(), hf.cpu().numpy()[:, 4:6].copy(), "shard")
    g = sf["buf"][0]
    assert len(np.unique(g)) == 3 and not np.array_equal(g[4], g[5])
    assert not full._meet.any().item() and not part._meet.any().item()


def test_graph_replay_equals_eager(device):
    """One rollout captured on one stream (a linear graph) and replayed once against the eager one."""
    import torch

    E, K = 4, 3
    g = _grids(E, 40, 256, seed=7)
    eager, graphed = _env(device, g, 1), _env(device, g, 1)
    actions = torch.as_tensor(np.array([[0, 5, 7, 8], [-1, 9, 4, 2], [6, 6, 1, 3]], np.int32), device=device)
    er, eh = eager.rollout(actions)
    rew_o = torch.zeros((K, E), dtype=torch.float64, device=device)
    hit_o = torch.zeros((K, E), dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.rollout(actions, reward_out=rew_o, hit_out=hit_o)
    ref.assert_states_equal(_state(graphed), ref.make_state(g, THR, 1), "capture runs nothing")
    assert not rew_o.any().item()
    graph.replay()
    torch.cuda.synchronize(device)
    ref.assert_states_equal(_state(graphed), _state(eager), "replay")
    _assert_records(rew_o, hit_o, er.cpu().numpy(), eh.cpu().numpy(), "replay")
    assert not graphed._meet.any().item()


def test_grid_too_large_for_lds_takes_k_launches(device):
    """(2, 130, 256): two padded planes of 4 * (1 + 132 * 65) bytes exceed 64 KiB, so the rollout runs K launches of
    the step kernel; the caller sees the same results and records."""
    import torch

    E, H, W, K = 2, 130, 256, 3
    assert 2 * 4 * (1 + (H + 2) * (W // 4 + 1)) > 65536
    g = _grids(E, H, W, seed=13)
    a, b = _env(device, g, 0), _env(device, g, 0)
    actions = np.random.default_rng(3).integers(-1, 10, (K, E)).astype(np.int32)
    want_r, want_h = _step_k(a, actions)
    act_o = torch.full((K, E), -7, dtype=torch.int32, device=device)
    rew_o, hit_o = b.rollout(actions, action_out=act_o)
    ref.assert_states_equal(_state(b), _state(a), "K launches vs K steps")
    _assert_records(rew_o, hit_o, want_r, want_h, "K launches")
    assert np.array_equal(act_o.cpu().numpy(), actions)
    assert (b.parity.cpu().numpy() == 1).all()
    assert not b._meet.any().item()


def test_rollout_validation(device):
    import torch

    E, K = 2, 3
    g = _grids(E, 5, 7, seed=2)
    env = _env(device, g, 1)
    before = _state(env)
    good = torch.zeros((K, E), dtype=torch.int32, device=device)
    with pytest.raises(ValueError):
        env.rollout(torch.zeros((K, E), dtype=torch.float32, device=device))   # dtype
    with pytest.raises(ValueError):
        env.rollout(np.zeros((K, E), np.float64))                               # dtype, host
    with pytest.raises(ValueError):
        env.rollout(torch.zeros((K, E + 1), dtype=torch.int32, device=device))  # shape
    with pytest.raises(ValueError):
        env.rollout(torch.zeros(E, dtype=torch.int32, device=device))           # not (K, E)
    with pytest.raises(ValueError):
        env.rollout(good, K=K + 1)                                              # K disagrees
    with pytest.raises(ValueError):
        env.rollout()                                                           # neither actions nor K
    with pytest.raises(ValueError):
        env.rollout(good, reward_out=torch.zeros((K, E), dtype=torch.float32, device=device))
    with pytest.raises(ValueError):
        env.rollout(good, reward_out=torch.zeros((K + 1, E), dtype=torch.float64, device=device))
    with pytest.raises(ValueError):
        env.rollout(good, hit_out=torch.zeros((K, E), dtype=torch.uint8))       # a host tensor
    with pytest.raises(ValueError):
        env.rollout(good, hit_out=torch.zeros((K, E), dtype=torch.int32, device=device))
    with pytest.raises(ValueError):
        env.rollout(good, action_out=torch.zeros((K, E), dtype=torch.int64, device=device))
    with pytest.raises(ValueError):
        env.rollout(good, action_out=torch.zeros((E, K), dtype=torch.int32, device=device).t())  # not contiguous
    ref.assert_states_equal(_state(env), before, "a refused call runs nothing")
    r, h = env.rollout(K=0)
    assert tuple(r.shape) == (0, E) and r.dtype is torch.float64 and tuple(h.shape) == (0, E) and h.dtype is torch.uint8
    r, h = env.rollout(good[:0])
    assert tuple(r.shape) == (0, E) and tuple(h.shape) == (0, E)
    ref.assert_states_equal(_state(env), before, "K = 0")
    # int64 device actions, host arrays and tensors and a replaced bound tensor all work
    twin = _env(device, g, 1)
    env.rollout(good.to(torch.int64) + 5)
    new_pos = env.pos.clone()
    env.pos = new_pos
    env.rollout(good + 3)
    twin.rollout(np.full((K, E), 5))
    twin.rollout(torch.full((K, E), 3))  # a host tensor: the helicopter converts it like a numpy array
    ref.assert_states_equal(_state(env), _state(twin), "converted actions, rebound pos")
    assert env._ctx["position"] is new_pos
    assert not env._meet.any().item() and not twin._meet.any().item()
