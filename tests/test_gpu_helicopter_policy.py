"""GPU: the helicopter policy inside the env's launches. env.act (gca_helicopter_policy_act) against the host build,
and env.rollout_policy (gca_helicopter_policy_rollout: K closed-loop steps in one launch, the grid resident in LDS)
against K x (observe, act, step) on the device and against the host build's rollout: both planes of buf, every state
tensor and every record, bit for bit."""
import numpy as np
import pytest

import _bulldozer_policy_ref as bref
import _helicopter_policy_ref as pref
import _helicopter_ref as href
import _policy_obs_ref as obs

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678
THR = np.array([0.05, 0.4])


def _env(device, grids, max_freeze, env_offset=0, pos=None, thr=THR, rng_step=None):
    import torch

    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv

    E, H, W = grids.shape
    env = BatchedForestFireHelicopterEnv(E, H, W, device=device, seed=SEED, env_offset=env_offset, freeze=max_freeze,
                                         materialize_obs=False)
    env.reset(grids=grids, positions=pos)
    env.thresholds.copy_(torch.as_tensor(np.broadcast_to(thr, (E, 2)).copy(), device=device))
    if rng_step is not None:
        env.set_state(rng_step=rng_step)
    return env


def _policy(device, d, w):
    from gymca_amd.forest_fire.helicopter import HelicopterPolicy

    return HelicopterPolicy((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device=device).load(w)


def _state(env):
    s = {k: getattr(env, k).cpu().numpy() for k in href.STATE_KEYS}
    s["rng_step"] = s["rng_step"].view(np.uint32)
    return s


def _host(t):
    return {k: v.cpu().numpy() for k, v in t.items()}


def _steps_k(env, pol, K, seed, greedy=False):
    """K x (observe, act, step) on the device; the records as rollout_policy defines them, as host arrays."""
    import torch

    rows = {n: [] for n in pref.RECORDS}
    for _ in range(K):
        lo, co = env.observe(pol.radius, pol.block)
        act, lg, va = env.act(pol, lo, co, seed=seed, greedy=greedy)
        env.step(act)
        for n, t in zip(pref.RECORDS, (act, lg, va, env.reward.clone(), env.hit.clone(), lo, co)):
            rows[n].append(t)
    return {n: torch.stack(v).cpu().numpy() for n, v in rows.items()}


def _corners(E, H, W):
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    return np.array([corners[e % 4] for e in range(E)], np.int32)


# the CPU test's shapes, the flagship's radius 5 / block 8 at Hd = 128, and Hd = 256 (the fewest groups, G = 4)
ACT_SHAPES = pref.SHAPES + [(5, 8, 128, 42, 42), (1, 4, 256, 5, 5)]


@pytest.mark.parametrize("shape", ACT_SHAPES)
def test_act_equals_the_host_build(device, shape):
    import torch

    r, B, Hd, H, W = shape
    E, off = 5, 3
    d = pref.dims(*shape)
    w = pref.make_weights(d, seed=Hd + H, head=2.0)
    buf, parity, _ = obs.make_case(E, H, W, B, codes=obs.HELI_CODES, seed=1)
    pos = obs.positions(E, H, W)
    local, coarse = obs.host_observe(buf, parity, pos, obs.HELI_CODES, r, B)
    rs = np.array([0, 1, 7, 0xFFFFFFFF, 12345], np.uint32)
    env = _env(device, pref.grids(E, H, W), 2, env_offset=off, rng_step=rs.astype(np.int64))
    pol = _policy(device, d, w)
    before = _state(env)
    lo_d, co_d = torch.as_tensor(local, device=device), torch.as_tensor(coarse, device=device)
    for greedy in (False, True):
        want_a, want_l, want_v = pref.host_act(w, d, local, coarse, rs, env_offset=off, seed=91, greedy=greedy)
        act, lg, va = env.act(pol, lo_d, co_d, seed=91, greedy=greedy)
        assert np.array_equal(lg.cpu().numpy().view(np.uint32), want_l.view(np.uint32)), "logits"
        assert np.array_equal(va.cpu().numpy().view(np.uint32), want_v.view(np.uint32)), "value"
        assert np.array_equal(act.cpu().numpy(), want_a), "action"
    href.assert_states_equal(_state(env), before, "act leaves every env tensor untouched")
    # without an observation act() observes the env's own state
    lo, co = env.observe(r, B)
    a1, l1, v1 = env.act(pol, seed=91)
    a2, l2, v2 = env.act(pol, lo, co, seed=91)
    assert torch.equal(a1, a2) and torch.equal(l1, l2) and torch.equal(v1, v2)
    href.assert_states_equal(_state(env), before, "act leaves every env tensor untouched")


# (E, H, W) with the policy (radius, block, hidden) each grid gets
ROLLOUT_GRIDS = [((3, 1, 1), (0, 1, 32)), ((4, 5, 5), (1, 64, 32)), ((3, 3, 67), (2, 4, 128)), ((2, 42, 42), (3, 8, 64))]


@pytest.mark.parametrize("max_freeze", [0, 2, None])
@pytest.mark.parametrize("K", [1, 7, 70])
@pytest.mark.parametrize("grid,net", ROLLOUT_GRIDS)
def test_rollout_policy_equals_k_observe_act_step(device, grid, net, K, max_freeze):
    """The envs start in the grid's four corners, so the windows hang over the edges and the first moves run into them.
    K = 70 crosses the kernel's 64-step record chunk."""
    import torch

    (E, H, W), (r, B, Hd) = grid, net
    d = pref.dims(r, B, Hd, H, W)
    w = pref.make_weights(d, seed=5, head=3.0)
    g, pos = pref.grids(E, H, W, seed=H * W + K), _corners(E, H, W)
    thr = THR if H * W > 1 else np.array([0.5, 0.5])
    a, b = _env(device, g, max_freeze, pos=pos, thr=thr), _env(device, g, max_freeze, pos=pos, thr=thr)
    mf = a.max_freeze
    pol = _policy(device, d, w)
    want = _steps_k(a, pol, K, seed=17)
    got = _host(b.rollout_policy(pol, K, seed=17))
    sa, sb = _state(a), _state(b)
    href.assert_states_equal(sb, sa, "rollout_policy vs K x (observe, act, step)")
    pref.assert_records_equal(got, want, "device")
    assert torch.equal(b.reward, torch.as_tensor(got["reward"][-1], device=device))
    host = href.make_state(g, thr, mf, pos=pos)
    host_rec = pref.host_rollout_policy(host, w, d, K, mf, SEED, 0, policy_seed=17)
    href.assert_states_equal(sb, host, "rollout_policy vs the host rollout")
    pref.assert_records_equal(got, host_rec, "host")
    assert (sb["steps_elapsed"] == K).all()
    if K == 70 and H * W > 1:
        assert len(np.unique(got["action"])) > 1 and got["hit"].any()
    assert not b._meet.any().item()


def test_the_action_follows_the_observation_of_its_own_step(device):
    """Weights whose logits depend only on the FIRE entry of the window cell right of the helicopter: FIRE there ->
    action 5 (right, onto it), else action 7 (down). A policy fed a stale or a post-step observation fails: with a CA
    pass every step the cell changes between steps."""
    E, H, W, K = 6, 9, 12, 40
    d = pref.dims(1, 4, 32, H, W)
    w = {k: np.zeros_like(v) for k, v in pref.make_weights(d).items()}
    n0 = 1 * d["S"] + 2                       # window cell (row 1, column 2): right of the centre
    w["w_local"][n0, 2, 0] = 1.0              # hidden unit 0 = 1 iff that cell is FIRE
    w["w_out"][0, 5] = 20.0
    w["b2"][7] = 10.0
    g = pref.grids(E, H, W, seed=21)
    pol = _policy(device, d, w)
    for greedy in (True, False):  # the logits are 10 apart or more: the draw takes the maximum too (p > 1 - 1e-3)
        env = _env(device, g, 0, pos=_corners(E, H, W), thr=np.array([0.3, 0.5]))
        rec = _host(env.rollout_policy(pol, K, seed=3, greedy=greedy))
        fire_right = rec["local"].reshape(K, E, -1)[:, :, n0] == 2
        want = np.where(fire_right, 5, 7)
        if greedy:
            assert np.array_equal(rec["action"], want)
        else:
            assert (rec["action"] == want).mean() > 0.99
        assert fire_right.any() and not fire_right.all()
        assert rec["hit"].any()
        # the logits the step recorded are those of its own window
        assert np.array_equal(rec["logits"][..., 5] == 20.0, fire_right)


def test_state_carries_across_calls_and_interleaves(device):
    E, H, W, K = 3, 9, 13, 9
    d = pref.dims(2, 4, 64, H, W)
    w = pref.make_weights(d, seed=8, head=3.0)
    g = pref.grids(E, H, W, seed=4)
    a, b = _env(device, g, 1), _env(device, g, 1)
    pol = _policy(device, d, w)
    one = _host(a.rollout_policy(pol, 2 * K, seed=5))
    first = _host(b.rollout_policy(pol, K, seed=5))
    second = _host(b.rollout_policy(pol, K, seed=5))
    href.assert_states_equal(_state(b), _state(a), "K + K vs 2K")
    pref.assert_records_equal({n: np.concatenate([first[n], second[n]]) for n in one}, one, "K + K vs 2K")
    # step / rollout / rollout_policy interleave: the same on both envs
    for env in (a, b):
        env.step(np.full(E, 4, np.int32))
        env.rollout(np.full((2, E), 1, np.int32))
    ra, rb = _host(a.rollout_policy(pol, 3, seed=6)), _host(b.rollout_policy(pol, 3, seed=6, record=("action",)))
    href.assert_states_equal(_state(b), _state(a), "interleaved")
    assert set(rb) == {"action"} and np.array_equal(ra["action"], rb["action"])
    # a replaced policy tensor rebinds the call
    new_b2 = pol.b2.clone()
    new_b2[3] += 50.0
    pol.b2 = new_b2
    rec = _host(a.rollout_policy(pol, 2, seed=6, greedy=True))
    assert (rec["action"] == 3).all()


def test_sharded_rollout_equals_the_unsharded(device):
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv

    kw = dict(device=device, seed=SEED, freeze=1, materialize_obs=False)
    full = BatchedForestFireHelicopterEnv(8, 12, 20, **kw)
    part = BatchedForestFireHelicopterEnv(2, 12, 20, env_offset=4, **kw)
    full.reset()
    part.reset()
    d = pref.dims(2, 4, 32, 12, 20)
    pol = _policy(device, d, pref.make_weights(d, seed=2, head=3.0))
    rf, rp = _host(full.rollout_policy(pol, 6, seed=9)), _host(part.rollout_policy(pol, 6, seed=9))
    sf, sp = _state(full), _state(part)
    for key in href.STATE_KEYS:
        x = sf[key][:, 4:6] if key == "buf" else sf[key][4:6]
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), sp[key].view(np.uint8)), key
    pref.assert_records_equal(rp, {n: np.ascontiguousarray(v[:, 4:6]) for n, v in rf.items()}, "shard")
    assert len(np.unique(rf["action"])) > 1


def test_graph_replay_equals_eager(device):
    import torch

    E, H, W, K = 4, 10, 11, 5
    d = pref.dims(1, 4, 32, H, W)
    g = pref.grids(E, H, W, seed=7)
    eager, graphed = _env(device, g, 1), _env(device, g, 1)
    pol = _policy(device, d, pref.make_weights(d, seed=2, head=3.0))
    want = _host(eager.rollout_policy(pol, K, seed=4))
    outs = {n + "_out": torch.zeros_like(torch.as_tensor(v), device=device) for n, v in want.items()}
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec = graphed.rollout_policy(pol, K, seed=4, **outs)
    href.assert_states_equal(_state(graphed), href.make_state(g, THR, 1), "capture runs nothing")
    graph.replay()
    torch.cuda.synchronize(device)
    href.assert_states_equal(_state(graphed), _state(eager), "replay")
    pref.assert_records_equal(_host(rec), want, "replay")
    assert all(rec[n] is outs[n + "_out"] for n in want)


@pytest.mark.parametrize("H,W,B", [(40, 512, 2), (130, 256, 16)])
def test_grid_too_large_for_lds_takes_the_k_launch_path(device, H, W, B):
    """40 x 512 at block 2: the two padded planes (43 KiB) plus the network's words (a coarse map of 10240 floats) exceed
    64 KiB; 130 x 256: the planes alone do. Either way the rollout runs K x 3 launches and the caller sees the same
    results, with every record kept and with none (the window, the coarse map and the action of a step then live in the
    env's scratch)."""
    E, K = 2, 3
    C = 2 * -(-H // B) * -(-W // B)
    planes = 2 * 4 * ((1 + (H + 2) * (W // 4 + 1) + 3) & ~3) + 64
    assert planes + 4 * (C + 1296) > 65536 and 4 * (C + 1296) <= 65536
    assert (planes > 65536) == (H == 130)
    d = pref.dims(2, B, 32, H, W)
    w = pref.make_weights(d, seed=6, head=3.0)
    g = pref.grids(E, H, W, seed=13)
    a, b, c = _env(device, g, 0), _env(device, g, 0), _env(device, g, 0)
    pol = _policy(device, d, w)
    want = _steps_k(a, pol, K, seed=2)
    got = _host(b.rollout_policy(pol, K, seed=2))
    none = c.rollout_policy(pol, K, seed=2, record=())
    assert none == {}
    href.assert_states_equal(_state(b), _state(a), "K x 3 launches vs K x (observe, act, step)")
    href.assert_states_equal(_state(c), _state(a), "no records kept")
    pref.assert_records_equal(got, want, "K x 3 launches")
    assert (b.parity.cpu().numpy() == 1).all()


def test_greedy_is_deterministic_across_seeds(device):
    E, H, W, K = 3, 7, 9, 12
    d = pref.dims(2, 4, 32, H, W)
    g = pref.grids(E, H, W, seed=5)
    pol = _policy(device, d, pref.make_weights(d, seed=1, head=3.0))
    recs = []
    for seed in (1, 2):
        env = _env(device, g, 1)
        recs.append(_host(env.rollout_policy(pol, K, seed=seed, greedy=True)))
    pref.assert_records_equal(recs[0], recs[1], "greedy")
    assert np.array_equal(recs[0]["action"], pref.greedy_ref(recs[0]["logits"]).reshape(K, E))
    sampled = _host(_env(device, g, 1).rollout_policy(pol, K, seed=1))
    assert not np.array_equal(sampled["action"], recs[0]["action"])


def test_rollout_policy_validation(device):
    import torch

    from gymca_amd.forest_fire.helicopter import HelicopterPolicy

    E, H, W, K = 2, 5, 7, 3
    env = _env(device, pref.grids(E, H, W, seed=2), 1)
    d = pref.dims(1, 4, 32, H, W)
    pol = _policy(device, d, pref.make_weights(d))
    before = _state(env)
    with pytest.raises(ValueError, match="K >= 0"):
        env.rollout_policy(pol, -1)
    with pytest.raises(ValueError, match="HelicopterPolicy"):
        env.rollout_policy(object(), K)
    with pytest.raises(ValueError, match="grid"):
        env.rollout_policy(HelicopterPolicy((H, W + 1), 1, 4, 32, device=device), K)
    with pytest.raises(ValueError, match="lives on"):
        env.rollout_policy(HelicopterPolicy((H, W), 1, 4, 32, device="cpu"), K)
    with pytest.raises(ValueError, match="unknown records"):
        env.rollout_policy(pol, K, record=("actions",))
    with pytest.raises(ValueError, match="logits_out"):
        env.rollout_policy(pol, K, logits_out=torch.zeros((K, E, 10), dtype=torch.float32, device=device))  # shape
    with pytest.raises(ValueError, match="reward_out"):
        env.rollout_policy(pol, K, reward_out=torch.zeros((K, E), dtype=torch.float32, device=device))     # dtype
    with pytest.raises(ValueError, match="local_out"):
        env.rollout_policy(pol, K, local_out=torch.zeros((K, E, 3, 3), dtype=torch.uint8))                 # device
    with pytest.raises(ValueError, match="w_coarse"):
        pol.w_coarse = torch.zeros((d["C"], 32), dtype=torch.float32)                                      # device
    with pytest.raises(ValueError, match="both local and coarse"):
        env.act(pol, local=torch.zeros((E, 3, 3), dtype=torch.uint8, device=device))
    with pytest.raises(ValueError, match="coarse"):
        env.act(pol, torch.zeros((E, 3, 3), dtype=torch.uint8, device=device),
                torch.zeros((E, 2, 2, 3), dtype=torch.float32, device=device))
    href.assert_states_equal(_state(env), before, "a refused call runs nothing")
    rec = env.rollout_policy(pol, 0)
    assert tuple(rec["logits"].shape) == (0, E, 9) and tuple(rec["local"].shape) == (0, E, 3, 3)
    href.assert_states_equal(_state(env), before, "K = 0")


def test_the_cache_of_bound_policy_calls_is_bounded(device):
    """Many policies against one env do not all stay alive, and one that was dropped is bound again and acts as before."""
    import torch

    from gymca_amd.forest_fire.helicopter import HelicopterPolicy

    E, H, W = 2, 5, 7
    env = _env(device, pref.grids(E, H, W, seed=2), 1)
    d = pref.dims(1, 4, 32, H, W)
    pol = _policy(device, d, pref.make_weights(d))
    lo, co = env.observe(1, 4)   # the rollouts below move the env on: the logits are compared on this observation
    _, l0, _ = env.act(pol, lo, co, seed=1)
    for i in range(env._POLICY_CALLS_MAX + 3):
        env.act(HelicopterPolicy(env, 1, 4, 32, seed=i), seed=1)
        env.rollout_policy(HelicopterPolicy(env, 1, 4, 32, seed=100 + i), 1, record=())
    assert len(env._policy_calls) <= env._POLICY_CALLS_MAX
    assert all(pc[1] is not pol for pc in env._policy_calls.values())
    _, l1, _ = env.act(pol, lo, co, seed=1)
    assert torch.equal(l1, l0)


@pytest.mark.parametrize("shape", bref.TRUNK_SHAPES)
def test_device_trunk_is_one_for_both_agents(device, shape):
    """gca_helicopter_policy_act and gca_bulldozer_policy_act on weights that share the trunk: the same nine logits,
    value and move, bit for bit (both kernels run policy_outputs of gca_policy_dev.h), and both equal the host build."""
    import torch

    from gymca_amd import _device as dev
    from gymca_amd import _lib

    d, wh, wb, local, coarse = bref.trunk_case(shape)
    E = local.shape[0]
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    d_local, d_coarse = up(local), up(coarse)
    d_rs, d_se = up(np.arange(E, dtype=np.int32)), up(np.arange(E, dtype=np.int64))
    got = []
    for w, name, n_act, n_log, key in ((wh, "gca_helicopter_policy_act", 1, 9, (dev.ptr(d_rs),)),
                                       (wb, "gca_bulldozer_policy_act", 2, 11, (dev.ptr(d_se), None))):
        dw = {k: up(v) for k, v in w.items()}
        s = _lib.Policy()
        s.radius, s.block, s.hidden = d["radius"], d["block"], d["hidden"]
        for k, t in dw.items():
            setattr(s, k, t.data_ptr())
        action = torch.full((E, n_act), -7, dtype=torch.int32, device=device)
        logits = torch.full((E, n_log), 5.5, dtype=torch.float32, device=device)
        value = torch.full((E,), 5.5, dtype=torch.float32, device=device)
        _lib.call(name, s, d["C"], dev.ptr(d_local), dev.ptr(d_coarse), *key, 0, 0, 1, dev.ptr(action), dev.ptr(logits),
                  dev.ptr(value), E, dev.stream_ptr(device))
        torch.cuda.synchronize(device)
        got.append((action.cpu().numpy(), logits.cpu().numpy(), value.cpu().numpy()))
    heli, bdz = (got[0][0][:, 0],) + got[0][1:], got[1]
    bref.assert_same_trunk(heli, bdz)
    want = pref.host_act(wh, d, local, coarse, np.arange(E, dtype=np.uint32), greedy=True)
    bref.assert_same_trunk(want, bdz)
