"""GPU: the bulldozer policy inside the env's launches. gca_bulldozer_policy_act on the device against the host build,
and BatchedForestFireBulldozerEnv.rollout_policy / gca_bulldozer_policy_rollout (the resident one-launch kernel, the
K x 3 launch path and the non-fused env's loop) against K eager (observe, act, step) calls on a twin env. Bit for bit:
every record, both grid planes and every state tensor. The eager calls themselves are pinned elsewhere (observe:
tests/test_gpu_policy_obs.py, step / reset: tests/test_gpu_bulldozer_reset.py, act: here against the host build, which
tests/test_bulldozer_policy_host.py pins to the numpy restatement)."""
import numpy as np
import pytest

import _bulldozer_policy_ref as bref
import _policy_obs_ref as obs

pytestmark = pytest.mark.gpu

STATE = ("parity", "pos", "counts", "accu", "done", "hit", "steps", "rng_step", "steps_elapsed", "episode",
         "last_episode_length", "_terminated", "_truncated_u8")
RECORDS = ("action", "logits", "value", "reward", "terminated", "truncated", "local", "coarse")
# (H, W, block): one wave; two waves; three waves with the largest block; 512-wide rows with a strip of the observation
# cut short (48 = 32 + 16); sixteen waves
GRIDS = [(32, 256, 8), (64, 256, 16), (96, 256, 32), (48, 512, 8), (256, 512, 8)]
E = 3
RADIUS = 5
EMPTY_GRID = dict(p_tree=0.0, p_empty=1.0)  # EMPTY but for the one FIRE cell: the fire dies at the first CA pass


def _env(H, W, device, n_envs=E, **kw):
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv

    kw.setdefault("t_move", 0.3)
    kw.setdefault("t_shoot", 0.25)
    return BatchedForestFireBulldozerEnv(n_envs, H, W, device=device, seed=17, materialize_obs=False, **kw)


def _mid_episode(env):
    """Fires sprinkled over both planes, mixed parity, and fractions of time that make env 1 take a CA pass at its first
    step whatever it does (0.9995 + t_any >= 1) while env 0 cannot (0 + 0.551 < 1). Env 0's agent stands in a 3 x 3
    patch of TREE cells: whatever it moves, a shot at its first step hits a tree (_policy makes it shoot there)."""
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    n, H, W = env.num_envs, env.nrows, env.ncols
    rng = np.random.default_rng(11)
    g = env.grids().cpu().numpy()
    g[rng.random(g.shape) < 0.03] = env._fire
    i0, j0 = (int(v) for v in env.pos[0].cpu().numpy())
    assert 1 <= i0 < H - 1 and 1 <= j0 < W - 1
    g[0, i0 - 1:i0 + 2, j0 - 1:j0 + 2] = env._tree
    g = torch.as_tensor(g, device=env.device)
    env.buf[0].copy_(g)
    env.buf[1].copy_(g)
    env.parity.copy_(torch.as_tensor((np.arange(n) % 2).astype(np.uint8), device=env.device))
    env.accu.copy_(torch.as_tensor(np.array([0.0, 0.9995, 0.5, 0.25, 0.75, 0.1])[:n], device=env.device))
    env.steps_elapsed.copy_(torch.as_tensor(np.array([0, 3, 2**32 + 1, 7, 9, 11])[:n], device=env.device))
    call("gca_count_cells", dev.ptr(env.buf[0]), n, H, W, env._empty, env._tree, env._fire, dev.ptr(env.counts),
         dev.stream_ptr(env.device))


def _pair(device, H, W, n=2, prepare=_mid_episode, n_envs=E, **kw):
    envs = [_env(H, W, device, n_envs, **kw) for _ in range(n)]
    for env in envs:
        env.reset(seed=5)
        if prepare is not None:
            prepare(env)
    return envs


def _policy(env, block, hidden, radius=RADIUS, seed=0):
    """Weights with logits a few units apart (varied actions), the shoot head leaning to `shoot`, and hidden unit 0
    rewired: it is 0.5 exactly when the agent's own cell and its eight neighbours are all TREE (nine lookups of 1.0 and a
    bias of -8.5: exact in any summation order) and 0 otherwise, and it moves the shoot logits by -+ 60. So an agent
    standing in a patch of trees shoots for certain (P(no shot) = e^-120 is below the 2^-24 grid of the uniform unless
    the uniform is exactly 0) and hits whatever it moves; everywhere else both heads are sampled as usual."""
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    pol = BulldozerPolicy(env, radius, block, hidden)
    d = bref.dims(radius, block, hidden, env.nrows, env.ncols)
    w = bref.make_weights(d, seed=seed, head=3.0)
    w["b2"][9], w["b2"][10] = -3.0, 3.0
    S = 2 * radius + 1
    w["w_local"][:, :, 0], w["w_coarse"][:, 0], w["b1"][0], w["w_out"][0, :] = 0.0, 0.0, -8.5, 0.0
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            w["w_local"][(radius + di) * S + radius + dj, 1, 0] = 1.0
    w["w_out"][0, 9], w["w_out"][0, 10] = -120.0, 120.0
    return pol.load(w)


def _eager(env, pol, K, seed=3, greedy=False):
    """K x (observe, act, step): the records as rollout_policy defines them, plus each step's env.steps and env.hit."""
    import torch

    rec = {n: [] for n in RECORDS + ("steps", "hit")}
    for _ in range(K):
        lo, co = env.observe(pol.radius, pol.block)
        a, lg, v = env.act(pol, lo, co, seed=seed, greedy=greedy)
        env.step(a)
        for n, t in (("local", lo), ("coarse", co), ("action", a), ("logits", lg), ("value", v), ("reward", env.reward),
                     ("terminated", env._terminated if env.autoreset else env.done),
                     ("truncated", env._truncated_u8 if env.autoreset else torch.zeros_like(env.done)),
                     ("steps", env.steps), ("hit", env.hit)):
            rec[n].append(t.clone())
    return {n: torch.stack(v) for n, v in rec.items()}


def _outputs(env, pol, K):
    """All eight output tensors, filled with values no record holds."""
    import torch

    n = env.num_envs
    S, Hc, Wc = pol.S, pol.Hc, pol.Wc
    new = lambda shape, dtype, fill: torch.full(shape, fill, dtype=dtype, device=env.device)
    return dict(action_out=new((K, n, 2), torch.int32, -7), logits_out=new((K, n, 11), torch.float32, 5.5),
                value_out=new((K, n), torch.float32, 5.5), reward_out=new((K, n), torch.float64, 5.5),
                terminated_out=new((K, n), torch.uint8, 7), truncated_out=new((K, n), torch.uint8, 7),
                local_out=new((K, n, S, S), torch.uint8, 9), coarse_out=new((K, n, 2, Hc, Wc), torch.float32, 5.5))


def _same(x, y):
    import torch

    if x.is_floating_point():  # NaN where NaN, equal bits elsewhere
        return torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))
    return torch.equal(x, y)


def _assert_envs_equal(a, b, where=""):
    import torch

    torch.cuda.synchronize(a.device)
    assert torch.equal(a.buf, b.buf), f"{where}: buf (both planes)"
    for k in STATE:
        assert torch.equal(getattr(a, k), getattr(b, k)), f"{where}: {k}"
    assert _same(a.reward, b.reward), f"{where}: reward"


def _assert_records_equal(want, got, where=""):
    for n in RECORDS:
        assert want[n].shape == got[n].shape and want[n].dtype == got[n].dtype, f"{where}: {n} shape / dtype"
        assert _same(want[n], got[n]), f"{where}: record {n} differs"


def _assert_exercised(want, ca=True, hit=True):
    """The expected (K x 3) run itself took env steps with and without a CA pass and Modify hit at least once: an
    input that never exercises them fails here instead of passing vacuously."""
    if ca:
        assert (want["steps"] > 0).any() and (want["steps"] == 0).any(), want["steps"]
    if hit:
        assert (want["hit"] != 0).any(), want["hit"]


# ------------------------------------------------------------------ act
@pytest.mark.parametrize("shape", bref.SHAPES)
def test_act_on_the_device_equals_the_host_build(device, shape):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd import _lib

    r, B, Hd, H, W = shape
    n = 4
    d = bref.dims(*shape)
    w = bref.make_weights(d, seed=Hd, head=3.0)
    buf, parity, _ = obs.make_case(n, H, W, B)
    local, coarse = obs.host_observe(buf, parity, obs.positions(n, H, W), obs.CODES, r, B)
    se = np.array([3, 17, 2**32 + 5, 250], np.int64)
    ep = np.array([1, 2, 7, 0xFFFFFFFF], np.uint32)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    dw = {k: up(v) for k, v in w.items()}
    s = _lib.BulldozerPolicyStruct()
    s.radius, s.block, s.hidden = r, B, Hd
    for k, t in dw.items():
        setattr(s, k, t.data_ptr())
    d_local, d_coarse, d_se, d_ep = up(local), up(coarse), up(se), up(ep.view(np.int32))
    for greedy in (0, 1):
        for ep_host, ep_dev in ((ep, d_ep), (None, None)):
            want = bref.host_act(w, d, local, coarse, se, ep_host, env_offset=5, seed=99, greedy=bool(greedy))
            action = torch.full((n, 2), -7, dtype=torch.int32, device=device)
            logits = torch.full((n, 11), 5.5, dtype=torch.float32, device=device)
            value = torch.full((n,), 5.5, dtype=torch.float32, device=device)
            _lib.call("gca_bulldozer_policy_act", s, d["C"], dev.ptr(d_local), dev.ptr(d_coarse), dev.ptr(d_se),
                      None if ep_dev is None else dev.ptr(ep_dev), 5, 99, greedy, dev.ptr(action), dev.ptr(logits),
                      dev.ptr(value), n, dev.stream_ptr(device))
            torch.cuda.synchronize(device)
            assert np.array_equal(logits.cpu().numpy().view(np.uint32), want[1].view(np.uint32)), "logits"
            assert np.array_equal(value.cpu().numpy().view(np.uint32), want[2].view(np.uint32)), "value"
            assert np.array_equal(action.cpu().numpy(), want[0]), "action"
    # the nullable outputs
    action2 = torch.full((n, 2), -7, dtype=torch.int32, device=device)
    _lib.call("gca_bulldozer_policy_act", s, d["C"], dev.ptr(d_local), dev.ptr(d_coarse), dev.ptr(d_se), None, 5, 99, 1,
              dev.ptr(action2), None, None, n, dev.stream_ptr(device))
    assert torch.equal(action2, action)


# ------------------------------------------------------------------ rollout_policy against K x (observe, act, step)
@pytest.mark.parametrize("hidden", [32, 256])
@pytest.mark.parametrize("K", [1, 7, 40])
@pytest.mark.parametrize("H,W,block", GRIDS)
def test_rollout_policy_equals_k_observe_act_step(device, H, W, block, K, hidden):
    eager, roll = _pair(device, H, W)
    pol = _policy(eager, block, hidden)
    want = _eager(eager, pol, K)
    got = roll.rollout_policy(pol, K, seed=3, **_outputs(roll, pol, K))
    assert set(got) == set(RECORDS)
    _assert_envs_equal(eager, roll, "after the rollout")
    _assert_records_equal(want, got, "rollout")
    # at every K: env 1 takes a pass at its first step and env 0 cannot, and env 0's first shot hits (_mid_episode)
    _assert_exercised(want)
    assert int(want["action"][0, 0, 1]) == 1 and int(want["hit"][0, 0]) == 1
    assert int(roll.steps_elapsed[2]) > 2**32   # the draw's key takes the low 32 bits of a counter beyond them
    if K > 1:
        assert len(np.unique(got["action"][..., 0].cpu().numpy())) > 1


@pytest.mark.parametrize("grid_kw", [{}, EMPTY_GRID], ids=["forest", "empty"])
@pytest.mark.parametrize("H,W,block", GRIDS)
def test_rollout_policy_with_autoreset(device, H, W, block, grid_kw):
    """autoreset with a time limit of 5 steps, K = 12: every env resets at least twice; on the empty grid the fire dies
    at the first CA pass, so episodes terminate. Row k + 1 after a reset is the new episode's observation."""
    K = 12
    prepare = None if grid_kw else _mid_episode
    eager, roll = _pair(device, H, W, prepare=prepare, autoreset=True, max_episode_steps=5, **grid_kw)
    pol = _policy(eager, block, 64)
    want = _eager(eager, pol, K)
    got = roll.rollout_policy(pol, K, seed=3, **_outputs(roll, pol, K))
    _assert_envs_equal(eager, roll, "after the rollout")
    _assert_records_equal(want, got, "rollout")
    ended = (want["terminated"] | want["truncated"]).cpu().numpy()
    assert (ended.sum(0) >= 2).all(), ended
    assert (eager.episode.cpu().numpy() >= 2).all()
    if grid_kw:
        assert want["terminated"].any(), "no termination on the K x 3 path"
    else:
        assert want["truncated"].any()
        _assert_exercised(want, hit=False)
    # the observation after an episode's end is the new episode's: it differs from a run without the reset only
    # through the reset, and it equals the eager observe() of the reset state (compared above); spot-check one row
    k, e = [int(v[0]) for v in np.nonzero(ended[:-1])]
    assert not _same(got["coarse"][k + 1, e], got["coarse"][k, e]) or grid_kw


def test_a_done_env_without_autoreset_repeats_the_noop(device):
    """Env 0 starts without a fire: done at step 0, then the no-op step, K - 1 times, observed, acted on and recorded."""
    import torch

    H, W, block, K = 32, 256, 8, 6
    grids = np.full((E, H, W), 3, np.uint8)
    grids[1:, 20, 100] = 25
    positions = np.array([[5, 5], [10, 200], [31, 255]])
    envs = [_env(H, W, device) for _ in range(2)]
    for env in envs:
        env.reset(seed=5, grids=grids, positions=positions)
    eager, roll = envs
    pol = _policy(eager, block, 64)
    want = _eager(eager, pol, K)
    got = roll.rollout_policy(pol, K, seed=3, **_outputs(roll, pol, K))
    _assert_envs_equal(eager, roll, "after the rollout")
    _assert_records_equal(want, got, "rollout")
    term, rew = got["terminated"].cpu().numpy(), got["reward"].cpu().numpy()
    assert (term[:, 0] == 1).all() and (term[:, 1:] == 0).all(), term
    assert (rew[1:, 0] == 0.0).all() and (rew[:, 1:] != 0.0).all(), rew
    assert not got["truncated"].any()
    for k in range(2, K):  # steps_elapsed stays at 1: the same key, the same action; nothing moves, the same observation
        for n in ("action", "logits", "value", "local", "coarse"):
            assert _same(got[n][k, 0], got[n][1, 0]), (n, k)
    assert int(roll.steps_elapsed[0]) == 1 and (roll.steps_elapsed[1:].cpu().numpy() == K).all()


@pytest.mark.parametrize("H,W", [(64, 256), (256, 512)])
def test_the_in_launch_modify_is_seen_by_the_next_step(device, H, W):
    """From first principles, no reference run: a greedy policy that never moves and shoots exactly when the window's
    centre is a TREE, the agent on the grid's only tree, timings too small for a CA pass in three steps. Two and sixteen
    waves: thread 0 (wave 0) writes the Modify byte and adjusts the coarse map, while the window's centre cell is
    gathered by virtual threads 96..103 (radius 2, 32 hidden units: eight threads per weight row, 32 groups, cell 12 in
    group 12), which another wave runs, and the coarse map is read by every wave."""
    import torch

    block, K, r, hidden = 8, 3, 2, 32
    n_envs = 2
    positions = np.array([[13, 200], [24, 7]])
    grids = np.zeros((n_envs, H, W), np.uint8)
    grids[:, 2, 2] = 25                       # a fire far from the agent: the env is not done
    for e, (i, j) in enumerate(positions):
        grids[e, i, j] = 3                    # the only tree, under the agent
    env = _env(H, W, device, n_envs, t_move=0.001, t_shoot=0.001)
    env.reset(seed=5, grids=grids, positions=positions)
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    pol = BulldozerPolicy(env, r, block, hidden)
    S = pol.S
    w = {k: np.zeros(v, np.float32) for k, v in pol.weight_shapes().items()}
    w["b2"][4] = 1.0                               # move: not_move
    w["w_local"][(S * S) // 2, 1, 0] = 1.0         # unit 0 is 1 exactly when the centre cell is a TREE
    w["w_out"][0, 10] = 1.0                        # shoot logit 1 = unit 0
    w["b2"][9] = 0.5                               # shoot logit 0
    pol.load(w)
    got = env.rollout_policy(pol, K, greedy=True, **_outputs(env, pol, K))
    torch.cuda.synchronize(device)
    assert int(env.steps.max()) == 0 and (env.rng_step == 0).all()      # no CA pass occurred
    action = got["action"].cpu().numpy()
    assert (action[..., 0] == 4).all()
    assert (action[..., 1] == np.array([1, 0, 0])[:, None]).all(), action[..., 1]
    local, coarse = got["local"].cpu().numpy(), got["coarse"].cpu().numpy()
    assert (local[0, :, r, r] == 1).all() and (local[1, :, r, r] == 0).all() and (local[2, :, r, r] == 0).all()
    inv = np.float32(1.0 / (block * block))
    for e, (i, j) in enumerate(positions):
        expect = coarse[0, e].copy()
        assert expect[0, i // block, j // block] == inv and expect[0].sum() == inv
        expect[0, i // block, j // block] -= inv
        assert np.array_equal(coarse[1, e], expect) and np.array_equal(coarse[2, e], expect)
        assert coarse[1, e][0].sum() == 0.0 and coarse[1, e][1, 0, 0] == inv        # the fire's block is untouched
    assert (env.hit.cpu().numpy() == 0).all() and (env.counts[:, 1] == 0).all()    # the tree is gone, the last step missed


def test_state_carries_across_calls(device):
    import torch

    H, W, block = 64, 256, 16
    eager, roll = _pair(device, H, W)
    pol = _policy(eager, block, 64)
    rng = np.random.default_rng(2)
    one = torch.as_tensor(np.array([[1, 1], [7, 0], [4, 1]], np.int32), device=device)
    acts = torch.as_tensor(np.stack([rng.integers(0, 9, (4, E)), rng.integers(0, 2, (4, E))], 2).astype(np.int32),
                           device=device)
    w1 = _eager(eager, pol, 7)
    eager.step(one)
    for k in range(4):
        eager.step(acts[k])
    w2 = _eager(eager, pol, 5)
    g1 = roll.rollout_policy(pol, 7, seed=3)
    roll.step(one)
    roll.rollout(acts)
    g2 = roll.rollout_policy(pol, 5, seed=3)
    _assert_envs_equal(eager, roll, "after the sequence")
    _assert_records_equal(w1, g1, "first rollout")
    _assert_records_equal(w2, g2, "second rollout")
    _assert_exercised({k: torch.cat([w1[k], w2[k]]) for k in ("steps", "hit")}, hit=False)


def test_two_shards_equal_the_joint_env(device):
    import torch

    H, W, block, K = 32, 256, 8, 9
    joint = _env(H, W, device, 4, autoreset=True, max_episode_steps=4)
    shards = [_env(H, W, device, 2, env_offset=off, autoreset=True, max_episode_steps=4) for off in (0, 2)]
    for env in [joint] + shards:
        env.reset(seed=5)
    pol = _policy(joint, block, 64)
    want = joint.rollout_policy(pol, K, seed=3)
    for i, sh in enumerate(shards):
        got = sh.rollout_policy(pol, K, seed=3)
        torch.cuda.synchronize(device)
        sl = slice(2 * i, 2 * i + 2)
        for n in RECORDS:
            assert _same(got[n], want[n][:, sl].contiguous()), f"shard {i}: record {n}"
        assert torch.equal(sh.buf, joint.buf[:, sl]), f"shard {i}: buf"
        for k in STATE:
            assert torch.equal(getattr(sh, k), getattr(joint, k)[sl]), f"shard {i}: {k}"
    assert (joint.episode.cpu().numpy() >= 2).all()


def test_graph_capture_replays_the_eager_call(device):
    import torch

    H, W, block, K = 64, 256, 16, 10
    eager, roll = _pair(device, H, W, autoreset=True, max_episode_steps=4)
    pol = _policy(eager, block, 64)
    want = eager.rollout_policy(pol, K, seed=3, **_outputs(eager, pol, K))
    names = ("buf", "reward") + STATE
    start = {n: getattr(roll, n).clone() for n in names}
    outs = _outputs(roll, pol, K)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        roll.rollout_policy(pol, K, seed=3, **outs)  # binds the call and allocates its scratch outside the capture
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        roll.rollout_policy(pol, K, seed=3, **outs)
    for n in names:  # back to the start state, in place: the graph holds the tensors' addresses
        getattr(roll, n).copy_(start[n])
    for t in outs.values():
        t.fill_(1)
    graph.replay()
    _assert_envs_equal(eager, roll, "after the replay")
    _assert_records_equal(want, {n: outs[n + "_out"] for n in RECORDS}, "replay")


# ------------------------------------------------------------------ the other paths
@pytest.mark.parametrize("H,W,block,autoreset", [(32, 256, 4, False), (40, 256, 16, True), (48, 512, 64, False)])
def test_shapes_off_the_resident_path_take_the_launch_path(device, H, W, block, autoreset):
    """block 4, H % block != 0 and block 64 are not shapes of the observation's rows form: K x 3 (+ reset) launches inside
    gca_bulldozer_policy_rollout, with all records, with none (everything through `scratch`) and with some."""
    K = 9
    kw = dict(autoreset=True, max_episode_steps=4) if autoreset else {}
    eager, full, none, some = _pair(device, H, W, n=4, **kw)
    pol = _policy(eager, block, 64)
    want = _eager(eager, pol, K)
    got = full.rollout_policy(pol, K, seed=3, **_outputs(full, pol, K))
    _assert_envs_equal(eager, full, "all records")
    _assert_records_equal(want, got, "all records")
    _assert_exercised(want, hit=False)
    assert none.rollout_policy(pol, K, seed=3, record=()) == {}
    _assert_envs_equal(eager, none, "no records")
    part = some.rollout_policy(pol, K, seed=3, record=("value", "truncated", "coarse"))
    assert set(part) == {"value", "truncated", "coarse"}
    _assert_envs_equal(eager, some, "three records")
    for n in part:
        assert _same(part[n], want[n]), n


def test_resident_path_with_some_and_no_records(device):
    H, W, block, K = 64, 256, 16, 9
    eager, none, some = _pair(device, H, W, n=3)
    pol = _policy(eager, block, 64)
    want = _eager(eager, pol, K)
    assert none.rollout_policy(pol, K, seed=3, record=()) == {}
    _assert_envs_equal(eager, none, "no records")
    part = some.rollout_policy(pol, K, seed=3, record=("action", "terminated", "local"))
    _assert_envs_equal(eager, some, "three records")
    for n in part:
        assert _same(part[n], want[n]), n
    k0 = none.rollout_policy(pol, 0, seed=3)
    assert k0["action"].shape == (0, E, 2)
    _assert_envs_equal(eager, none, "K = 0 changes nothing")


def test_a_non_fused_env_runs_observe_act_step(device):
    H, W, block, K = 24, 64, 8, 8
    eager, roll = _pair(device, H, W, autoreset=True, max_episode_steps=5)
    assert not roll.fused
    pol = _policy(eager, block, 32, radius=3)
    want = _eager(eager, pol, K)
    got = roll.rollout_policy(pol, K, seed=3, **_outputs(roll, pol, K))
    _assert_envs_equal(eager, roll, "after the rollout")
    _assert_records_equal(want, got, "rollout")
    part = eager.rollout_policy(pol, 3, seed=4, record=("reward",))
    assert set(part) == {"reward"} and part["reward"].shape == (3, E)


# ------------------------------------------------------------------ other cell codes and effects (the ABI's other instantiations)
CODES = (0, 2, 9)


def _coded_envs(device, H, W, chain, n=2):
    """tests/test_gpu_bulldozer_codes.py's construction: envs with private codes (0, 2, 9) set before reset() -- the
    STD = false instantiations -- and, with `chain`, the effect {TREE: FIRE, FIRE: EMPTY}, whose Modify changes the FIRE
    count (the kernel's barrier-per-step instantiation). Every call the env makes is the C ABI's with these params."""
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    empty, tree, fire = CODES
    rng = np.random.default_rng(3)
    sprinkle = rng.random((E, H, W)) < 0.04
    envs = []
    for _ in range(n):
        env = _env(H, W, device, p_tree=0.6, p_empty=0.4)
        env._tree, env._fire = tree, fire
        p = env.params
        p.tree, p.fire = tree, fire
        p.effect[3] = -1
        p.effect[tree] = fire if chain else empty
        if chain:
            p.effect[fire] = empty
        env.reset(seed=4)
        g = env.grids()
        assert set(torch.unique(g).tolist()) == {empty, tree, fire}
        g[torch.as_tensor(sprinkle, device=device)] = fire
        env.buf[0].copy_(g)
        env.buf[1].copy_(g)
        env.accu.copy_(torch.as_tensor(np.array([0.0, 0.9995, 0.5]), device=device))
        call("gca_count_cells", dev.ptr(env.buf[0]), E, H, W, empty, tree, fire, dev.ptr(env.counts),
             dev.stream_ptr(device))
        envs.append(env)
    return envs


@pytest.mark.parametrize("chain", [False, True])
@pytest.mark.parametrize("H,W,block", [(40, 256, 8), (48, 512, 16)])
def test_other_codes_and_an_effect_that_touches_fire(device, H, W, block, chain):
    K = 16
    eager, roll = _coded_envs(device, H, W, chain)
    pol = _policy(eager, block, 64)
    want = _eager(eager, pol, K)
    got = roll.rollout_policy(pol, K, seed=3, **_outputs(roll, pol, K))
    _assert_envs_equal(eager, roll, "after the rollout")
    _assert_records_equal(want, got, "rollout")
    _assert_exercised(want)
    assert (want["local"] == 2).any() and (want["coarse"][:, :, 1] > 0).any()   # FIRE seen under its private code


# ------------------------------------------------------------------ validation
def test_validation_raises_before_any_launch(device):
    import torch

    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy
    from gymca_amd.forest_fire.helicopter import HelicopterPolicy

    H, W = 32, 256
    env, = _pair(device, H, W, n=1)
    pol = _policy(env, 8, 32)
    before = {n: getattr(env, n).clone() for n in ("buf", "reward") + STATE}
    bad = [
        (dict(policy=HelicopterPolicy((H, W), 2, 8, 32, device=device)), "BulldozerPolicy"),
        (dict(policy=object()), "BulldozerPolicy"),
        (dict(policy=BulldozerPolicy((H, 512), 2, 8, 32, device=device)), "grid"),
        (dict(policy=BulldozerPolicy((H, W), 2, 8, 32, device="cpu")), "lives on"),
        (dict(K=-1), "K >= 0"),
        (dict(record=("action", "hit")), "unknown records"),
        (dict(logits_out=torch.zeros((4, E, 11), dtype=torch.float64, device=device)), "logits_out"),
        (dict(logits_out=torch.zeros((4, E, 9), dtype=torch.float32, device=device)), "logits_out"),
        (dict(action_out=torch.zeros((4, E), dtype=torch.int32, device=device)), "action_out"),
        (dict(terminated_out=torch.zeros((4, E), dtype=torch.bool, device=device)), "terminated_out"),
        (dict(coarse_out=torch.zeros((4, E, 2, 4, 32), dtype=torch.float32)), "coarse_out"),
        (dict(local_out=torch.zeros((4, E, 11, 12), dtype=torch.uint8, device=device)[..., :11]), "local_out"),
    ]
    for over, msg in bad:
        kw = dict(policy=pol, K=4)
        kw.update(over)
        with pytest.raises(ValueError, match=msg):
            env.rollout_policy(kw.pop("policy"), kw.pop("K"), **kw)
    with pytest.raises(ValueError, match="BulldozerPolicy"):
        env.act(object())
    with pytest.raises(ValueError, match="both local and coarse"):
        env.act(pol, local=torch.zeros((E, 11, 11), dtype=torch.uint8, device=device))
    with pytest.raises(ValueError, match="action_out"):
        env.act(pol, action_out=torch.zeros((E,), dtype=torch.int32, device=device))
    torch.cuda.synchronize(device)
    for n, t in before.items():
        assert _same(getattr(env, n), t), n
    # a replaced policy tensor is bound again: the new weights act
    a0, l0, _ = env.act(pol, seed=1)
    pol.b2 = pol.b2 + 1.0
    _, l1, _ = env.act(pol, seed=1)
    assert torch.allclose(l1, l0 + 1.0, atol=1e-5) and not torch.equal(l1, l0)
    # the env's cache of bound calls is bounded: many policies against one env do not all stay alive, and one that was
    # dropped is bound again and acts as before
    for i in range(env._POLICY_CALLS_MAX + 3):
        env.act(BulldozerPolicy(env, 2, 8, 32, seed=i), seed=1)
    assert len(env._policy_calls) <= env._POLICY_CALLS_MAX
    _, l2, _ = env.act(pol, seed=1)
    assert torch.equal(l2, l1)
