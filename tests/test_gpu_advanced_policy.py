"""GPU: the bulldozer agent on the Advanced bulldozer env. gca_advanced_policy_act (observe and act in one launch) against
the two launches it is defined by, the host build and the numpy restatements, bit for bit; then the env's policy_act /
rollout_policy against the hand-written loop of public calls, as a graph, through the learner, and the training script."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _advanced_policy_ref as aref
import _bulldozer_policy_ref as bref
import _ppo_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

# (E, H, W, block, radius, hidden), plane offset in bytes
CASES = [((3, 32, 256, 8, 5, 64), 0),     # one strip
         ((2, 48, 256, 16, 0, 32), 0),    # a strip cut short; S = 1
         ((2, 64, 256, 32, 31, 256), 0),  # window taller than the grid; a strip per wave; the widest layer
         ((3, 32, 512, 8, 5, 64), 0),     # NW = 2, one lane per tile, no DPP sum
         ((2, 64, 512, 32, 2, 128), 0),
         ((5, 160, 256, 8, 5, 64), 0),    # five strips over four waves: a wave takes two
         ((2, 24, 40, 4, 3, 32), 0),      # generic form
         ((3, 32, 256, 8, 5, 64), 4)]     # a plane offset by 4 bytes: the unaligned route to the generic form
STATE = ("pos", "accu", "wind_index", "time_step", "is_night", "rng_step", "counts", "dousing", "steps_elapsed",
         "reward_accumulated", "reward", "done")


def _policy(device, d, w):
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    return BulldozerPolicy((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device=device).load(w)


def _device_case(device, shape, offset):
    """The shared case on the device: (d, w, policy, planes (E, H, W) u8 at `offset` bytes into its allocation, pos,
    ts, host arrays)."""
    import torch

    d, w, planes, pos, ts = aref.make_case(shape)
    E, H, W = planes.shape
    store = torch.zeros(E * H * W + 16, dtype=torch.uint8, device=device)
    assert store.data_ptr() % 16 == 0
    view = store[offset:offset + E * H * W].view(E, H, W)
    view.copy_(torch.from_numpy(planes))
    assert view.data_ptr() % 8 == offset % 8 and view.is_contiguous()
    return (d, w, _policy(device, d, w), view, torch.from_numpy(pos).to(device), torch.from_numpy(ts).to(device),
            (planes, pos, ts))


def _outputs(device, d, E, stride=2):
    import torch

    kw = dict(device=device)
    return dict(action=torch.full((E, stride), aref.SENTINEL, dtype=torch.int32, **kw),
                logits=torch.full((E, 11), float("nan"), **kw), value=torch.full((E,), float("nan"), **kw),
                local=torch.full((E, d["S"], d["S"]), 0xAA, dtype=torch.uint8, **kw),
                coarse=torch.full((E, 2, d["Hc"], d["Wc"]), -1.0, **kw))


def _fused(device, pol, planes, pos, ts, o, greedy, env_offset=5, null=()):
    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    E, H, W = planes.shape
    p = lambda n: None if n in null else o[n].data_ptr()
    call("gca_advanced_policy_act", pol.struct, planes.data_ptr(), pos.data_ptr(), ts.data_ptr(), E, H, W, *aref.CODES,
         env_offset, aref.SEED, 1 if greedy else 0, o["action"].data_ptr(), int(o["action"].shape[1]), p("logits"),
         p("value"), p("local"), p("coarse"), dev.stream_ptr(device))


def _pair(device, pol, planes, pos, ts, o, greedy, env_offset=5):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    E, H, W = planes.shape
    st = dev.stream_ptr(device)
    call("gca_policy_observation", planes.data_ptr(), None, None, pos.data_ptr(), E, H, W, *aref.CODES, pol.radius,
         pol.block, 0, o["local"].data_ptr(), o["coarse"].data_ptr(), st)
    se = ts.to(torch.int64)
    call("gca_bulldozer_policy_act", pol.struct, pol.C, o["local"].data_ptr(), o["coarse"].data_ptr(), se.data_ptr(),
         None, env_offset, aref.SEED, 1 if greedy else 0, o["action"].data_ptr(), o["logits"].data_ptr(),
         o["value"].data_ptr(), E, st)


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("shape, offset", CASES)
def test_fused_launch_equals_the_pair(device, shape, offset, greedy):
    import torch

    d, w, pol, planes, pos, ts, _ = _device_case(device, shape, offset)
    E = planes.shape[0]
    a, b = _outputs(device, d, E), _outputs(device, d, E)
    _fused(device, pol, planes, pos, ts, a, greedy)
    _pair(device, pol, planes, pos, ts, b, greedy)
    torch.cuda.synchronize(device)
    for name in ("local", "coarse", "logits", "value", "action"):
        assert torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)), name
    assert (a["local"] == 3).any() and bool(torch.isfinite(a["logits"]).all())
    if d["radius"] > 0:
        assert (a["local"] != 3).any()
    # the nullable outputs change nothing else; a third action column stays the caller's
    c = _outputs(device, d, E, stride=3)
    _fused(device, pol, planes, pos, ts, c, greedy, null=("logits", "value", "local", "coarse"))
    assert torch.equal(c["action"][:, :2], a["action"]) and bool((c["action"][:, 2] == aref.SENTINEL).all())
    assert bool(torch.isnan(c["logits"]).all()) and bool((c["local"] == 0xAA).all()) and bool((c["coarse"] == -1).all())


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
def test_device_equals_the_host_build_and_the_restatements(device, greedy):
    d, w, pol, planes, pos, ts, (h_planes, h_pos, h_ts) = _device_case(device, CASES[0][0], 0)
    o = _outputs(device, d, planes.shape[0])
    _fused(device, pol, planes, pos, ts, o, greedy)
    got = {k: v.cpu().numpy() for k, v in o.items()}
    host = dict(zip(("action", "logits", "value", "local", "coarse"),
                    aref.host_act(d, w, h_planes, h_pos, h_ts, env_offset=5, greedy=greedy)))
    for name in got:
        assert np.array_equal(got[name].view(np.uint8), host[name].view(np.uint8)), name
    want_a, want_l, want_v, want_lo, want_co, out32 = aref.composed(d, w, h_planes, h_pos, h_ts, env_offset=5,
                                                                    greedy=greedy)
    assert np.array_equal(got["local"], want_lo) and np.array_equal(aref.bits(got["coarse"]), aref.bits(want_co))
    assert np.array_equal(aref.bits(got["logits"]), aref.bits(out32[:, :11]))
    assert np.array_equal(aref.bits(got["value"]), aref.bits(out32[:, 11]))
    assert np.array_equal(got["action"], want_a)


# ------------------------------------------------------------------ the env
def _env(device, E=3, ext=False, key=7):
    from gymca_amd.forest_fire.bulldozer import AdvancedForestFireBulldozerEnv

    env = AdvancedForestFireBulldozerEnv(32, 256, key=key, num_envs=E, device=device, observation="grid",
                                         hidden_rng="philox", enable_extensions=ext)
    env.reset()
    # env 1 has no fire left: its first step ends the episode, so a reset falls inside the K steps
    g = env.grid[env.cur].clone()
    g[1][g[1] == env._fire] = env._tree
    age = env.age[env.cur].clone()
    age[1] = 0
    env.set_state(grid=g, fire_age=age)
    return env


def _env_policy(env, seed=3):
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    d = bref.dims(5, 8, 64, env.nrows, env.ncols)
    return BulldozerPolicy(env, 5, 8, 64).load(bref.make_weights(d, seed=seed, head=2.0))


def _assert_same_state(a, b):
    import torch

    assert a.cur == b.cur
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.grid[a.cur], b.grid[b.cur]) and torch.equal(a.age[a.cur], b.age[b.cur])


def _hand_loop(env, pol, K, seed, extension=None):
    """K x (policy_act(fused=False) -> step -> record -> conditional_reset) in public calls; the records as rollout_policy
    lays them out."""
    import torch

    rows = {k: [] for k in env._POLICY_RECORDS}
    E = env.num_envs
    for _ in range(K):
        action = torch.zeros((E, 2 if extension is None else 3), dtype=torch.int32, device=env.device)
        if extension is not None:
            action[:, 2] = extension
        ls, cs = env.policy_record_shapes(pol, 1)["local"][1][1:], env.policy_record_shapes(pol, 1)["coarse"][1][1:]
        lo = torch.empty(ls, dtype=torch.uint8, device=env.device)
        co = torch.empty(cs, dtype=torch.float32, device=env.device)
        _, logits, value = env.policy_act(pol, seed=seed, action_out=action, local_out=lo, coarse_out=co, fused=False)
        env.step(action)
        rows["action"].append(action[:, :2].clone())
        rows["logits"].append(logits)
        rows["value"].append(value)
        rows["local"].append(lo)
        rows["coarse"].append(co)
        rows["reward"].append(env.reward.to(torch.float64))
        rows["terminated"].append(env.done.clone())
        rows["truncated"].append(torch.zeros(E, dtype=torch.uint8, device=env.device))
        env.conditional_reset()
    return {k: torch.stack(v) for k, v in rows.items()}


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "extensions"])
def test_rollout_policy_equals_the_hand_written_loop(device, ext):
    import torch

    K = 6
    env, twin = _env(device, ext=ext), _env(device, ext=ext)
    _assert_same_state(env, twin)
    pol = _env_policy(env)
    # policy_act() touches no state: twice without a step, the same action; fused and the pair agree
    a1, l1, v1 = env.policy_act(pol, seed=11)
    a2, l2, v2 = env.policy_act(pol, seed=11)
    a3, l3, v3 = env.policy_act(pol, seed=11, fused=False)
    assert torch.equal(a1, a2) and torch.equal(l1, l2) and torch.equal(v1, v2)
    assert torch.equal(a1, a3) and torch.equal(l1, l3) and torch.equal(v1, v3)
    _assert_same_state(env, twin)
    rec = env.rollout_policy(pol, K, seed=11, extension=1 if ext else 0)
    want = _hand_loop(twin, pol, K, 11, extension=1 if ext else None)
    spec = env.policy_record_shapes(pol, K)
    assert set(rec) == set(want) == set(spec)
    for name, (dtype, shape) in spec.items():
        assert rec[name].dtype is dtype and tuple(rec[name].shape) == shape, name
        assert torch.equal(rec[name].view(torch.uint8), want[name].contiguous().view(torch.uint8)), name
    _assert_same_state(env, twin)
    term = rec["terminated"].cpu().numpy()
    assert term[0, 1] == 1 and term.sum() < term.size  # the reset fell inside the K steps
    assert not rec["truncated"].any()
    assert rec["reward"].dtype is torch.float64 and len(torch.unique(rec["action"][..., 0])) > 1
    # the step after the reset observes the new episode: its fire is back in the coarse map
    assert float(rec["coarse"][0, 1, 1].sum()) == 0.0 and float(rec["coarse"][1, 1, 1].sum()) > 0.0


def test_rollout_policy_as_a_graph(device):
    import torch

    K = 4
    env, twin = _env(device), _env(device)
    pol = _env_policy(env)
    outs = {f"{k}_out": torch.empty(s, dtype=t, device=device) for k, (t, s) in env.policy_record_shapes(pol, K).items()}
    env.rollout_policy(pol, K, seed=11, **outs)  # warms the bound calls; the capture itself runs nothing
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        env.rollout_policy(pol, K, seed=11, **outs)
    graph.replay()
    graph.replay()
    for _ in range(3):
        want = twin.rollout_policy(pol, K, seed=11)
    torch.cuda.synchronize(device)
    for name, t in want.items():
        assert torch.equal(outs[f"{name}_out"].view(torch.uint8), t.view(torch.uint8)), name
    _assert_same_state(env, twin)
    assert int(env.time_step[0]) == 1 + 3 * K  # kept across the reset: the draw's key never repeats
    scratch = torch.zeros(4, device=device)
    with pytest.raises(ValueError, match="even K"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            scratch.add_(1.0)
            env.rollout_policy(pol, 3, seed=11)


def test_records_feed_the_learner(device):
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    E, K = 4, 8
    env = _env(device, E=E)
    d = bref.dims(5, 8, 64, env.nrows, env.ncols)
    w = bref.make_weights(d, seed=3, head=2.0)
    pol = BulldozerPolicy(env, 5, 8, 64).load(w)
    rec = env.rollout_policy(pol, K, seed=11)
    _, _, next_value = env.policy_act(pol, seed=11)
    adv, ret = ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95, terminal=rec["terminated"])
    host = {k: v.cpu().numpy() for k, v in rec.items()}
    want_a, want_r = R.host_gae(host["reward"], host["value"], next_value.cpu().numpy(), host["terminated"], 0.99, 0.95)
    assert np.array_equal(aref.bits(adv.cpu().numpy()), aref.bits(want_a))
    assert np.array_equal(aref.bits(ret.cpu().numpy()), aref.bits(want_r))
    # ppo_grad on the device against the device="cpu" policy's host build, to test_gpu_bulldozer_ppo.py's tolerance
    grads, stats = pol.ppo_grad(rec, adv, ret)
    cpu = BulldozerPolicy((env.nrows, env.ncols), 5, 8, 64, device="cpu").load(w)
    gh, sh = cpu.ppo_grad({k: v.cpu() for k, v in rec.items()}, adv.cpu(), ret.cpu())
    rows = np.arange(K * E)
    g64, s64, _, _ = R.loss_and_grad(w, d, host, want_a, want_r, rows, R.BDZ.heads)
    g32, s32, _, _ = R.loss_and_grad(w, d, host, want_a, want_r, rows, R.BDZ.heads, dtype="float32")
    e = R.errors({k: v.cpu().numpy() for k, v in grads.items()}, stats.cpu().numpy(),
                 {k: v.numpy().astype(np.float64) for k, v in gh.items()}, sh.numpy().astype(np.float64))
    e32 = R.errors(g32, s32, g64, s64)
    keep = ("loss", "v_loss", "entropy", "adv_mean", "adv_std", "b2", "w_out")  # w_local / w_coarse / b1: relu kinks
    R.assert_within({k: e[k] for k in keep}, e32, "advanced env, device vs host")
    # one update, 2 x 2 minibatches: finite statistics, every tensor moves
    opt = ppo.Adam({n: getattr(pol, n) for n in WEIGHTS}, lr=1e-3)
    before = {n: t.clone() for n, t in pol.state_dict().items()}
    st, info = pol.ppo_update(opt, rec, adv, ret, epochs=2, minibatches=2, seed=7)
    assert tuple(st.shape) == (4, 8) and bool(torch.isfinite(st).all()) and bool(torch.isfinite(info).all())
    for n, t in pol.state_dict().items():
        assert bool(torch.isfinite(t).all()) and not torch.equal(t, before[n]), n


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_training_script_runs(graph):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_advanced_ppo.py"), "--envs", "4", "--rows", "32",
           "--cols", "256", "--steps", "8", "--iterations", "2"] + (["--graph"] if graph else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    assert out.stdout.count("iteration ") == 2
