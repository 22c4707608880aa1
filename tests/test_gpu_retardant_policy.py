"""GPU: the bulldozer agent that sees the retardant on the Advanced bulldozer env. gca_advanced_policy_observation against
the host build and the numpy restatement (tests/_retardant_obs_ref.py), from the dousing bits and from the u8 layer;
gca_advanced_policy_act_retardant (observe and act in one launch) against the two launches it is defined by, bit for bit;
then the env's observe / policy_act / rollout_policy with a BulldozerPolicy(retardant=True) against the hand-written loop
of public calls, as a graph, through the learner, and the step-by-step proof that the agent sees where it has doused."""
import numpy as np
import pytest

import _bulldozer_policy_ref as bref
import _retardant_obs_ref as rref

pytestmark = pytest.mark.gpu

# (E, H, W, block, radius, hidden), the grid plane's offset in bytes, the bit plane's offset in bytes
CASES = [((3, 32, 256, 8, 5, 64), 0, 0),      # rows form; a dword of bits holds four tile rows
         ((3, 32, 256, 16, 0, 32), 0, 0),     # two tile rows per dword; S = 1
         ((3, 32, 256, 32, 31, 256), 0, 0),   # one tile row per dword: the two words of a tile; the largest window
         ((2, 40, 512, 8, 5, 64), 0, 0),      # NW = 2: a strip cut short, one lane per tile
         ((2, 32, 512, 32, 2, 128), 0, 0),    # NW = 2, two words per tile row
         ((2, 24, 40, 4, 3, 32), 0, 0),       # generic form; W % 16 != 0: the u8 layer only; the pad word
         ((3, 32, 256, 8, 5, 64), 4, 0),      # a plane offset by 4 bytes: the grid's generic form, the bits by dwords
         ((2, 24, 48, 4, 3, 32), 0, 0),       # generic form with bits: four tiles share a word
         ((2, 40, 80, 64, 2, 32), 0, 0),      # a tile of four words and one of one; blocks stick out of the grid
         ((3, 32, 256, 8, 5, 64), 0, 2)]      # bits offset by 2 bytes: the masked words at a rows-form shape
IDS = [f"{s[1]}x{s[2]}b{s[3]}r{s[4]}+{o}+{bo}" for s, o, bo in CASES]
ROT = {(2, 24, 40, 4, 3, 32): 1, (2, 24, 48, 4, 3, 32): 1, (2, 40, 80, 64, 2, 32): 2}


def _offset_copy(device, host, offset):
    """`host` copied into a device allocation `offset` bytes after its 16-B aligned start."""
    import torch

    raw = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
    store = torch.zeros(raw.size + 16, dtype=torch.uint8, device=device)
    assert store.data_ptr() % 16 == 0
    view = store[offset:offset + raw.size]
    view.copy_(torch.from_numpy(raw))
    return view


def _device_case(device, shape, offset, bits_offset):
    """The shared case on the device: the policy, the device tensors (bits None where W % 16 != 0) and the host
    arrays."""
    import torch

    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    d, w, planes, dousing, pos, ts = rref.make_case(shape, ROT.get(shape, 0), above_one=False)
    E, H, W = planes.shape
    pol = BulldozerPolicy((H, W), d["radius"], d["block"], d["hidden"], device=device, retardant=True).load(w)
    assert pol.C == d["C"]
    t = dict(planes=_offset_copy(device, planes, offset), dousing=torch.from_numpy(dousing).to(device),
             pos=torch.from_numpy(pos).to(device), ts=torch.from_numpy(ts).to(device), bits=None)
    assert t["planes"].data_ptr() % 8 == offset % 8
    if W % 16 == 0:
        t["bits"] = _offset_copy(device, rref.pack_bits(dousing), bits_offset)
        assert t["bits"].data_ptr() % 4 == bits_offset % 4
    return d, w, pol, t, (planes, dousing, pos, ts)


def _outputs(device, d, E, stride=2):
    import torch

    kw = dict(device=device)
    return dict(action=torch.full((E, stride), rref.SENTINEL, dtype=torch.int32, **kw),
                logits=torch.full((E, 11), float("nan"), **kw), value=torch.full((E,), float("nan"), **kw),
                local=torch.full((E, d["S"], d["S"]), 0xAA, dtype=torch.uint8, **kw),
                feat=torch.full((E, d["C"]), -1.0, **kw))


def _observe(device, d, t, o, shape, bits, null=()):
    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    E, H, W = shape[:3]
    p = lambda n: None if n in null else o[n].data_ptr()
    # without bits the u8 layer is read; with them it must not be: the launch then gets a layer of the wrong content
    layer = t["dousing"] if not bits else 1 - t["dousing"]
    call("gca_advanced_policy_observation", t["planes"].data_ptr(), layer.data_ptr(),
         t["bits"].data_ptr() if bits else None, t["pos"].data_ptr(), E, H, W, *rref.CODES, d["radius"], d["block"],
         p("local"), p("feat"), dev.stream_ptr(device))
    return layer


def _fused(device, pol, t, o, shape, bits, greedy, env_offset, null=()):
    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    E, H, W = shape[:3]
    p = lambda n: None if n in null else o[n].data_ptr()
    layer = t["dousing"] if not bits else 1 - t["dousing"]
    call("gca_advanced_policy_act_retardant", pol.struct, t["planes"].data_ptr(), layer.data_ptr(),
         t["bits"].data_ptr() if bits else None, t["pos"].data_ptr(), t["ts"].data_ptr(), E, H, W, *rref.CODES,
         env_offset, rref.SEED, 1 if greedy else 0, o["action"].data_ptr(), int(o["action"].shape[1]), p("logits"),
         p("value"), p("local"), p("feat"), dev.stream_ptr(device))
    return layer


def _pair(device, pol, d, t, o, shape, bits, greedy, env_offset):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    layer = _observe(device, d, t, o, shape, bits)
    se = t["ts"].to(torch.int64)
    call("gca_bulldozer_policy_act", pol.struct, pol.C, o["local"].data_ptr(), o["feat"].data_ptr(), se.data_ptr(), None,
         env_offset, rref.SEED, 1 if greedy else 0, o["action"].data_ptr(), o["logits"].data_ptr(),
         o["value"].data_ptr(), shape[0], dev.stream_ptr(device))
    return layer


@pytest.mark.parametrize("shape, offset, bits_offset", CASES, ids=IDS)
def test_observation_kernel_equals_the_host_build(device, shape, offset, bits_offset):
    import torch

    d, w, pol, t, (planes, dousing, pos, ts) = _device_case(device, shape, offset, bits_offset)
    E = shape[0]
    want_lo, want_fe = rref.host_observe(planes, dousing, pos, d["radius"], d["block"])
    ref_lo, ref_fe = rref.ref(planes, dousing, pos, d["radius"], d["block"])
    assert np.array_equal(want_lo, ref_lo) and np.array_equal(rref.bits(want_fe), rref.bits(ref_fe))
    assert (want_fe[:, d["Cg"]:] > 0).any()
    for bits in ([False, True] if t["bits"] is not None else [False]):
        o = _outputs(device, d, E)
        keep = _observe(device, d, t, o, shape, bits)
        torch.cuda.synchronize(device)
        assert np.array_equal(o["local"].cpu().numpy(), want_lo), bits
        assert np.array_equal(rref.bits(o["feat"].cpu().numpy()), rref.bits(want_fe)), bits
        # either output may be NULL and leaves the other as it is
        a, b = _outputs(device, d, E), _outputs(device, d, E)
        _observe(device, d, t, a, shape, bits, null=("feat",))
        _observe(device, d, t, b, shape, bits, null=("local",))
        assert torch.equal(a["local"], o["local"]) and bool((a["feat"] == -1).all())
        assert torch.equal(b["feat"].view(torch.int32), o["feat"].view(torch.int32)) and bool((b["local"] == 0xAA).all())
        del keep


@pytest.mark.parametrize("env_offset", [0, 5])
@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("shape, offset, bits_offset", CASES, ids=IDS)
def test_fused_launch_equals_the_pair(device, shape, offset, bits_offset, greedy, env_offset):
    import torch

    d, w, pol, t, host = _device_case(device, shape, offset, bits_offset)
    E = shape[0]
    first = None
    for bits in ([False, True] if t["bits"] is not None else [False]):
        a, b = _outputs(device, d, E), _outputs(device, d, E)
        k1 = _fused(device, pol, t, a, shape, bits, greedy, env_offset)
        k2 = _pair(device, pol, d, t, b, shape, bits, greedy, env_offset)
        torch.cuda.synchronize(device)
        for name in ("local", "feat", "logits", "value", "action"):
            assert torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)), (name, bits)
        assert bool(torch.isfinite(a["logits"]).all()) and bool((a["feat"][:, d["Cg"]:] > 0).any())
        # the nullable outputs change nothing else; a third action column stays the caller's
        c = _outputs(device, d, E, stride=3)
        k3 = _fused(device, pol, t, c, shape, bits, greedy, env_offset, null=("logits", "value", "local", "feat"))
        assert torch.equal(c["action"][:, :2], a["action"]) and bool((c["action"][:, 2] == rref.SENTINEL).all())
        assert bool(torch.isnan(c["logits"]).all()) and bool((c["local"] == 0xAA).all()) and bool((c["feat"] == -1).all())
        # the bits and the u8 layer say the same: both launches give the same bits
        if first is None:
            first = a
        else:
            assert all(torch.equal(a[n].view(torch.uint8), first[n].view(torch.uint8)) for n in a)
        del k1, k2, k3
    if env_offset == 5:  # the host build and the composition of the restatements, once per case
        planes, dousing, pos, ts = host
        want = dict(zip(("action", "logits", "value", "local", "feat"),
                        rref.host_act(d, w, planes, dousing, pos, ts, env_offset=5, greedy=greedy)))
        for name, x in want.items():
            assert np.array_equal(first[name].cpu().numpy().view(np.uint8), x.view(np.uint8)), name
        assert np.array_equal(want["action"], rref.composed(d, w, planes, dousing, pos, ts, env_offset=5,
                                                            greedy=greedy)[0])


# ------------------------------------------------------------------ the env
STATE = ("pos", "accu", "wind_index", "time_step", "is_night", "rng_step", "counts", "dousing", "dous_bits",
         "steps_elapsed", "reward_accumulated", "reward", "done")


def _env(device, E=3, key=7):
    from gymca_amd.forest_fire.bulldozer import AdvancedForestFireBulldozerEnv

    env = AdvancedForestFireBulldozerEnv(32, 256, key=key, num_envs=E, device=device, observation="grid",
                                         hidden_rng="philox")
    env.reset()
    # env 1 has no fire left: its first step ends the episode, so a reset falls inside the K steps
    g = env.grid[env.cur].clone()
    g[1][g[1] == env._fire] = env._tree
    age = env.age[env.cur].clone()
    age[1] = 0
    env.set_state(grid=g, fire_age=age)
    assert env.dous_bits is not None  # the packed layout: the launches read the bits
    return env


def _env_policy(env, seed=3):
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    d = rref.dims(5, 8, 64, env.nrows, env.ncols)
    return BulldozerPolicy(env, 5, 8, 64, retardant=True).load(bref.make_weights(d, seed=seed, head=2.0)), d


def _assert_same_state(a, b):
    import torch

    assert a.cur == b.cur
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.grid[a.cur], b.grid[b.cur]) and torch.equal(a.age[a.cur], b.age[b.cur])


def _hand_loop(env, pol, K, seed):
    """K x (policy_act(fused=False) -> step -> record -> conditional_reset) in public calls; the records as rollout_policy
    lays them out."""
    import torch

    rows = {k: [] for k in env._POLICY_RECORDS}
    E = env.num_envs
    spec = env.policy_record_shapes(pol, 1)
    for _ in range(K):
        action = torch.zeros((E, 2), dtype=torch.int32, device=env.device)
        lo = torch.empty(spec["local"][1][1:], dtype=torch.uint8, device=env.device)
        co = torch.empty(spec["coarse"][1][1:], dtype=torch.float32, device=env.device)
        _, logits, value = env.policy_act(pol, seed=seed, action_out=action, local_out=lo, coarse_out=co, fused=False)
        env.step(action)
        rows["action"].append(action.clone())
        rows["logits"].append(logits)
        rows["value"].append(value)
        rows["local"].append(lo)
        rows["coarse"].append(co)
        rows["reward"].append(env.reward.to(torch.float64))
        rows["terminated"].append(env.done.clone())
        rows["truncated"].append(torch.zeros(E, dtype=torch.uint8, device=env.device))
        env.conditional_reset()
    return {k: torch.stack(v) for k, v in rows.items()}


def test_rollout_policy_equals_the_hand_written_loop(device):
    import torch

    K = 6
    env, twin = _env(device), _env(device)
    pol, d = _env_policy(env)
    E = env.num_envs
    # observe(retardant=True) is the restatement of the env's own state
    lo, fe = env.observe(5, 8, retardant=True)
    want_lo, want_fe = rref.ref(env.grid[env.cur].cpu().numpy(), env.dousing.cpu().numpy(), env.pos.cpu().numpy(), 5, 8)
    assert tuple(fe.shape) == (E, d["C"]) and np.array_equal(lo.cpu().numpy(), want_lo)
    assert np.array_equal(rref.bits(fe.cpu().numpy()), rref.bits(want_fe))
    # policy_act() touches no state: twice without a step, the same action; fused and the pair agree
    a1, l1, v1 = env.policy_act(pol, seed=11)
    a2, l2, v2 = env.policy_act(pol, seed=11)
    a3, l3, v3 = env.policy_act(pol, seed=11, fused=False)
    assert torch.equal(a1, a2) and torch.equal(l1, l2) and torch.equal(v1, v2)
    assert torch.equal(a1, a3) and torch.equal(l1, l3) and torch.equal(v1, v3)
    _assert_same_state(env, twin)
    rec = env.rollout_policy(pol, K, seed=11)
    want = _hand_loop(twin, pol, K, 11)
    spec = env.policy_record_shapes(pol, K)
    assert set(rec) == set(want) == set(spec) and spec["coarse"][1] == (K, E, d["C"])
    for name, (dtype, shape) in spec.items():
        assert rec[name].dtype is dtype and tuple(rec[name].shape) == shape, name
        assert torch.equal(rec[name].view(torch.uint8), want[name].contiguous().view(torch.uint8)), name
    _assert_same_state(env, twin)
    term = rec["terminated"].cpu().numpy()
    assert term[0, 1] == 1 and term.sum() < term.size  # the reset fell inside the K steps
    # the agent shot, and later rows saw the retardant; the first row saw none
    assert bool(rec["action"][..., 1].any()) and bool(env.dousing.any())
    tail = rec["coarse"][:, :, d["Cg"]:]
    assert float(tail[0].abs().sum()) == 0.0 and float(tail[1:].abs().sum()) > 0.0


def test_records_feed_the_learner(device):
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    E, K = 3, 8
    env = _env(device, E=E)
    pol, d = _env_policy(env)
    rec = env.rollout_policy(pol, K, seed=11)
    _, _, next_value = env.policy_act(pol, seed=11)
    adv, ret = ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95, terminal=rec["terminated"])
    grads, stats = pol.ppo_grad(rec, adv, ret)
    assert tuple(grads["w_coarse"].shape) == (d["C"], 64) and bool(torch.isfinite(stats).all())
    assert float(grads["w_coarse"][d["Cg"]:].abs().sum()) > 0.0  # the retardant's weights learn
    opt = ppo.Adam({n: getattr(pol, n) for n in WEIGHTS}, lr=1e-3)
    before = {n: t.clone() for n, t in pol.state_dict().items()}
    st, info = pol.ppo_update(opt, rec, adv, ret, epochs=2, minibatches=2, seed=7)
    assert tuple(st.shape) == (4, 8) and bool(torch.isfinite(st).all()) and bool(torch.isfinite(info).all())
    for n, t in pol.state_dict().items():
        assert bool(torch.isfinite(t).all()) and not torch.equal(t, before[n]), n


def test_rollout_policy_as_a_graph(device):
    import torch

    K = 4
    env, twin = _env(device), _env(device)
    pol, _ = _env_policy(env)
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


def test_the_agent_sees_where_it_has_doused(device):
    """A policy that reads one input only, the retardant flag of the window's centre: hidden unit 0 is 1 on an undoused
    cell and 0 on a doused one, the shoot logits are (0, h_0 - 0.5), the move is `stay`. Greedy, it shoots exactly where
    it has not doused yet."""
    import torch

    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    env = _env(device)
    E = env.num_envs
    r, B, Hd = 5, 8, 64
    d = rref.dims(r, B, Hd, env.nrows, env.ncols)
    w = {k: np.zeros_like(v) for k, v in bref.make_weights(d).items()}
    centre = 3 * d["Hc"] * d["Wc"] + r * d["S"] + r
    w["w_coarse"][centre, 0] = -1.0
    w["b1"][0] = 1.0
    w["w_out"][0, 10] = 1.0
    w["b2"][10] = -0.5
    w["b2"][4] = 1.0  # move 4: not_move
    pol = BulldozerPolicy(env, r, B, Hd, retardant=True).load(w)
    for fused in (True, False):
        a0, _, _ = env.policy_act(pol, greedy=True, fused=fused)
        assert a0.tolist() == [[4, 1]] * E, fused  # nothing doused yet: shoot
    pos0 = env.pos.clone()
    env.step(a0)
    assert torch.equal(env.pos, pos0) and int(env.dousing.sum()) == E and bool(env.done[1]) and not bool(env.done[0])
    for fused in (True, False):
        a1, _, _ = env.policy_act(pol, greedy=True, fused=fused)
        assert a1.tolist() == [[4, 0]] * E, fused  # its own retardant lies under it: the shoot column flipped
    env.conditional_reset()  # env 1 was finished: its dousing layer is empty again
    assert int(env.dousing[1].sum()) == 0 and int(env.dousing.sum()) == E - 1
    for fused in (True, False):
        a2, _, _ = env.policy_act(pol, greedy=True, fused=fused)
        assert a2.tolist() == [[4, 0], [4, 1], [4, 0]], fused


def test_training_script_takes_the_retardant_flag():
    import os
    import subprocess
    import sys

    from conftest import ROOT

    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_advanced_ppo.py"), "--envs", "4", "--rows", "32",
           "--cols", "256", "--steps", "8", "--iterations", "2", "--retardant"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    assert out.stdout.count("iteration ") == 2


def test_the_windy_env_refuses_a_retardant_policy(device):
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv, BulldozerPolicy

    env = BatchedForestFireBulldozerEnv(2, 32, 256, device=device, seed=17, materialize_obs=False, t_move=0.3,
                                        t_shoot=0.25)
    env.reset(seed=5)
    pol = BulldozerPolicy(env, 2, 8, 32, retardant=True)
    with pytest.raises(ValueError, match="no retardant layer"):
        env.act(pol)
    with pytest.raises(ValueError, match="no retardant layer"):
        env.rollout_policy(pol, 2)
    env.act(BulldozerPolicy(env, 2, 8, 32))  # the same policy without the keyword is taken
