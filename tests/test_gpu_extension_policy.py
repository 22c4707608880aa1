"""GPU: the extension agent (include/gca.h "extension policy"). The displayed plane against the restated reference and
against the frame kernel's own channel stack; the observe-and-act launch against the three launches it is defined by, bit
for bit; the env's policy_act / rollout_policy against the hand-written loop of public calls and as a graph; the
three-head learner against the float64 yardsticks, and the loop end to end."""
import numpy as np
import pytest

import _adam_ref as A
import _extension_policy_ref as X
import _ppo_ref as R
import _ppo_vclip_ref as V

pytestmark = pytest.mark.gpu

EXT = X.AGENT
SEED = 0x1234ABCD5678


def _t(x, dtype, device):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x), device=device).to(dtype).contiguous()


def _display(device, params, grid, night, time_step=None, choice=None, stride=1):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    E, H, W = grid.shape
    g, n = _t(grid, torch.uint8, device), _t(night, torch.int32, device)
    ts = None if time_step is None else _t(time_step, torch.int32, device)
    ch = None if choice is None else _t(choice, torch.int32, device)
    out = torch.full((E, H, W), 0xEE, dtype=torch.uint8, device=device)
    call("gca_advanced_display", params, E, H, W, dev.ptr(g), dev.ptr(n), dev.ptr(ts), dev.ptr(ch), stride, dev.ptr(out),
         dev.stream_ptr(device))
    return out.cpu().numpy()


# ------------------------------------------------------------------ the displayed plane
@pytest.mark.parametrize("should_transform", [True, False], ids=["transform", "plain"])
@pytest.mark.parametrize("name", X.DISPLAY_CASES)
def test_display_equals_the_restated_reference_and_the_frame_kernels_channels(device, name, should_transform):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    grid, choice, night = X.display_case(name)
    E, H, W = grid.shape
    params = X.obs_params(True, should_transform)
    want = X.want_display(grid, choice, night, True, should_transform)
    got = _display(device, params, grid, night, None, choice)
    assert np.array_equal(got, want)
    act = np.zeros((E, 3), np.int32)
    act[:, 2] = choice
    assert np.array_equal(_display(device, params, grid, night, None, act.reshape(-1)[2:], 3), want)
    assert np.array_equal(X.host_display(params, grid, night, None, choice), want)
    # gca_adv_observation's `channels` output on the same inputs selects to the same plane
    g, n, a = _t(grid, torch.uint8, device), _t(night, torch.int32, device), _t(act, torch.int32, device)
    pos = torch.zeros((E, 2), dtype=torch.int32, device=device)
    rgb = torch.empty((E, H, W, 3), dtype=torch.float32, device=device)
    ch = torch.full((E, H, W, 5), 255, dtype=torch.uint8, device=device)
    call("gca_adv_observation", params, 0, E, H, W, dev.ptr(g), None, dev.ptr(pos), dev.ptr(n), None, dev.ptr(a), 3,
         dev.ptr(rgb), dev.ptr(ch), None, dev.stream_ptr(device))
    ch = ch.cpu().numpy()
    for e in range(E):
        exts = ch[e][..., 3:]
        has = np.array([np.any(x > 0) for x in exts])
        sel = exts[..., min(int(np.argmax(has)), exts.shape[-1] - 1)] if has.any() else ch[e][..., 0]
        assert np.array_equal(sel, got[e]), e


def test_display_visibility_branch_through_the_c_abi(device):
    g = X.code3_case()
    grid = np.stack([g, g, g, g])
    p = X.obs_params(True, True, tree=1, fire=3)
    night = np.array([0, 1, 0, 1], np.int32)
    ts, pre = np.array([400, 800, 399, 401], np.int32), np.array([1, 0, 0, 1], np.int32)
    for choice in (0, 1, 2):
        ch = np.full(4, choice, np.int32)
        want = X.want_display(grid, ch, night, True, True)
        assert np.array_equal(_display(device, p, grid, night, None, ch), want)
        if choice == 1:  # unblur shows the raw plane: its 3s are 0 by day and 3 by night (a blurred 3 is rare)
            assert (want[0] != 3).all() and (want[1] == 3).any()
        assert np.array_equal(_display(device, p, grid, night, ts, ch), X.want_display(grid, ch, pre, True, True))


# ------------------------------------------------------------------ observe the display and act: one launch == the triple
def _outputs(device, d, E, stride=3):
    import torch

    kw = dict(device=device)
    return dict(action=torch.full((E, stride), -7, dtype=torch.int32, **kw),
                logits=torch.full((E, 14), float("nan"), **kw), value=torch.full((E,), float("nan"), **kw),
                local=torch.full((E, d["S"], d["S"]), 0xAA, dtype=torch.uint8, **kw),
                coarse=torch.full((E, 2, d["Hc"], d["Wc"]), -1.0, **kw))


def _policy(device, d, w):
    from gymca_amd.forest_fire.bulldozer import ExtensionBulldozerPolicy

    return ExtensionBulldozerPolicy((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device=device).load(w)


# (radius, block, hidden, H, W): the generic form; the rows form at both widths with a strip cut short and more strips
# than waves; hidden 32 and 256; W = 512 with block 8 (one lane per tile: no lane sum, every lane stores) and block 32
ACT_SHAPES = [(2, 4, 64, 13, 11), (5, 8, 32, 32, 256), (5, 16, 256, 64, 512), (3, 8, 64, 40, 256), (2, 32, 32, 160, 256),
              (5, 8, 64, 32, 512), (2, 32, 32, 64, 512)]


@pytest.mark.parametrize("should_transform", [True, False], ids=["transform", "plain"])
@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("shape", ACT_SHAPES)
def test_fused_launch_equals_the_triple(device, shape, greedy, should_transform):
    d, w, _, grid, pos, night, ts, choice = X.act_case(shape)
    _fused_against_the_triple(device, d, w, X.obs_params(True, should_transform), grid, pos, night, ts, choice, greedy)


@pytest.mark.parametrize("greedy", [False, True], ids=["sampled", "greedy"])
@pytest.mark.parametrize("shape", [ACT_SHAPES[0], ACT_SHAPES[1], ACT_SHAPES[5]])
def test_fused_launch_equals_the_triple_on_planes_that_hold_the_value_3(device, shape, greedy):
    """Codes {0, 1, 3}, tree = 1, fire = 3, by day and by night: visibility's 3 -> 0 in the window's classes and in the
    blurred strip, and the raw display's fallback to the generic loops where the FIRE code is the literal 3."""
    d, w, params, grid, pos, night, ts, choice = X.act_case(shape, code3=True)
    pre = np.where(ts % 400 == 0, 1 - night, night)
    raw = choice == 1
    assert (raw & (pre == 0)).any() and (raw & (pre == 1)).any() and (grid == 3).any()
    coarse = _fused_against_the_triple(device, d, w, params, grid, pos, night, ts, choice, greedy)
    fire = coarse.reshape(len(grid), 2, -1)[:, 1].sum(1)
    # the raw display by day shows no fire at all; by night the plane's 3s are there
    assert (fire[raw & (pre == 0)] == 0).all() and (fire[raw & (pre == 1) & (grid == 3).any((1, 2))] > 0).all()


def _fused_against_the_triple(device, d, w, params, grid, pos, night, ts, choice, greedy):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call

    pol = _policy(device, d, w)
    E, H, W = grid.shape
    g, po = _t(grid, torch.uint8, device), _t(pos, torch.int32, device)
    n, t, c = _t(night, torch.int32, device), _t(ts, torch.int32, device), _t(choice, torch.int32, device)
    st = dev.stream_ptr(device)

    def fused(o, cp, cstride):
        call("gca_advanced_policy_act_display", pol.struct, params, dev.ptr(g), dev.ptr(po), dev.ptr(n), dev.ptr(t), cp,
             cstride, E, H, W, 3, SEED, 1 if greedy else 0, dev.ptr(o["action"]), int(o["action"].shape[1]),
             dev.ptr(o["logits"]), dev.ptr(o["value"]), dev.ptr(o["local"]), dev.ptr(o["coarse"]), st)

    a, b = _outputs(device, d, E), _outputs(device, d, E)
    fused(a, dev.ptr(c), 1)
    plane = torch.empty((E, H, W), dtype=torch.uint8, device=device)
    call("gca_advanced_display", params, E, H, W, dev.ptr(g), dev.ptr(n), dev.ptr(t), dev.ptr(c), 1, dev.ptr(plane), st)
    call("gca_policy_observation", dev.ptr(plane), None, None, dev.ptr(po), E, H, W, params.empty, params.tree,
         params.fire, pol.radius, pol.block, 0, dev.ptr(b["local"]), dev.ptr(b["coarse"]), st)
    se = t.to(torch.int64)
    call("gca_extension_policy_act", pol.struct, pol.C, dev.ptr(b["local"]), dev.ptr(b["coarse"]), dev.ptr(se), None, 3,
         SEED, 1 if greedy else 0, dev.ptr(b["action"]), dev.ptr(b["logits"]), dev.ptr(b["value"]), E, st)
    torch.cuda.synchronize(device)
    for name in ("local", "coarse", "logits", "value", "action"):
        assert torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)), name
    assert bool(torch.isfinite(a["logits"]).all()) and bool(((a["action"] >= 0) & (a["action"] <= 8)).all())
    if d["radius"] > 0:
        assert (a["local"] == 3).any() and (a["local"] != 3).any()
    # the host build agrees, and so the device equals the restated display, observation and network
    host = X.host_act_display(w, d, params, grid, pos, night, ts, choice, env_offset=3, seed=SEED, greedy=greedy)
    for name, h in zip(("action", "logits", "value", "local", "coarse"), host):
        assert np.array_equal(a[name].cpu().numpy().reshape(h.shape).view(np.uint8), h.view(np.uint8)), name
    # `choice` aliasing column 2 of the action rows (a wider stride; the fourth column stays the caller's)
    o = _outputs(device, d, E, stride=4)
    o["action"][:, 2] = c
    fused(o, o["action"].data_ptr() + 8, 4)
    assert torch.equal(o["action"][:, :3], a["action"]) and bool((o["action"][:, 3] == -7).all())
    assert torch.equal(o["logits"].view(torch.uint8), a["logits"].view(torch.uint8))
    assert torch.equal(o["coarse"].view(torch.uint8), a["coarse"].view(torch.uint8))
    return a["coarse"].cpu().numpy()


# ------------------------------------------------------------------ the env
STATE = ("pos", "accu", "wind_index", "time_step", "is_night", "rng_step", "counts", "dousing", "steps_elapsed",
         "reward_accumulated", "reward", "done")


def _env(device, E=4, key=7):
    from gymca_amd.forest_fire.bulldozer import AdvancedForestFireBulldozerEnv

    env = AdvancedForestFireBulldozerEnv(32, 256, key=key, num_envs=E, device=device, observation="grid",
                                         hidden_rng="philox", enable_extensions=True)
    env.reset()
    # env 1 has no fire left: its first step ends the episode, so a reset falls inside the K steps
    g = env.grid[env.cur].clone()
    g[1][g[1] == env._fire] = env._tree
    age = env.age[env.cur].clone()
    age[1] = 0
    env.set_state(grid=g, fire_age=age)
    return env


def _env_policy(env, seed=3, hidden=64):
    from gymca_amd.forest_fire.bulldozer import ExtensionBulldozerPolicy

    d = X.dims(5, 8, hidden, env.nrows, env.ncols)
    return ExtensionBulldozerPolicy(env, 5, 8, hidden).load(X.make_weights(d, seed=seed, head=2.0))


def _assert_same_state(a, b):
    import torch

    assert a.cur == b.cur
    for name in STATE:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.grid[a.cur], b.grid[b.cur]) and torch.equal(a.age[a.cur], b.age[b.cur])


def _hand_loop(env, pol, K, seed):
    """K x (policy_act(choice = the previous action's third column, fused=False) -> step -> record ->
    conditional_reset) in public calls; the records as rollout_policy lays them out."""
    import torch

    names = env._POLICY_RECORDS + ("is_night",)
    rows = {k: [] for k in names}
    E = env.num_envs
    prev = torch.zeros(E, dtype=torch.int32, device=env.device)
    for _ in range(K):
        spec = env.policy_record_shapes(pol, 1)
        lo = torch.empty(spec["local"][1][1:], dtype=torch.uint8, device=env.device)
        co = torch.empty(spec["coarse"][1][1:], dtype=torch.float32, device=env.device)
        rows["is_night"].append(env.is_night.to(torch.uint8))
        action, logits, value = env.policy_act(pol, seed=seed, local_out=lo, coarse_out=co, fused=False, choice=prev)
        assert tuple(action.shape) == (E, 3) and tuple(logits.shape) == (E, 14)
        env.step(action)
        prev = action[:, 2].clone()
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


def test_env_policy_act_fused_equals_the_triple_and_follows_the_previous_choice(device):
    import torch

    env = _env(device)
    E = env.num_envs
    for hidden in (32, 256):
        pol = _env_policy(env, hidden=hidden)
        for greedy in (False, True):
            for choice in (None, torch.tensor([0, 1, 2, 1], dtype=torch.int32, device=device)):
                lo = [torch.empty((E, 11, 11), dtype=torch.uint8, device=device) for _ in range(2)]
                co = [torch.empty((E, 2, 4, 32), dtype=torch.float32, device=device) for _ in range(2)]
                a = env.policy_act(pol, seed=11, greedy=greedy, local_out=lo[0], coarse_out=co[0], fused=True,
                                   choice=choice)
                b = env.policy_act(pol, seed=11, greedy=greedy, local_out=lo[1], coarse_out=co[1], fused=False,
                                   choice=choice)
                for x, y in zip(a + (lo[0], co[0]), b + (lo[1], co[1])):
                    assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    # display() / observe(display=True): the plane of the restated reference, and the choice of the previous step
    pol = _env_policy(env)
    grid = env.grid[env.cur].cpu().numpy()
    night = env.is_night.cpu().numpy()
    zero = np.zeros(E, np.int32)
    assert np.array_equal(env.display().cpu().numpy(), X.want_display(grid, zero, night, True, True))  # after reset(): 0
    ch = torch.tensor([2, 1, 0, 1], dtype=torch.int32, device=device)
    assert np.array_equal(env.display(choice=ch).cpu().numpy(), X.want_display(grid, ch.cpu().numpy(), night, True, True))
    local, coarse = env.observe(5, 8, display=True, choice=ch)
    act = torch.zeros((E, 3), dtype=torch.int32, device=device)
    _, _, _ = env.policy_act(pol, seed=11, action_out=act, local_out=local.clone(), coarse_out=coarse.clone(), choice=ch)
    lo2 = torch.empty_like(local)
    co2 = torch.empty_like(coarse)
    env.policy_act(pol, seed=11, local_out=lo2, coarse_out=co2, choice=ch)
    assert torch.equal(lo2, local) and torch.equal(co2.view(torch.uint8), coarse.view(torch.uint8))
    act[:, 2] = torch.tensor([1, 2, 1, 0], dtype=torch.int32, device=device)
    env.step(act)
    env.conditional_reset()  # keeps the choice
    grid = env.grid[env.cur].cpu().numpy()
    pre = np.where(env.time_step.cpu().numpy() % 400 == 0, 1 - env.is_night.cpu().numpy(), env.is_night.cpu().numpy())
    assert np.array_equal(env.display().cpu().numpy(), X.want_display(grid, np.array([1, 2, 1, 0]), pre, True, True))
    env.reset()  # forgets it
    grid = env.grid[env.cur].cpu().numpy()
    assert np.array_equal(env.display().cpu().numpy(), X.want_display(grid, zero, zero, True, True))
    with pytest.raises(ValueError, match="action_out"):
        env.policy_act(pol, action_out=torch.zeros((E, 2), dtype=torch.int32, device=device))


# (H, W, radius, block, hidden): the rows form at both widths (block 8 at W = 512: a lane per tile), the generic form
ENV_SHAPES = [(32, 256, 5, 8, 32), (64, 512, 5, 16, 256), (32, 512, 5, 8, 64), (32, 32, 2, 4, 64)]


@pytest.mark.parametrize("H, W, radius, block, hidden", ENV_SHAPES)
def test_env_policy_act_fused_equals_the_triple_at_every_shape(device, H, W, radius, block, hidden):
    """env.policy_act(fused=True) == env.policy_act(fused=False), bit for bit, through the Python wrapper (the bound
    call's slots, the choice taken from the previous step's action tensor): every shape, the bulldozer in a corner, on
    an edge and in the middle, sampled and greedy, mixed choices across the envs."""
    import torch

    from gymca_amd.forest_fire.bulldozer import AdvancedForestFireBulldozerEnv, ExtensionBulldozerPolicy

    E = 4
    env = AdvancedForestFireBulldozerEnv(H, W, key=5, num_envs=E, device=device, observation="grid", use_hidden=False,
                                         enable_extensions=True)
    env.reset()
    d = X.dims(radius, block, hidden, H, W)
    pol = ExtensionBulldozerPolicy(env, radius, block, hidden).load(X.make_weights(d, seed=hidden, head=2.0))
    ls, cs = (E, d["S"], d["S"]), (E, 2, d["Hc"], d["Wc"])

    def both(**kw):
        out = []
        for fused in (True, False):
            lo = torch.full(ls, 0xAA, dtype=torch.uint8, device=device)
            co = torch.full(cs, -1.0, device=device)
            out.append(env.policy_act(pol, seed=11, local_out=lo, coarse_out=co, fused=fused, **kw) + (lo, co))
        for x, y in zip(*out):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
        return out[0]

    act = torch.tensor([[4, 0, 1], [4, 1, 2], [4, 0, 0], [4, 1, 2]], dtype=torch.int32, device=device)
    env.step(act)  # the next display follows this action's third column
    env.set_state(position=np.array([(0, 0), (0, W // 2), (H // 2, W // 2), (H - 1, W - 1)], np.int32))
    grid, night = env.grid[env.cur].cpu().numpy(), env.is_night.cpu().numpy()
    seen = {}
    for greedy in (False, True):
        a, l, v, lo, co = both(greedy=greedy)  # choice=None: column 2 of the action tensor step() was given
        assert tuple(a.shape) == (E, 3) and tuple(l.shape) == (E, 14) and (lo == 3).any() and (lo != 3).any()
        b = both(greedy=greedy, choice=act[:, 2])
        assert torch.equal(co, b[4]) and torch.equal(a, b[0])
        seen[greedy] = co
        c = both(greedy=greedy, choice=torch.tensor([2, 0, 1, 1], dtype=torch.int32, device=device))
        assert not torch.equal(c[4], co)  # other choices, another observation
    # what the wrapper showed the network is the restated display's observation
    plane = torch.from_numpy(X.want_display(grid, act[:, 2].cpu().numpy(), night, True, True)).to(device)
    keep = env.grid[env.cur].clone()
    env.grid[env.cur].copy_(plane)
    _, want_co = env.observe(radius, block)
    env.grid[env.cur].copy_(keep)
    assert torch.equal(seen[False], want_co) and torch.equal(seen[True], want_co)


def test_rollout_policy_equals_the_hand_written_loop(device):
    import torch

    K = 4
    env, twin = _env(device), _env(device)
    pol = _env_policy(env)
    rec = env.rollout_policy(pol, K, seed=11, record=env._POLICY_RECORDS + ("is_night",))
    want = _hand_loop(twin, pol, K, 11)
    spec = env.policy_record_shapes(pol, K)
    assert set(rec) == set(want) == set(spec)
    assert spec["action"][1] == (K, 4, 3) and spec["logits"][1] == (K, 4, 14) and spec["is_night"][1] == (K, 4)
    for name, (dtype, shape) in spec.items():
        assert rec[name].dtype is dtype and tuple(rec[name].shape) == shape, name
        assert torch.equal(rec[name].view(torch.uint8), want[name].contiguous().view(torch.uint8)), name
    _assert_same_state(env, twin)
    term = rec["terminated"].cpu().numpy()
    assert term[0, 1] == 1 and term.sum() < term.size  # an env terminated inside the window
    assert len(torch.unique(rec["action"][..., 2])) > 1 and int(rec["action"][..., 2].max()) <= 2
    # nobody's default changes: no is_night record unless it is asked for
    assert "is_night" not in twin.rollout_policy(pol, 2, seed=11)
    out = torch.full((2, 4), 9, dtype=torch.uint8, device=device)
    assert twin.rollout_policy(pol, 2, seed=11, record=(), is_night_out=out)["is_night"] is out and int(out.max()) <= 1


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
        want = twin.rollout_policy(pol, K, seed=11, record=tuple(env.policy_record_shapes(pol, K)))
    torch.cuda.synchronize(device)
    for name, t in want.items():
        assert torch.equal(outs[f"{name}_out"].view(torch.uint8), t.view(torch.uint8)), name
    _assert_same_state(env, twin)
    # a capture with no eager rollout before it would replay the start-of-rollout zeroing of the choice: refused
    fresh = _env(device)
    scratch = torch.zeros(4, device=device)
    with pytest.raises(ValueError, match="needs a preceding eager rollout_policy"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            scratch.add_(1.0)
            fresh.rollout_policy(pol, 2, seed=11, record=())


# ------------------------------------------------------------------ the learner
def _dev(a, device):
    import torch

    return torch.from_numpy(np.array(a)).to(device)


def _learner(device, c):
    pol = _policy(device, c["d"], c["w"])
    rec = {k: _dev(v, device) for k, v in c["rec"].items()}
    return pol, rec, _dev(c["adv"], device), _dev(c["ret"], device)


@pytest.mark.parametrize("shape", X.SHAPES)
def test_ppo_grad_within_the_tolerance_and_reproducible(device, shape):
    import torch

    c = X.ppo_case(shape)
    R.check_case(c)
    idx = R.minibatch(c, 257)
    args = (c["w"], c["d"], c["rec"], c["adv"], c["ret"], idx, EXT.heads)
    g64, s64, _, _ = R.loss_and_grad(*args)
    g32, s32, _, _ = R.loss_and_grad(*args, dtype="float32")
    pol, rec, adv, ret = _learner(device, c)
    grads, stats = pol.ppo_grad(rec, adv, ret, _dev(idx, device))
    got = {k: v.cpu().numpy() for k, v in grads.items()}
    R.assert_within(R.errors(got, stats.cpu().numpy(), g64, s64), R.errors(g32, s32, g64, s64), f"device {shape}")
    g2, s2 = pol.ppo_grad(rec, adv, ret, _dev(idx, device))
    assert all(torch.equal(grads[k].view(torch.uint8), g2[k].view(torch.uint8)) for k in R.GRADS)
    assert torch.equal(stats.view(torch.uint8), s2.view(torch.uint8))
    assert np.abs(got["w_out"][:, 11:14]).max() > 0


@pytest.mark.parametrize("shape", X.SHAPES)
def test_ppo_grad_vclip_within_the_tolerance_and_reproducible(device, shape):
    import torch

    c = X.vclip_case(shape)
    idx, f64, f32 = V.minibatch(c, 300)
    pol, rec, adv, ret = _learner(device, c)
    rec["value"] = _dev(c["vo"], device)
    grads, stats, vs = pol.ppo_grad(rec, adv, ret, _dev(idx, device), clip_vloss=True)
    got = {k: v.cpu().numpy() for k, v in grads.items()}
    R.assert_within(V.errors(got, stats.cpu().numpy(), vs.cpu().numpy(), f64), V.yard_errors(f32, f64),
                    f"device vclip {shape}")
    V.assert_shares(vs.cpu().numpy(), f64, len(idx), f"device vclip {shape}")
    g2, s2, v2 = pol.ppo_grad(rec, adv, ret, _dev(idx, device), clip_vloss=True)
    assert all(torch.equal(grads[k].view(torch.uint8), g2[k].view(torch.uint8)) for k in R.GRADS)
    assert torch.equal(stats.view(torch.uint8), s2.view(torch.uint8)) and torch.equal(vs, v2)


@pytest.mark.parametrize("clip_vloss", [False, True], ids=["plain", "vclip"])
def test_ppo_update_equals_the_hand_written_loop(device, clip_vloss):
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    c = X.vclip_case(X.SHAPES[0])
    T, EPOCHS, MB = c["T"], 2, 2

    def setup():
        pol, rec, adv, ret = _learner(device, c)
        rec["value"] = _dev(c["vo"], device)
        return pol, ppo.Adam({n: getattr(pol, n) for n in WEIGHTS}, lr=2.5e-4), rec, adv, ret

    pol, opt, rec, adv, ret = setup()
    out = pol.ppo_update(opt, rec, adv, ret, epochs=EPOCHS, minibatches=MB, seed=5, clip_vloss=clip_vloss)
    stats, info = out[0], out[1]
    assert tuple(stats.shape) == (4, 8) and bool(torch.isfinite(stats).all()) and bool(torch.isfinite(info).all())
    pol2, opt2, _, _, _ = setup()
    perm = ppo.permutation(T, EPOCHS, seed=5, counter=opt2.count)
    N = T // MB
    want = []
    for e in range(EPOCHS):
        for mb in range(MB):
            r = pol2.ppo_grad(rec, adv, ret, perm[e, mb * N:(mb + 1) * N], clip_vloss=clip_vloss)
            want.append(r[1])
            opt2.step(r[0])
    assert np.array_equal(A.bits(stats), A.bits(torch.stack(want)))
    for n in WEIGHTS:
        assert np.array_equal(A.bits(getattr(pol, n)), A.bits(getattr(pol2, n))), n
        assert not np.array_equal(getattr(pol, n).cpu().numpy(), c["w"][n]), n  # the weights change


def test_rollout_gae_ppo_update_end_to_end(device):
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    E, K = 4, 8
    env = _env(device, E=E)
    pol = _env_policy(env)
    rec = env.rollout_policy(pol, K, seed=11, record=env._POLICY_RECORDS + ("is_night",))
    assert tuple(rec["action"].shape) == (K, E, 3) and tuple(rec["logits"].shape) == (K, E, 14)
    _, _, next_value = env.policy_act(pol, seed=11)
    adv, ret = ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95, terminal=rec["terminated"])
    opt = ppo.Adam({n: getattr(pol, n) for n in WEIGHTS}, lr=1e-3)
    before = {n: t.clone() for n, t in pol.state_dict().items()}
    st, info, vst = pol.ppo_update(opt, rec, adv, ret, epochs=2, minibatches=2, seed=7, clip_vloss=True)
    assert tuple(st.shape) == (4, 8) and bool(torch.isfinite(st).all()) and bool(torch.isfinite(info).all())
    assert bool(torch.isfinite(vst).all())
    for n, t in pol.state_dict().items():
        assert bool(torch.isfinite(t).all()) and not torch.equal(t, before[n]), n
    # the reference's two rates are defined on these records
    day = rec["is_night"] == 0
    assert int(day.sum()) + int((~day).sum()) == K * E
