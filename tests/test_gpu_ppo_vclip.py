"""GPU: the learner's clipped value loss on the device (<Agent>Policy.ppo_grad(clip_vloss=True),
gca_<agent>_policy_grad_vclip) for both agents: against the float64 autograd yardstick of tests/_ppo_vclip_ref.py within
4 x the error of torch's own float32 autograd and against the host build, the two shares exactly, at the minibatch
sizes around the kernels' sample tile; equal bits across calls; vf_coef = 0 against the plain entry; ppo_update eager
against one captured graph; the Advanced env's records end to end; and --clip-vloss of the three training scripts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import _policy_ref as P
import _ppo_ref as R
import _ppo_vclip_ref as V

pytestmark = pytest.mark.gpu


def _pick(agent):
    """Each agent's smallest shape (the fewest network inputs) and its 256-unit shape."""
    size = lambda s: P.dims(*s)["SS"] + P.dims(*s)["C"]
    shapes = R.SHAPES[agent]
    return {shapes.index(min(shapes, key=size))} | {i for i, s in enumerate(shapes) if s[2] == 256}


PICK = {a: _pick(a) for a in R.AGENTS}


def _dev(a, device):
    import torch

    return None if a is None else torch.from_numpy(np.array(a)).to(device)


def _policy(device, c):
    d = c["d"]
    return c["agent"].policy_class()((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device=device).load(c["w"])


def _records(device, c):
    rec = {k: _dev(v, device) for k, v in c["rec"].items()}
    rec["value"] = _dev(c["vo"], device)
    return rec, _dev(c["adv"], device), _dev(c["ret"], device)


def _nan_outputs(pol):
    import torch

    grads = {k: torch.full(s, float("nan"), device=pol.device) for k, s in pol.weight_shapes().items()}
    return grads, torch.full((8,), float("nan"), device=pol.device), torch.full((3,), float("nan"), device=pol.device)


def _same_bits(a, b):
    import torch

    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("agent, shape", R.params(pick=PICK))
def test_vclip_against_the_float64_yardstick_and_the_host(device, agent, shape):
    from gymca_amd import _lib

    c = V.case(agent, shape)
    R.check_case(c)
    assert len(PICK[agent]) == 2
    pol = _policy(device, c)
    rec, adv, ret = _records(device, c)
    ts = R.kernel_tile(_lib.load(), c)  # the kernels' own sample tile
    assert ts > 1
    for N in (1, ts - 1, ts, ts + 1, 2 * ts + 3, 1200):
        idx, f64, f32 = V.minibatch(c, N)
        gh, sh, vh = V.host_grad(agent, c["w"], c["d"], c["rec"], c["adv"], c["ret"], c["vo"], idx)
        grads, stats, vstats = _nan_outputs(pol)
        out = pol.ppo_grad(rec, adv, ret, _dev(idx, device), grads_out=grads, stats_out=stats, clip_vloss=True,
                           vstats_out=vstats)
        assert out[1] is stats and out[2] is vstats
        got = {k: v.cpu().numpy() for k, v in grads.items()}
        st, vs = stats.cpu().numpy(), vstats.cpu().numpy()
        assert all(np.isfinite(g).all() for g in got.values()) and np.isfinite(st).all() and np.isfinite(vs).all()
        where = f"{agent} {shape} N={N}"
        e32 = V.yard_errors(f32, f64)
        R.assert_within(V.errors(got, st, vs, f64), e32, where)
        V.assert_shares(vs, f64, N, where)
        host = ({k: gh[k].astype(np.float64) for k in gh}, sh.astype(np.float64), (float(vh[0]),))
        R.assert_within(V.errors(got, st, vs, host), e32, where + " vs host")
        assert vs[1] == vh[1] and vs[2] == vh[2]


@pytest.mark.parametrize("agent, shape", R.params(pick=PICK))
def test_vclip_is_reproducible(device, agent, shape):
    import torch

    c = V.case(agent, shape)
    pol = _policy(device, c)
    rec, adv, ret = _records(device, c)
    idx = _dev(V.draw(c, 333, 0)[0], device)
    for i in (idx, None):
        g1, s1, v1 = pol.ppo_grad(rec, adv, ret, i, clip_vloss=True)
        g2, s2, v2 = _nan_outputs(pol)
        pol.ppo_grad(rec, adv, ret, i, grads_out=g2, stats_out=s2, clip_vloss=True, vstats_out=v2)
        assert all(_same_bits(g1[k], g2[k]) for k in g1) and _same_bits(s1, s2) and _same_bits(v1, v2)
    # idx = None is rows 0 .. T - 1
    g3, s3, v3 = pol.ppo_grad(rec, adv, ret, torch.arange(c["T"], dtype=torch.int32, device=device), clip_vloss=True)
    assert all(_same_bits(g1[k], g3[k]) for k in g1) and _same_bits(s1, s3) and _same_bits(v1, v3)


@pytest.mark.parametrize("agent, shape", R.params(pick=PICK))
def test_vclip_with_vf_coef_zero_equals_the_plain_entry(device, agent, shape):
    import torch

    c = V.case(agent, shape)
    pol = _policy(device, c)
    rec, adv, ret = _records(device, c)
    for N in (1, 333, 1200):
        idx = _dev(V.draw(c, N, 0)[0], device)
        g, s, _ = pol.ppo_grad(rec, adv, ret, idx, vf_coef=0.0, clip_vloss=True)
        gp, sp = pol.ppo_grad(rec, adv, ret, idx, vf_coef=0.0)
        for k in g:
            assert torch.equal(g[k], gp[k]), (N, k)  # as numbers: -0.0 == 0.0
        for i in (1, 3, 4, 5, 6, 7):
            assert torch.equal(s[i], sp[i]), (N, R.STATS[i])


def test_ppo_update_clip_vloss_eager_and_as_one_graph(device):
    import torch

    from gymca_amd.forest_fire import ppo

    agent = R.HELI
    # the helicopter's smallest shape
    shape = next(R.SHAPES[agent][i] for i in sorted(PICK[agent]) if R.SHAPES[agent][i][2] != 256)
    c = V.case(agent, shape)
    K, E, EPOCHS, MB = 16, 8, 2, 2
    T, steps = K * E, EPOCHS * MB
    cut = lambda a: _dev(np.ascontiguousarray(a[:T]).reshape((K, E) + a.shape[1:]), device)
    rec = {k: cut(v) for k, v in c["rec"].items()}
    rec["value"] = cut(c["vo"])
    adv, ret = cut(c["adv"]), cut(c["ret"])

    def setup():
        pol = _policy(device, c)
        return pol, ppo.Adam(pol.state_dict(), lr=1e-3)

    pol2, opt2 = setup()
    eager = pol2.ppo_update(opt2, rec, adv, ret, epochs=EPOCHS, minibatches=MB, seed=5, clip_vloss=True)
    assert tuple(eager[2].shape) == (steps, 3) and bool(torch.isfinite(eager[2]).all())
    pol, opt = setup()
    stats = torch.full((steps, 8), float("nan"), device=device)
    info = torch.full((steps, 2), float("nan"), device=device)
    vstats = torch.full((steps, 3), float("nan"), device=device)
    perm = torch.full((EPOCHS, T), -1, dtype=torch.int32, device=device)
    grads = {n: torch.empty(s, device=device) for n, s in pol.weight_shapes().items()}
    ws = torch.empty(pol._ppo_workspace(T // MB, None).numel(), dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pol.ppo_update(opt, rec, adv, ret, epochs=EPOCHS, minibatches=MB, seed=5, stats_out=stats, info_out=info,
                             perm_out=perm, grads_out=grads, workspace=ws, clip_vloss=True, vstats_out=vstats)
    assert out[0] is stats and out[1] is info and out[2] is vstats
    graph.replay()
    torch.cuda.synchronize(device)
    assert _same_bits(stats, eager[0]) and _same_bits(info, eager[1]) and _same_bits(vstats, eager[2])
    for n in pol.state_dict():
        assert _same_bits(pol.state_dict()[n], pol2.state_dict()[n]), n
    assert bool(((vstats[:, 1:] >= 0) & (vstats[:, 1:] <= 1)).all())


def test_advanced_env_records_reach_the_clipped_value_loss(device):
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer import AdvancedForestFireBulldozerEnv, BulldozerPolicy

    E, K = 4, 4
    env = AdvancedForestFireBulldozerEnv(64, 64, key=7, num_envs=E, device=device, observation="grid",
                                         hidden_rng="philox")
    env.reset()
    pol = BulldozerPolicy(env, 5, 8, 64, seed=3)
    rec = env.rollout_policy(pol, K, seed=11)
    _, _, next_value = env.policy_act(pol, seed=11)
    adv, ret = ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95, terminal=rec["terminated"])
    opt = ppo.Adam(pol.state_dict(), lr=1e-3)
    st, info, vs = pol.ppo_update(opt, rec, adv, ret, epochs=2, minibatches=2, seed=7, clip_vloss=True)
    assert tuple(st.shape) == (4, 8) and tuple(vs.shape) == (4, 3)
    assert bool(torch.isfinite(st).all()) and bool(torch.isfinite(info).all()) and bool(torch.isfinite(vs).all())
    assert bool(((vs[:, 1:] >= 0) & (vs[:, 1:] <= 1)).all())
    # the recorded values reach the kernel: the first minibatch runs on unchanged weights, so no value has left the clip
    # range around its record, and other records give other statistics
    assert float(vs[0, 2]) == 0
    pol2 = BulldozerPolicy(env, 5, 8, 64, seed=3)
    shifted = {**rec, "value": rec["value"] + 1.0}
    _, _, vs2 = pol2.ppo_grad(shifted, adv, ret, clip_vloss=True)
    assert float(vs2[2]) == 1.0


SCRIPTS = {"helicopter": (["--envs", "8", "--steps", "8", "--updates", "2", "--graph"], "update "),
           "bulldozer": (["--envs", "4", "--rows", "32", "--steps", "8", "--iterations", "2"], "iteration "),
           "advanced": (["--envs", "4", "--rows", "32", "--cols", "256", "--steps", "8", "--iterations", "2", "--graph"],
                        "iteration ")}


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_training_scripts_take_clip_vloss(name):
    args, head = SCRIPTS[name]
    cmd = [sys.executable, os.path.join(ROOT, "scripts", f"train_{name}_ppo.py")] + args + ["--clip-vloss"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0
    lines = [l for l in out.stdout.splitlines() if l.startswith(head)]
    assert len(lines) == 2
    for l in lines:  # U and the two shares are on the printed line, the shares in [0, 1]
        m = re.search(r"U (\S+)  u-share (\S+)  v-clip (\S+)$", l)
        assert m, l
        U, us, vc = (float(x) for x in m.groups())
        assert np.isfinite(U) and 0 <= us <= 1 and 0 <= vc <= 1, l
