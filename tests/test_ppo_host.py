"""CPU: the PPO update of the host build for both agents (gca_gae, gca_<agent>_policy_grad and its workspace query):
the GAE recurrence against its numpy float32 restatement bit for bit, the per-head loss gradient and statistics against
the float64 autograd yardstick of tests/_ppo_ref.py within 4 x the error of torch's own float32 autograd, every argument
error with its message, and the Python surface on a host policy. What only the bulldozer has is in
test_bulldozer_ppo_host.py. No GPU."""
import ctypes

import numpy as np
import pytest

import _policy_ref as P
import _ppo_ref as R

agents = pytest.mark.parametrize("agent", R.AGENTS, ids=repr)
# (N, norm_adv) of the gradient test, each agent's own
BATCHES = {R.HELI: ((1, True), (2, False), (65, True), (1000, True), (1000, False)),
           R.BDZ: ((1, True), (2, False), (65, True), (257, False), (1000, True))}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("mode", [None, "ones", "random"])
@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("K", [1, 2, 7])
def test_host_gae_equals_the_float32_restatement(K, E, mode):
    reward, value, nxt, term = R.gae_case(K, E, mode)
    want_a, want_r = R.gae_ref(reward, value, nxt, term, 0.99, 0.95)
    adv, ret = R.host_gae(reward, value, nxt, term, 0.99, 0.95)
    assert np.array_equal(_bits(adv), _bits(want_a)) and np.array_equal(_bits(ret), _bits(want_r))
    if mode == "ones":  # nothing is bootstrapped anywhere: A = r - v
        assert np.array_equal(adv, reward.astype(np.float32) - value)
    if mode == "random":  # next_value never enters: the last row is terminal
        adv2, _ = R.host_gae(reward, value, nxt + 5, term, 0.99, 0.95)
        assert np.array_equal(_bits(adv2), _bits(adv))


def test_gae_python_surface_on_host_arrays():
    from gymca_amd import GCAError
    from gymca_amd.forest_fire import ppo

    reward, value, nxt, term = R.gae_case(7, 5, "random")
    want = R.gae_ref(reward, value, nxt, term, 0.9, 0.8)
    adv, ret = ppo.gae(reward, value, nxt, 0.9, 0.8, terminal=term)
    assert np.array_equal(_bits(adv), _bits(want[0])) and np.array_equal(_bits(ret), _bits(want[1]))
    a2, r2 = np.empty_like(adv), np.empty_like(ret)
    got = ppo.gae(reward, value, nxt, 0.9, 0.8, terminal=term, adv_out=a2, ret_out=r2)
    assert got[0] is a2 and got[1] is r2 and np.array_equal(_bits(a2), _bits(adv))
    with pytest.raises(ValueError, match="reward"):
        ppo.gae(reward.astype(np.float32), value, nxt)
    with pytest.raises(ValueError, match="next_value"):
        ppo.gae(reward, value, nxt[:-1])
    # K == 0 is a no-op; K < 0 an argument error, reported before anything runs
    adv0, _ = R.host_gae(reward, value, nxt, None, 0.99, 0.95, K=0)
    assert np.isnan(adv0).all()
    with pytest.raises(GCAError, match=r"argument: gae: K >= 0$"):
        R.host_gae(reward, value, nxt, None, 0.99, 0.95, K=-1)
    assert ppo.STATS == R.STATS


@pytest.mark.parametrize("agent, shape", R.params())
def test_host_gradient_against_the_float64_yardstick(agent, shape):
    c = R.case(agent, shape)
    R.check_case(c)
    for N, norm_adv in BATCHES[agent]:
        idx = R.minibatch(c, N)
        args = (c["w"], c["d"], c["rec"], c["adv"], c["ret"], idx)
        g64, s64, _, _ = R.loss_and_grad(*args, agent.heads, norm_adv=norm_adv)
        g32, s32, _, _ = R.loss_and_grad(*args, agent.heads, norm_adv=norm_adv, dtype="float32")
        grads, stats = R.host_grad(agent, *args, norm_adv=norm_adv)
        assert all(np.isfinite(g).all() for g in grads.values()) and np.isfinite(stats).all()
        R.assert_within(R.errors(grads, stats, g64, s64), R.errors(g32, s32, g64, s64), f"{shape} N={N} {norm_adv}")
        # a (cell, class) row the minibatch never selects is exactly zero
        cls = c["rec"]["local"].reshape(c["T"], -1)[idx] & 3
        absent = np.ones((c["d"]["SS"], 4), bool)
        absent[np.arange(c["d"]["SS"])[None, :].repeat(N, 0), cls] = False
        assert (grads["w_local"][absent] == 0).all() and (N > 2 or absent.any())
        if N == 1:
            assert stats[1] == 0 and stats[7] == 0  # the normalised advantage of one sample is zero
    # idx = None is rows 0 .. N - 1 (all T rows on the host: every helicopter shape, the bulldozer's smallest)
    if agent is R.HELI or shape == R.SHAPES[agent][0]:
        rows = np.arange(c["T"], dtype=np.int32)
        a, sa = R.host_grad(agent, c["w"], c["d"], c["rec"], c["adv"], c["ret"], None)
        b, sb = R.host_grad(agent, c["w"], c["d"], c["rec"], c["adv"], c["ret"], rows)
        assert all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in R.GRADS) and np.array_equal(_bits(sa), _bits(sb))


def _one_sample(agent):
    c = R.case(agent, R.SHAPES[agent][0])
    idx = R.minibatch(c, 1)
    grads, stats = R.host_grad(agent, c["w"], c["d"], c["rec"], c["adv"], c["ret"], idx, ent_coef=0.0, vf_coef=0.0)
    assert stats[1] == 0 and stats[7] == 0 and all((g == 0).all() for g in grads.values())


def test_normalised_advantage_of_one_sample_is_zero():  # the helicopter's, under the name it has always had
    _one_sample(R.HELI)


def test_normalised_advantage_of_one_sample_is_zero_bulldozer():
    _one_sample(R.BDZ)


@agents
def test_argument_errors_and_their_messages(agent):
    from gymca_amd import GCAError, _lib

    c = R.case(agent, R.SHAPES[agent][0])
    w, d, rec, adv, ret, T = c["w"], c["d"], c["rec"], c["adv"], c["ret"], c["T"]
    name = agent.entry[len("gca_"):]  # helicopter_policy, bulldozer_policy
    who = f"argument: {name}_grad: "

    def refused(text, **kw):
        with pytest.raises(GCAError) as e:
            R.host_grad(agent, kw.pop("w", w), kw.pop("d", d), rec, adv, ret, kw.pop("idx", None), **kw)
        assert str(e.value).endswith(text), str(e.value)

    for record in ("local", "coarse", "action", "logits", "advantage", "returns"):
        refused(who + "null record", null=record)
    refused(who + f"workspace smaller than {agent.entry}_grad_workspace", ws_bytes=64)
    refused(who + "workspace, w_local, w_coarse and b1 16-B aligned", ws_offset=4)
    refused(who + "the outputs may alias neither each other nor the weights", alias="outputs")
    refused(who + "the outputs may alias neither each other nor the weights", alias="weights")
    refused(who + "idx outside [0, T)", idx=np.array([0, T], np.int32))
    refused(who + "idx outside [0, T)", idx=np.array([-1], np.int32))
    refused(who + "N <= T without idx", N=T + 1)
    refused(who + "N >= 1", N=0)
    refused(who + "1 <= T < 2^31", T=0)
    refused(who + "clip_coef >= 0", clip_coef=-0.1)
    # the one message the two entry points word differently
    refused({R.HELI: "argument: helicopter_policy: hidden must be a power of two in [32, 256]",
             R.BDZ: who + "policy.hidden must be a power of two in [32, 256]"}[agent], d={**d, "hidden": 48})
    # which check fires first when several fail; a refused call has written nothing
    refused(who + "null record", null="action", N=T + 1, ws_bytes=64)
    refused(who + "N <= T without idx", N=T + 1, ws_bytes=64)
    # the workspace query: bytes, growing with N; < 0 with the message on an argument error
    s, keep = P.policy_struct(w, d)
    lib = _lib.load_cpu()
    q = lambda N: getattr(lib, agent.entry + "_grad_workspace")(ctypes.byref(s), d["C"], N)
    tile = R.kernel_tile(lib, c)
    assert 0 < q(1) == q(tile) < q(tile + 1) < q(100000) and tile > 1
    assert q(0) == -1 and {R.HELI: b"helicopter_policy_grad_workspace",
                           R.BDZ: b"argument: bulldozer_policy_grad_workspace: radius in [0, 31]"}[agent] \
        in lib.gca_last_error()
    assert len(_lib._SIGNATURES[agent.entry + "_grad"][0]) == 24
    if agent is R.HELI:
        assert {"gca_gae", "gca_helicopter_policy_grad", "gca_helicopter_policy_grad_workspace"} <= set(_lib.CPU_SYMBOLS)
    else:  # two heads' partials: larger than the helicopter's on the same network
        assert q(1) > lib.gca_helicopter_policy_grad_workspace(ctypes.byref(s), d["C"], 1)
        assert {"gca_bulldozer_policy_grad", "gca_bulldozer_policy_grad_workspace"} <= set(_lib.CPU_BULLDOZER_POLICY_SYMBOLS)


def test_ppo_grad_python_surface_on_a_host_policy():
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.helicopter import HelicopterPolicy

    shape = R.SHAPES[R.HELI][0]
    c = R.case(R.HELI, shape)
    r, B, Hd, H, W = shape
    pol = HelicopterPolicy((H, W), r, B, Hd, device="cpu").load(c["w"])
    K, E = 4, c["T"] // 4
    rec = {k: torch.from_numpy(v.copy()).reshape((K, E) + v.shape[1:]) for k, v in c["rec"].items()}
    adv, ret = torch.from_numpy(c["adv"].copy()).reshape(K, E), torch.from_numpy(c["ret"].copy()).reshape(K, E)
    idx = torch.from_numpy(R.minibatch(c, 257))
    grads, stats = pol.ppo_grad(rec, adv, ret, idx)
    want, ws = R.host_grad(R.HELI, c["w"], c["d"], c["rec"], c["adv"], c["ret"], idx.numpy())
    assert set(grads) == set(R.GRADS) and {k: tuple(v.shape) for k, v in grads.items()} == pol.weight_shapes()
    assert all(np.array_equal(_bits(grads[k].numpy()), _bits(want[k])) for k in R.GRADS)
    assert stats.dtype is torch.float32 and tuple(stats.shape) == (8,) and len(ppo.STATS) == 8
    assert np.array_equal(_bits(stats.numpy()), _bits(ws))
    # the caller's outputs and workspace; flattened records; an in-place update keeps the bound addresses
    out = {k: torch.full_like(v, float("nan")) for k, v in grads.items()}
    st = torch.empty(8)
    flat = {k: v.reshape((K * E,) + v.shape[2:]) for k, v in rec.items()}
    g2, s2 = pol.ppo_grad(flat, adv.reshape(-1), ret.reshape(-1), idx, grads_out=out, stats_out=st,
                          workspace=torch.empty(1 << 22, dtype=torch.uint8))
    assert s2 is st and all(g2[k] is out[k] and torch.equal(out[k], grads[k]) for k in R.GRADS)
    v0 = pol.version
    pol.w_out.add_(grads["w_out"], alpha=-0.1)
    g3, _ = pol.ppo_grad(rec, adv, ret, idx)
    assert pol.version == v0 and not torch.equal(g3["w_out"], grads["w_out"])
    with pytest.raises(ValueError, match="workspace"):
        pol.ppo_grad(rec, adv, ret, idx, workspace=torch.empty(16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="advantage"):
        pol.ppo_grad(rec, adv[:, :-1], ret, idx)
    with pytest.raises(ValueError, match="idx"):
        pol.ppo_grad(rec, adv, ret, idx.long())
    with pytest.raises(ValueError, match="lack"):
        pol.ppo_grad({k: v for k, v in rec.items() if k != "logits"}, adv, ret, idx)
    with pytest.raises(ValueError, match=r"grads_out\['b1'\]"):
        pol.ppo_grad(rec, adv, ret, idx, grads_out={**out, "b1": torch.zeros(3)})
