"""CPU: the learner's clipped value loss in the host build (gca_<agent>_policy_grad_vclip) for both agents: gradients,
the eight statistics and U against the float64 autograd yardstick of tests/_ppo_vclip_ref.py within 4 x the error of
torch's own float32 autograd, the two shares exactly, vf_coef = 0 against the plain entry, one inside sample against the
plain loss, every new refusal, and the Python surface (clip_vloss) on a host policy. No GPU."""
import numpy as np
import pytest

import _ppo_ref as R
import _ppo_vclip_ref as V

agents = pytest.mark.parametrize("agent", R.AGENTS, ids=repr)
PICK = {R.HELI: (0, 1), R.BDZ: (0, 1)}  # each agent's first two shapes
SIZES = (1, 2, 65, 300)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("agent, shape", R.params(pick=PICK))
def test_host_vclip_against_the_float64_yardstick(agent, shape):
    c = V.case(agent, shape)
    R.check_case(c)
    assert len(c["vrows"]) >= 0.85 * c["T"]
    for N in SIZES:
        for norm_adv in (True, False):
            idx, f64, f32 = V.minibatch(c, N, norm_adv)
            where = f"{agent} {shape} N={N} norm_adv={norm_adv}"
            grads, stats, vs = V.host_grad(agent, c["w"], c["d"], c["rec"], c["adv"], c["ret"], c["vo"], idx,
                                           norm_adv=norm_adv)
            assert all(np.isfinite(g).all() for g in grads.values()) and np.isfinite(stats).all()
            R.assert_within(V.errors(grads, stats, vs, f64), V.yard_errors(f32, f64), where)
            V.assert_shares(vs, f64, N, where)
            if N >= 65:  # the clipped loss is not the plain one here
                assert abs(f64[1][2] - R.loss_and_grad(c["w"], c["d"], c["rec"], c["adv"], c["ret"], idx, agent.heads,
                                                       norm_adv=norm_adv)[1][2]) > 1e-3
    # a null vstats is allowed and changes nothing else
    idx, _, _ = V.minibatch(c, 65)
    a = V.host_grad(agent, c["w"], c["d"], c["rec"], c["adv"], c["ret"], c["vo"], idx)
    b = V.host_grad(agent, c["w"], c["d"], c["rec"], c["adv"], c["ret"], c["vo"], idx, vstats=False)
    assert all(np.array_equal(_bits(a[0][k]), _bits(b[0][k])) for k in R.GRADS) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.isnan(b[2]).all()


@agents
def test_host_vclip_with_vf_coef_zero_equals_the_plain_entry(agent):
    c = V.case(agent, R.SHAPES[agent][0])
    idx, _, _ = V.minibatch(c, 300)
    args = (agent, c["w"], c["d"], c["rec"], c["adv"], c["ret"])
    g, s, _ = V.host_grad(*args, c["vo"], idx, vf_coef=0.0)
    gp, sp = R.host_grad(*args, idx, vf_coef=0.0)
    for k in R.GRADS:
        assert np.array_equal(g[k], gp[k]), k  # as numbers: -0.0 == 0.0
    for i in (1, 3, 4, 5, 6, 7):
        assert s[i] == sp[i], R.STATS[i]
    assert s[0] == sp[0] and s[2] != sp[2]  # the loss has no value term; v_loss is the clipped one


@agents
def test_one_inside_sample_is_the_plain_loss(agent):
    c = V.case(agent, R.SHAPES[agent][0])
    inside = np.abs(c["v64"] - c["vo"]) < c["clip_coef"]
    row = int(c["vrows"][inside[c["vrows"]]][0])
    idx = np.array([row], np.int32)
    args = (c["w"], c["d"], c["rec"], c["adv"], c["ret"])
    g64, s64, _, _ = R.loss_and_grad(*args, idx, agent.heads)  # the PLAIN yardstick
    g32, s32, _, _ = R.loss_and_grad(*args, idx, agent.heads, dtype="float32")
    g, s, vs = V.host_grad(agent, *args, c["vo"], idx)
    R.assert_within(R.errors(g, s, g64, s64), R.errors(g32, s32, g64, s64), f"{agent} one inside sample")
    assert vs[1] == 0 and vs[2] == 0 and abs(vs[0] - s[2]) <= 1e-6 * abs(s[2])


@agents
def test_vclip_refusals_and_their_messages(agent):
    from gymca_amd import GCAError, _lib

    c = V.case(agent, R.SHAPES[agent][0])
    w, d, rec, adv, ret, vo, T = c["w"], c["d"], c["rec"], c["adv"], c["ret"], c["vo"], c["T"]
    who = f"argument: {agent.entry[len('gca_'):]}_grad_vclip: "

    def refused(text, **kw):
        with pytest.raises(GCAError) as e:
            V.host_grad(agent, w, d, rec, adv, ret, vo, kw.pop("idx", None), **kw)
        assert str(e.value).endswith(text), str(e.value)

    refused(who + "null record", null="value")
    refused(who + "null record", null="logits")
    refused(who + f"workspace smaller than {agent.entry}_grad_workspace", ws_bytes=64)
    refused(who + "the outputs may alias neither each other nor the weights", alias="vstats")
    refused(who + "idx outside [0, T)", idx=np.array([0, T], np.int32))
    refused(who + "idx outside [0, T)", idx=np.array([-1], np.int32))
    refused(who + "N <= T without idx", N=T + 1)
    assert len(_lib._SIGNATURES[agent.entry + "_grad_vclip"][0]) == 26
    assert agent.entry + "_grad_vclip" in _lib.CPU_VCLIP_SYMBOLS and agent.entry + "_grad_vclip" in _lib.EXPORTED_SYMBOLS


def _host_policy(agent, c, K=4):
    import torch

    d = c["d"]
    pol = agent.policy_class()((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device="cpu").load(c["w"])
    E = c["T"] // K
    rec = {k: torch.from_numpy(v.copy()).reshape((K, E) + v.shape[1:]) for k, v in c["rec"].items()}
    adv, ret = torch.from_numpy(c["adv"].copy()).reshape(K, E), torch.from_numpy(c["ret"].copy()).reshape(K, E)
    return pol, rec, adv, ret, torch.from_numpy(c["vo"].copy()).reshape(K, E)


@agents
def test_ppo_grad_clip_vloss_on_a_host_policy(agent):
    import torch

    from gymca_amd.forest_fire import ppo

    assert ppo.VSTATS == V.VSTATS == ("v_loss_unclipped", "u_share", "v_clip_fraction")
    c = V.case(agent, R.SHAPES[agent][0])
    pol, rec, adv, ret, vo = _host_policy(agent, c)
    idx_np, _, _ = V.minibatch(c, 300)
    idx = torch.from_numpy(idx_np)
    with_value = {**rec, "value": vo}
    grads, stats, vstats = pol.ppo_grad(with_value, adv, ret, idx, clip_vloss=True)
    want = V.host_grad(agent, c["w"], c["d"], c["rec"], c["adv"], c["ret"], c["vo"], idx_np)
    assert all(np.array_equal(_bits(grads[k].numpy()), _bits(want[0][k])) for k in R.GRADS)
    assert np.array_equal(_bits(stats.numpy()), _bits(want[1])) and np.array_equal(_bits(vstats.numpy()), _bits(want[2]))
    vs = torch.full((3,), float("nan"))
    out = pol.ppo_grad(with_value, adv, ret, idx, clip_vloss=True, vstats_out=vs)
    assert out[2] is vs and torch.equal(vs, vstats)
    # the refusals of the Python surface
    with pytest.raises(ValueError, match=r"lack \['value'\]"):
        pol.ppo_grad(rec, adv, ret, idx, clip_vloss=True)
    with pytest.raises(ValueError, match=r"records\['value'\]"):
        pol.ppo_grad({**rec, "value": vo.double()}, adv, ret, idx, clip_vloss=True)
    with pytest.raises(ValueError, match=r"records\['value'\]"):
        pol.ppo_grad({**rec, "value": vo[:, :-1].contiguous()}, adv, ret, idx, clip_vloss=True)
    with pytest.raises(ValueError, match="vstats_out"):
        pol.ppo_grad(with_value, adv, ret, idx, clip_vloss=True, vstats_out=torch.zeros(4))
    with pytest.raises(ValueError, match="vstats_out"):
        pol.ppo_grad(with_value, adv, ret, idx, vstats_out=vs)
    # clip_vloss=False: "value" is not looked at, whatever it holds
    plain = pol.ppo_grad(rec, adv, ret, idx)
    for junk in (vo, "not a tensor", vo.double()[:, :3]):
        g, s = pol.ppo_grad({**rec, "value": junk}, adv, ret, idx)
        assert all(np.array_equal(_bits(g[k].numpy()), _bits(plain[0][k].numpy())) for k in R.GRADS)
        assert np.array_equal(_bits(s.numpy()), _bits(plain[1].numpy()))


def test_ppo_update_clip_vloss_on_a_host_policy():
    import torch

    from gymca_amd.forest_fire import ppo

    agent = R.HELI
    c = V.case(agent, R.SHAPES[agent][0])

    def run(value, **kw):
        pol, rec, adv, ret, vo = _host_policy(agent, c)
        opt = ppo.Adam(pol.state_dict(), lr=1e-3)
        if value:
            rec = {**rec, "value": vo}
        out = pol.ppo_update(opt, rec, adv, ret, epochs=2, minibatches=2, seed=3, **kw)
        return out, [t.clone() for t in pol.tensors()]

    (s0, i0), w0 = run(False)
    (s1, i1), w1 = run(True)  # clip_vloss=False: a "value" record changes no bit
    assert np.array_equal(_bits(s0.numpy()), _bits(s1.numpy())) and np.array_equal(_bits(i0.numpy()), _bits(i1.numpy()))
    assert all(np.array_equal(_bits(a.numpy()), _bits(b.numpy())) for a, b in zip(w0, w1))
    vs_out = torch.full((4, 3), float("nan"))
    (s2, i2, vs), w2 = run(True, clip_vloss=True, vstats_out=vs_out)
    assert vs is vs_out and tuple(s2.shape) == (4, 8) and tuple(i2.shape) == (4, 2)
    assert torch.isfinite(vs).all() and ((vs[:, 1:] >= 0) & (vs[:, 1:] <= 1)).all() and (vs[:, 0] > 0).all()
    assert not np.array_equal(_bits(s2.numpy()[:, 2]), _bits(s0.numpy()[:, 2]))  # another value loss
    assert any(not torch.equal(a, b) for a, b in zip(w0, w2))
    with pytest.raises(ValueError, match="value"):
        run(False, clip_vloss=True)
    with pytest.raises(ValueError, match="vstats_out"):
        run(True, clip_vloss=True, vstats_out=torch.zeros(3, 3))
