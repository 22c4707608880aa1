"""CPU: what only the bulldozer's PPO step of the host build has (the gradient against the yardstick, the argument
errors and the rest of what both agents share are in test_ppo_host.py): the reduction of the per-head loss to the
helicopter's one-head loss in closed form, the device build refusing as the host build does, and
BulldozerPolicy.ppo_grad / ppo_update on a device="cpu" policy."""
import ctypes

import numpy as np
import pytest

import _bulldozer_policy_ref as bref
import _ppo_ref as R

HELI, BDZ = R.HELI, R.BDZ


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("norm_adv", [True, False])
def test_constant_shoot_logits_reduce_to_the_one_head_loss(norm_adv):
    """A 12-output network whose two shoot logits are the same constant, with recorded shoot logits that are equal too:
    ratio_shoot = 1 exactly (never clipped), ent_shoot = ln 2 with a zero gradient, pg_shoot = -A^. Against the
    helicopter's host build on the trunk-sharing ten-output network (both sum in double and round once, so a tensor
    agrees within two roundings of its largest element):
      pg = (pg_heli - mean A^) / 2, entropy = (ent_heli + ln 2) / 2, approx_kl = kl_heli / 2, clip = clip_heli / 2,
      v_loss = v_loss_heli; the move columns of g_w_out / g_b2 are half the helicopter's, the value column equal;
      g_b2[9] = -(1 / 2N) sum_s A^_s (1[shoot_s = 0] - 1/2) = -g_b2[10], the shoot columns of g_w_out likewise with h_s."""
    ch = R.case(HELI, R.SHAPES[HELI][0])
    d, wh, T = ch["d"], ch["w"], ch["T"]
    w = bref.weights_from_helicopter(wh, seed=1)
    w["w_out"][:, 9:11] = 0
    w["b2"][9:11] = np.float32(0.75)
    rng = np.random.default_rng(7)
    shoot = rng.integers(0, 2, T).astype(np.int32)
    rec = {"local": ch["rec"]["local"], "coarse": ch["rec"]["coarse"],
           "action": np.stack([ch["rec"]["action"], shoot], 1).astype(np.int32),
           "logits": np.concatenate([ch["rec"]["logits"], np.full((T, 2), -0.3, np.float32)], 1)}
    idx = R.minibatch(ch, 257)
    ent_coef, vf_coef = 0.01, 0.5
    gh, sh = R.host_grad(HELI, wh, d, ch["rec"], ch["adv"], ch["ret"], idx, norm_adv=norm_adv)
    gb, sb = R.host_grad(BDZ, w, d, rec, ch["adv"], ch["ret"], idx, norm_adv=norm_adv)
    A = ch["adv"][idx].astype(np.float64)
    if norm_adv:
        A = (A - A.mean()) / (A.std() + 1e-8)
    N = len(idx)
    close = lambda got, want: np.all(np.abs(np.asarray(got, np.float64) - want) <= 2 * R.U * max(np.abs(want).max(), 1e-30)
                                     + 2 * R.U * np.abs(want))
    pg, ent = (float(sh[1]) - A.mean()) / 2, (float(sh[3]) + np.log(2.0)) / 2
    want = np.array([pg - ent_coef * ent + vf_coef * float(sh[2]), pg, sh[2], ent, sh[4] / 2, sh[5] / 2, sh[6], sh[7]])
    for i, k in enumerate(R.STATS):
        assert abs(float(sb[i]) - want[i]) <= 8 * R.U * max(abs(want[i]), 1.0), (k, sb[i], want[i])  # O(1) figures
    g_shoot = -(A * ((shoot[idx] == 0) - 0.5)).sum() / (2 * N)
    assert close(gb["b2"][9], np.array(g_shoot)) and close(gb["b2"][10], np.array(-g_shoot)) and g_shoot != 0
    assert close(gb["b2"][:9], gh["b2"][:9].astype(np.float64) / 2) and close(gb["b2"][11], gh["b2"][9].astype(np.float64))
    assert close(gb["w_out"][:, :9], gh["w_out"][:, :9].astype(np.float64) / 2)
    assert close(gb["w_out"][:, 11], gh["w_out"][:, 9].astype(np.float64))
    assert np.array_equal(gb["w_out"][:, 9], -gb["w_out"][:, 10]) and np.abs(gb["w_out"][:, 9]).max() > 0
    # the shoot columns of w_out are zero, so the hidden layer sees the move head at half weight and the value head
    # whole: without the value term its gradients are half the helicopter's
    gh0, _ = R.host_grad(HELI, wh, d, ch["rec"], ch["adv"], ch["ret"], idx, norm_adv=norm_adv, vf_coef=0.0)
    gb0, _ = R.host_grad(BDZ, w, d, rec, ch["adv"], ch["ret"], idx, norm_adv=norm_adv, vf_coef=0.0)
    for k in ("w_local", "w_coarse", "b1"):
        assert close(gb0[k], gh0[k].astype(np.float64) / 2), k


def test_both_builds_refuse_alike_without_a_gpu():
    """The device library makes the same checks before it touches the GPU: the same status and text for a refused
    call (host pointers are never read: every call here is refused by an argument check)."""
    from gymca_amd import _lib

    c = R.case(BDZ, R.SHAPES[BDZ][0])
    s, keep = bref.policy_struct(c["w"], c["d"])
    A = lambda i: 0x5000000 + 0x100000 * i
    base = [ctypes.byref(s), c["d"]["C"], A(0), A(1), A(2), A(3), A(4), A(5), 16, None, 4, 0.2, 0.01, 0.5, 1, A(6), A(7),
            A(8), A(9), A(10), A(11), A(12), 1 << 40, None]
    cases = {2: "null record", 5: "null record", 21: "null output or workspace", 8: "1 <= T < 2^31", 10: "N >= 1",
             22: "workspace smaller than gca_bulldozer_policy_grad_workspace", 1: "C = 2 Hc Wc, at most 15088"}
    for pos, text in cases.items():
        args = list(base)
        args[pos] = {8: 0, 10: 0, 22: 64, 1: 3}.get(pos)
        got = []
        for lib in (_lib.load_cpu(), _lib.load()):
            status = lib.gca_bulldozer_policy_grad(*args)
            got.append((status, lib.gca_last_error().decode()))
        assert got[0] == got[1] == (1, "argument: bulldozer_policy_grad: " + text), (pos, got)


def test_ppo_grad_python_surface_on_a_host_policy():
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy

    shape = R.SHAPES[BDZ][0]
    c = R.case(BDZ, shape)
    r, Bk, Hd, H, W = shape
    pol = BulldozerPolicy((H, W), r, Bk, Hd, device="cpu").load(c["w"])
    assert pol.HEADS == (9, 2) and pol.N_LOGITS == 11 and pol.GRAD_ENTRY == "gca_bulldozer_policy_grad"
    K, E = 4, c["T"] // 4
    rec = {k: torch.from_numpy(v.copy()).reshape((K, E) + v.shape[1:]) for k, v in c["rec"].items()}
    assert rec["action"].shape == (K, E, 2) and rec["logits"].shape == (K, E, 11)
    adv, ret = torch.from_numpy(c["adv"].copy()).reshape(K, E), torch.from_numpy(c["ret"].copy()).reshape(K, E)
    idx = torch.from_numpy(R.minibatch(c, 257))
    grads, stats = pol.ppo_grad(rec, adv, ret, idx)
    want, ws = R.host_grad(BDZ, c["w"], c["d"], c["rec"], c["adv"], c["ret"], idx.numpy())
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
    # idx = None: all T rows in order
    ga, sa = pol.ppo_grad(rec, adv, ret)
    gb, sb = pol.ppo_grad(rec, adv, ret, torch.arange(c["T"], dtype=torch.int32))
    assert all(torch.equal(ga[k], gb[k]) for k in R.GRADS) and torch.equal(sa, sb)
    v0 = pol.version
    pol.w_out.add_(grads["w_out"], alpha=-0.1)
    g3, _ = pol.ppo_grad(rec, adv, ret, idx)
    assert pol.version == v0 and not torch.equal(g3["w_out"], grads["w_out"])
    with pytest.raises(ValueError, match="workspace"):
        pol.ppo_grad(rec, adv, ret, idx, workspace=torch.empty(16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="advantage"):
        pol.ppo_grad(rec, adv[:, :-1], ret, idx)
    with pytest.raises(ValueError, match=r"records\['logits'\] must be a contiguous float32 tensor of 1200 x 11"):
        pol.ppo_grad({**rec, "logits": rec["logits"][..., :9].contiguous()}, adv, ret, idx)
    with pytest.raises(ValueError, match=r"records\['local'\]"):  # an action of one value per row: T is then 600
        pol.ppo_grad({**rec, "action": rec["action"][..., 0].contiguous()}, adv, ret, idx)
    with pytest.raises(ValueError, match="idx"):
        pol.ppo_grad(rec, adv, ret, idx.long())
    with pytest.raises(ValueError, match="lack"):
        pol.ppo_grad({k: v for k, v in rec.items() if k != "logits"}, adv, ret, idx)
    with pytest.raises(ValueError, match=r"grads_out\['b1'\]"):
        pol.ppo_grad(rec, adv, ret, idx, grads_out={**out, "b1": torch.zeros(3)})


def test_ppo_update_on_a_host_policy_equals_the_hand_written_loop():
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    shape = R.SHAPES[BDZ][0]
    c = R.case(BDZ, shape)
    r, Bk, Hd, H, W = shape

    def setup():
        pol = BulldozerPolicy((H, W), r, Bk, Hd, device="cpu").load(c["w"])
        return pol, ppo.Adam({n: getattr(pol, n) for n in WEIGHTS}, lr=1e-3)

    rec = {k: torch.from_numpy(v.copy()) for k, v in c["rec"].items()}
    adv, ret = torch.from_numpy(c["adv"].copy()), torch.from_numpy(c["ret"].copy())
    T, E, M = c["T"], 2, 3
    pol, opt = setup()
    stats, info = pol.ppo_update(opt, rec, adv, ret, epochs=E, minibatches=M, seed=5)
    assert stats.shape == (E * M, 8) and info.shape == (E * M, 2) and torch.isfinite(stats).all()
    pol2, opt2 = setup()
    perm = ppo.permutation(T, E, seed=5, counter=opt2.count)
    N = T // M
    for e in range(E):
        for mb in range(M):
            g, s = pol2.ppo_grad(rec, adv, ret, perm[e, mb * N:(mb + 1) * N])
            assert np.array_equal(_bits(s.numpy()), _bits(stats[e * M + mb].numpy()))
            opt2.step(g)
    assert all(np.array_equal(_bits(getattr(pol, n).numpy()), _bits(getattr(pol2, n).numpy())) for n in WEIGHTS)
    assert not np.array_equal(pol.w_out.numpy(), c["w"]["w_out"])
    with pytest.raises(ValueError, match="do not divide into 7 minibatches"):
        pol.ppo_update(opt, rec, adv, ret, epochs=1, minibatches=7)
