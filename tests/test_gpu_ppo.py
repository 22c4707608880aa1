"""GPU: the PPO update on the device, for both agents. forest_fire.ppo.gae (gca_gae) against the host build bit for
bit; <Agent>Policy.ppo_grad (gca_<agent>_policy_grad) against the float64 autograd yardstick of tests/_ppo_ref.py (the
per-head loss) within 4 x the error of torch's own float32 autograd (and against the host build), every element
written, exact zeros where no sample selects a class, equal bits across calls, idx=None, graph capture, several tiles
per split, and the helicopter's loop end to end on an env's records. All but the last on synthetic records of T = 1200
rows. The bulldozer's ppo_update and its end-to-end loop are in test_gpu_bulldozer_ppo.py."""
import numpy as np
import pytest

import _helicopter_policy_ref as pref
import _ppo_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, device):
    import torch

    return None if a is None else torch.from_numpy(np.array(a)).to(device)


@pytest.mark.parametrize("mode", [None, "ones", "random"])
@pytest.mark.parametrize("E", [1, 5, 257])
@pytest.mark.parametrize("K", [1, 2, 7])
def test_gae_equals_the_host_build(device, K, E, mode):
    import torch

    from gymca_amd.forest_fire import ppo

    reward, value, nxt, term = R.gae_case(K, E, mode)
    want_a, want_r = R.host_gae(reward, value, nxt, term, 0.99, 0.95)
    assert np.array_equal(_bits(want_a), _bits(R.gae_ref(reward, value, nxt, term, 0.99, 0.95)[0]))
    adv = torch.full((K, E), float("nan"), device=device)
    ret = torch.full((K, E), float("nan"), device=device)
    got = ppo.gae(_dev(reward, device), _dev(value, device), _dev(nxt, device), 0.99, 0.95, terminal=_dev(term, device),
                  adv_out=adv, ret_out=ret)
    assert got[0] is adv and got[1] is ret
    assert np.array_equal(_bits(adv.cpu().numpy()), _bits(want_a))
    assert np.array_equal(_bits(ret.cpu().numpy()), _bits(want_r))
    a2, _ = ppo.gae(_dev(reward, device), _dev(value, device), _dev(nxt, device), terminal=_dev(term, device))
    assert torch.equal(a2, adv)
    with pytest.raises(ValueError, match="reward"):
        ppo.gae(_dev(reward, device).float(), _dev(value, device), _dev(nxt, device))


def _policy(device, c):
    d = c["d"]
    return c["agent"].policy_class()((d["H"], d["W"]), d["radius"], d["block"], d["hidden"], device=device).load(c["w"])


def _records(device, c):
    return ({k: _dev(v, device) for k, v in c["rec"].items()}, _dev(c["adv"], device), _dev(c["ret"], device))


def _nan_outputs(pol):
    import torch

    grads = {k: torch.full(s, float("nan"), device=pol.device) for k, s in pol.weight_shapes().items()}
    return grads, torch.full((8,), float("nan"), device=pol.device)


# Each agent's own minibatch sizes beside those around the kernels' sample tile ts, and those that run without the
# normalisation too (beside ts + 1): the union would only add time at radius 31.
SIZES = {R.HELI: {1, 2, 63, 64, 65, 257, 1000}, R.BDZ: {1, 2, 257, 1000}}
BOTH_NORMS = {R.HELI: {1, 65, 1000}, R.BDZ: {1, 1000}}


@pytest.mark.parametrize("agent, shape", R.params())
def test_ppo_grad_against_the_float64_yardstick(device, agent, shape):
    from gymca_amd import _lib

    c = R.case(agent, shape)
    R.check_case(c)
    pol = _policy(device, c)
    rec, adv, ret = _records(device, c)
    ts = R.kernel_tile(_lib.load(), c)  # the kernels' own sample tile
    assert ts > 1
    worst = {}
    for N in sorted(SIZES[agent] | {ts - 1, ts, ts + 1}):
        idx = R.minibatch(c, N)
        assert idx[0] == 3 and (N < 257 or len(np.unique(idx)) < N)  # the class byte 7 is in; repeats
        cls = c["rec"]["local"].reshape(c["T"], -1)[idx] & 3
        if N >= 257:
            assert all((cls == k).any() for k in range(4))
        absent = np.ones((c["d"]["SS"], 4), bool)
        absent[np.arange(c["d"]["SS"])[None, :].repeat(N, 0), cls] = False
        for norm_adv in ((True, False) if N in BOTH_NORMS[agent] | {ts + 1} else (True,)):
            args = (c["w"], c["d"], c["rec"], c["adv"], c["ret"], idx)
            g64, s64, _, _ = R.loss_and_grad(*args, agent.heads, norm_adv=norm_adv)
            g32, s32, _, _ = R.loss_and_grad(*args, agent.heads, norm_adv=norm_adv, dtype="float32")
            gh, sh = R.host_grad(agent, *args, norm_adv=norm_adv)
            grads, stats = _nan_outputs(pol)
            pol.ppo_grad(rec, adv, ret, _dev(idx, device), norm_adv=norm_adv, grads_out=grads, stats_out=stats)
            got = {k: v.cpu().numpy() for k, v in grads.items()}
            st = stats.cpu().numpy()
            assert all(np.isfinite(g).all() for g in got.values()) and np.isfinite(st).all()
            assert (got["w_local"][absent] == 0).all() and (N > 2 or absent.any())
            where = f"{agent} {shape} N={N} norm_adv={norm_adv}"
            e, e32 = R.errors(got, st, g64, s64), R.errors(g32, s32, g64, s64)
            R.assert_within(e, e32, where)
            R.assert_within(R.errors(got, st, {k: gh[k].astype(np.float64) for k in gh}, sh.astype(np.float64)), e32,
                            where + " vs host")
            for k in e:
                worst[k] = max(worst.get(k, 0.0), e[k] / max(e32[k], R.FLOOR / R.MARGIN))
            if N == 1 and norm_adv:
                assert st[1] == 0 and st[7] == 0  # the normalised advantage of one sample is zero
    print(f"{agent} {shape} worst kernel / max(torch-f32, floor / 4):", {k: round(v, 2) for k, v in worst.items()})


@pytest.mark.parametrize("agent, shape", R.params(pick={R.HELI: (1, 5), R.BDZ: (1, 3)}))
def test_ppo_grad_is_reproducible_and_capturable(device, agent, shape):
    import torch

    c = R.case(agent, shape)
    pol = _policy(device, c)
    rec, adv, ret = _records(device, c)
    idx = _dev(R.minibatch(c, 333), device)
    g1, s1 = pol.ppo_grad(rec, adv, ret, idx)
    g2, s2 = _nan_outputs(pol)
    pol.ppo_grad(rec, adv, ret, idx, grads_out=g2, stats_out=s2)
    assert all(torch.equal(g1[k].view(torch.int32), g2[k].view(torch.int32)) for k in g1)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    # idx = None is rows 0 .. T - 1 (undecided rows included: both calls take the same side of every kink)
    ga, sa = pol.ppo_grad(rec, adv, ret, None)
    gb, sb = pol.ppo_grad(rec, adv, ret, torch.arange(c["T"], dtype=torch.int32, device=device))
    assert all(torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)) for k in ga)
    assert torch.equal(sa.view(torch.int32), sb.view(torch.int32))
    # inside a graph capture: no allocation, no sync; the replay gives the same bits
    g3, s3 = _nan_outputs(pol)
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pol.ppo_grad(rec, adv, ret, idx, grads_out=g3, stats_out=s3)
    for t in list(g3.values()) + [s3]:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize(device)
    assert all(torch.equal(g1[k].view(torch.int32), g3[k].view(torch.int32)) for k in g1)
    assert torch.equal(s1.view(torch.int32), s3.view(torch.int32))
    # a replaced tensor moves the version and is bound; an in-place update is seen without binding again
    v0 = pol.version
    pol.b2.add_(0.25)
    g4, _ = pol.ppo_grad(rec, adv, ret, idx)
    assert pol.version == v0 and not torch.equal(g4["b2"], g1["b2"])
    pol.b2 = pol.b2 - 0.25
    assert pol.version == v0 + 1
    g5, _ = pol.ppo_grad(rec, adv, ret, idx)
    assert torch.allclose(g5["b2"], g1["b2"], atol=1e-6)
    with pytest.raises(ValueError, match="idx"):
        pol.ppo_grad(rec, adv, ret, idx.cpu())


def test_rollout_gae_ppo_grad_end_to_end(device):
    import torch

    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv, HelicopterPolicy

    shape = pref.SHAPES[0]
    r, B, Hd, H, W = shape
    d = pref.dims(*shape)
    E, K = 8, 6
    env = BatchedForestFireHelicopterEnv(E, H, W, device=device, seed=5, materialize_obs=False)
    env.reset(grids=pref.grids(E, H, W, 3))
    w = pref.make_weights(d, seed=3, head=2.0)
    pol = HelicopterPolicy(env, r, B, Hd).load(w)
    rec = env.rollout_policy(pol, K, seed=11)
    _, _, next_value = env.act(pol, seed=11)
    adv, ret = ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95)
    want_a, want_r = R.host_gae(rec["reward"].cpu().numpy(), rec["value"].cpu().numpy(), next_value.cpu().numpy(), None,
                                0.99, 0.95)
    assert np.array_equal(_bits(adv.cpu().numpy()), _bits(want_a))
    assert np.array_equal(_bits(ret.cpu().numpy()), _bits(want_r))
    grads, stats = pol.ppo_grad(rec, adv, ret)
    st = stats.cpu().numpy()
    host = {k: v.cpu().numpy() for k, v in rec.items()}
    rows = np.arange(K * E)
    g64, s64, _, _ = R.loss_and_grad(w, d, host, want_a, want_r, rows, R.HELI.heads)
    g32, s32, _, _ = R.loss_and_grad(w, d, host, want_a, want_r, rows, R.HELI.heads, dtype="float32")
    # the weights are unchanged, so every ratio the kernel forms is 1 within rounding: nothing is clipped, and
    # approx_kl = mean((r - 1) - log r) ~ mean((r - 1)^2) / 2 bounds the kernel's own |ratio - 1| in the mean square;
    # 1e-10 is (1.4e-5)^2 / 2, a hundred roundings of a logit of a few units
    assert st[5] == 0 and 0 <= st[4] < 1e-10, (st[4], st[5])
    # with ratio = 1 and normalised advantages pg is -mean(A^), zero but for rounding: an absolute figure
    assert abs(st[1]) < 1e-6 and abs(s64[1]) < 1e-6
    e = R.errors({k: v.cpu().numpy() for k, v in grads.items()}, st, g64, s64)
    e32 = R.errors(g32, s32, g64, s64)
    keep = ("loss", "v_loss", "entropy", "adv_mean", "adv_std", "b2", "w_out")  # w_local / w_coarse / b1: relu kinks
    R.assert_within({k: e[k] for k in keep}, e32, "end to end")


def _many_tiles(device, agent, picks):
    """The production path the small cases never reach: several tiles per split in wgrad (LDS staged again per tile,
    the split's running sum) and more than 256 tile partials in reduce. With at least three row blocks there are at
    most 341 splits, so more than 341 tiles means more than one tile per split, whatever the shape."""
    from gymca_amd import _lib

    for si in picks:
        shape = R.SHAPES[agent][si]
        c = R.case(agent, shape)
        ts = R.kernel_tile(_lib.load(), c)
        N = 342 * ts + 5
        idx = R.minibatch(c, N)
        pol = _policy(device, c)
        rec, adv, ret = _records(device, c)
        args = (c["w"], c["d"], c["rec"], c["adv"], c["ret"], idx)
        g64, s64, _, _ = R.loss_and_grad(*args, agent.heads)
        g32, s32, _, _ = R.loss_and_grad(*args, agent.heads, dtype="float32")
        grads, stats = _nan_outputs(pol)
        pol.ppo_grad(rec, adv, ret, _dev(idx, device), grads_out=grads, stats_out=stats)
        got = {k: v.cpu().numpy() for k, v in grads.items()}
        assert all(np.isfinite(g).all() for g in got.values())
        R.assert_within(R.errors(got, stats.cpu().numpy(), g64, s64), R.errors(g32, s32, g64, s64),
                        f"{agent} {shape} N={N}")


def test_ppo_grad_many_tiles_per_split(device):  # the helicopter's, under the name it has always had
    _many_tiles(device, R.HELI, (1, 5))


def test_ppo_grad_many_tiles_per_split_bulldozer(device):  # its two smallest networks
    _many_tiles(device, R.BDZ, (0, 1))
