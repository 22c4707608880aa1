"""CPU: what the helicopter and the bulldozer agent share. The host build evaluates one network for both
(policy_outputs_host): with a shared trunk gca_helicopter_policy_act and gca_bulldozer_policy_act return the same nine
logits, value and move, bit for bit. HelicopterPolicy and BulldozerPolicy are one PolicyBase (load refuses the same
things with the same words), and both envs' cache of bound policy calls is the bounded one of BatchedEnvBase. No GPU."""
import numpy as np
import pytest

import _bulldozer_policy_ref as bref
import _helicopter_policy_ref as pref


@pytest.mark.parametrize("shape", bref.TRUNK_SHAPES)
def test_host_trunk_is_one_for_both_agents(shape):
    d, wh, wb, local, coarse = bref.trunk_case(shape)
    E = local.shape[0]
    assert E == 3 and not np.array_equal(wb["w_out"][:, 9:11], wh["w_out"][:, 8:10])
    heli = pref.host_act(wh, d, local, coarse, np.arange(E, dtype=np.uint32), greedy=True)
    bdz = bref.host_act(wb, d, local, coarse, np.arange(E, dtype=np.int64), greedy=True)
    bref.assert_same_trunk(heli, bdz)
    assert np.array_equal(heli[0], pref.greedy_ref(heli[1]))


def test_both_policies_load_refuses_alike():
    from gymca_amd.forest_fire._policy import PolicyBase
    from gymca_amd.forest_fire.bulldozer import BulldozerPolicy
    from gymca_amd.forest_fire.helicopter import HelicopterPolicy

    assert issubclass(HelicopterPolicy, PolicyBase) and issubclass(BulldozerPolicy, PolicyBase)
    assert not issubclass(HelicopterPolicy, BulldozerPolicy) and not issubclass(BulldozerPolicy, HelicopterPolicy)
    for cls, n_out in ((HelicopterPolicy, 10), (BulldozerPolicy, 12)):
        pol = cls((32, 256), 1, 8, 32, device="cpu")
        v0 = pol.version
        with pytest.raises(ValueError) as err:
            pol.load({**pol.state_dict(), "b2": np.zeros(n_out, np.int32)})   # integers are not cast silently
        assert str(err.value) == f"{cls.__name__}.load: b2 has dtype torch.int32, a float dtype is expected"
        assert pol.version == v0
        pol.load({k: v.double().numpy() for k, v in pol.state_dict().items()})  # any float dtype, arrays
        assert pol.version == v0 + 1 and pol.b2.dtype.is_floating_point and tuple(pol.b2.shape) == (n_out,)


def test_both_envs_policy_call_cache_is_bounded():
    """_policy_call is pure bookkeeping, so it runs on an env object that was never given a device: more policies than
    _POLICY_CALLS_MAX against one env do not all stay bound, the one bound longest ago goes first, a hit keeps its
    entry and a policy whose version moved is bound again."""
    from gymca_amd.forest_fire._batched import BatchedEnvBase
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv, BulldozerPolicy
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv, HelicopterPolicy

    for env_cls, pol_cls in ((BatchedForestFireHelicopterEnv, HelicopterPolicy),
                             (BatchedForestFireBulldozerEnv, BulldozerPolicy)):
        assert env_cls._policy_call is BatchedEnvBase._policy_call and env_cls._POLICY_CLASS is pol_cls
        env = object.__new__(env_cls)
        env._policy_calls = {}
        n_max = env._POLICY_CALLS_MAX
        assert n_max == 8
        made = []
        make = lambda: (made.append(1) or len(made),)
        pols = [pol_cls((32, 256), 0, 8, 32, seed=i, device="cpu") for i in range(n_max + 3)]
        first = env._policy_call("act", pols[0], make)
        assert first[:2] == (pols[0].version, pols[0]) and first[2] == 1
        for i, pol in enumerate(pols[1:], 1):
            if i == n_max - 1:
                assert env._policy_call("act", pols[0], make) is first   # a hit: no new call, moved to the end
            env._policy_call("act", pol, make)
            assert len(env._policy_calls) <= n_max
        assert len(made) == len(pols) and len(env._policy_calls) == n_max
        kept = [pc[1] for pc in env._policy_calls.values()]
        assert pols[0] in kept and pols[1] not in kept and pols[2] not in kept and pols[3] not in kept
        assert env._policy_call("act", pols[1], make)[2] == len(pols) + 1    # a dropped policy is bound again
        pols[0].b1 = pols[0].b1 + 1.0                                         # a replaced tensor moves the version
        again = env._policy_call("act", pols[0], make)
        assert again[0] == pols[0].version != first[0] and again[2] == len(pols) + 2
        assert len(env._policy_calls) == n_max
