"""The learner's side of a PPO loop on the batched envs' records (include/gca.h "PPO update"): gae(), the reference's
generalised advantage estimate (agents/jax_ppo.py:932-984) in one launch, and the names of the eight statistics that
HelicopterPolicy.ppo_grad returns beside the gradients."""
import numpy as np

from .. import _device as dev
from .._lib import call, call_cpu
from ._batched import check_tensor

STATS = ("loss", "pg_loss", "v_loss", "entropy", "approx_kl", "clip_fraction", "adv_mean", "adv_std")


def gamma_lambda(gamma, gae_lambda):
    """float32(gamma * gae_lambda) with the product in double, as jax's weak-typed Python scalars give it."""
    return float(np.float32(float(gamma) * float(gae_lambda)))


def _gae_host(reward, value, next_value, gamma, gae_lambda, terminal, adv_out, ret_out):
    K, E = value.shape
    reward = _host_array(reward, np.float64, (K, E), "reward")
    value = _host_array(value, np.float32, (K, E), "value")
    next_value = _host_array(next_value, np.float32, (E,), "next_value")
    terminal = None if terminal is None else _host_array(terminal, np.uint8, (K, E), "terminal")
    adv_out = np.empty((K, E), np.float32) if adv_out is None else _host_array(adv_out, np.float32, (K, E), "adv_out")
    ret_out = np.empty((K, E), np.float32) if ret_out is None else _host_array(ret_out, np.float32, (K, E), "ret_out")
    p = lambda a: None if a is None else a.ctypes.data
    call_cpu("gca_gae", p(reward), p(value), p(next_value), p(terminal), float(gamma), gamma_lambda(gamma, gae_lambda),
             K, E, p(adv_out), p(ret_out), None)
    return adv_out, ret_out


def _host_array(a, dtype, shape, what):
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == tuple(shape) and a.flags.c_contiguous):
        raise ValueError(f"gae: {what} must be a C-contiguous {np.dtype(dtype).name} {tuple(shape)} array")
    return a


def gae(reward, value, next_value, gamma=0.99, gae_lambda=0.95, terminal=None, adv_out=None, ret_out=None):
    """(advantage, returns), float32 (K, E), of a rollout's records: reward float64 (K, E) and value float32 (K, E) as
    rollout_policy writes them, next_value float32 (E,) the value of the state after the rollout (env.act gives it
    without side effects), terminal uint8 (K, E) or None: terminal[k, e] != 0 says that step k ended env e's episode, so
    nothing is bootstrapped across k -> k + 1 (None: never; the helicopter env never ends). The recurrence and its
    rounding are gca.h's. Device tensors run ONE launch of gca_gae on the current stream (no sync, and with both
    outputs given no allocation: capturable); numpy arrays go to the host build, bit for bit the same numbers. Given
    outputs must be contiguous float32 (K, E) and live where the inputs do; they are written in place and returned."""
    if isinstance(value, np.ndarray):
        if value.ndim != 2:
            raise ValueError("gae: value must have shape (K, E)")
        return _gae_host(reward, value, next_value, gamma, gae_lambda, terminal, adv_out, ret_out)
    import torch

    if not isinstance(value, torch.Tensor) or value.dim() != 2:
        raise ValueError("gae: value must be a (K, E) float32 tensor or array")
    K, E = value.shape
    di = value.get_device()
    check_tensor(value, torch.float32, (K, E), di, "gae", "value")
    check_tensor(reward, torch.float64, (K, E), di, "gae", "reward")
    check_tensor(next_value, torch.float32, (E,), di, "gae", "next_value")
    if terminal is not None:
        check_tensor(terminal, torch.uint8, (K, E), di, "gae", "terminal")
    outs = []
    for t, what in ((adv_out, "adv_out"), (ret_out, "ret_out")):
        outs.append(torch.empty((K, E), dtype=torch.float32, device=value.device) if t is None
                    else check_tensor(t, torch.float32, (K, E), di, "gae", what))
    p = lambda t: None if t is None else t.data_ptr()
    args = (p(reward), p(value), p(next_value), p(terminal), float(gamma), gamma_lambda(gamma, gae_lambda), K, E,
            p(outs[0]), p(outs[1]))
    if di < 0:
        call_cpu("gca_gae", *args, None)
    else:
        call("gca_gae", *args, dev.raw_stream(di))
    return outs[0], outs[1]
