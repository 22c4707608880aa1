"""The learner's side of a PPO loop on the batched envs' records (include/gca.h "PPO update"): gae(), the reference's
generalised advantage estimate (agents/jax_ppo.py:932-984) in one launch, the names of the eight statistics that
HelicopterPolicy.ppo_grad returns beside the gradients, Adam (the reference's clipped, annealed optimizer in two
launches per step, its step count on the device) and permutation (the minibatch shuffle in one launch)."""
import ctypes

import numpy as np

from .. import _device as dev
from .._lib import call, call_cpu
from ._batched import check_tensor

STATS = ("loss", "pg_loss", "v_loss", "entropy", "approx_kl", "clip_fraction", "adv_mean", "adv_std")
# ppo_grad(clip_vloss=True)'s further statistics (include/gca.h): U, the share of samples whose maximum is U, and the
# share whose value left the clip range around the recorded one
VSTATS = ("v_loss_unclipped", "u_share", "v_clip_fraction")


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


def _dev_index(device):
    return -1 if device.type == "cpu" else device.index


class Adam:
    """optax.chain(clip_by_global_norm(max_grad_norm), adam(lr, b1, b2, eps)) with the reference's linear learning-rate
    schedule (agents/jax_ppo.py:677-702, :775-783; the defaults are agents/args.py's), as gca_adam_step: two launches of
    hand-written kernels per step for all tensors together, the step count and the running b1 ** count / b2 ** count in
    a device-resident state block that the host never reads, so a step can be captured in a graph and replayed.

    params: a dict of 1 to 8 contiguous float32 tensors on one device (a cpu device runs the host build, bit for bit the
    same numbers); they are updated in place, so calls that bound their addresses stay valid. max_grad_norm <= 0: no
    clipping (the norm is still computed). anneal: None, or (steps_per_iteration, num_iterations): lr * max(1 - (count
    // steps_per_iteration) / num_iterations, 0) with the count before the step. The arithmetic and its order are
    include/gca.h's. The optimizer owns m, v, the state block and the workspace."""

    def __init__(self, params, lr=2.5e-4, b1=0.9, b2=0.999, eps=1e-5, max_grad_norm=0.5, anneal=None):
        import torch

        from .. import _lib

        if not isinstance(params, dict) or not 1 <= len(params) <= _lib.GCA_ADAM_MAX_TENSORS:
            raise ValueError(f"Adam: params must be a dict of 1 to {_lib.GCA_ADAM_MAX_TENSORS} tensors")
        first = next(iter(params.values()))
        if type(first) is not torch.Tensor:
            raise ValueError("Adam: params must hold torch tensors")
        self.device = first.device
        di = _dev_index(self.device)
        for n, t in params.items():
            if not (type(t) is torch.Tensor and t.dtype is torch.float32 and t.get_device() == di and t.is_contiguous()
                    and t.numel() >= 1):
                raise ValueError(f"Adam: params['{n}'] must be a non-empty contiguous float32 tensor on {self.device}")
        if anneal is None:
            spi, ni = 0, 0
        else:
            spi, ni = (int(x) for x in anneal)
            if spi < 1 or ni < 1:
                raise ValueError("Adam: anneal = (steps_per_iteration, num_iterations), both >= 1")
        self.params = dict(params)
        self.names = tuple(self.params)
        self.hyper = (float(lr), float(b1), float(b2), float(eps), float(max_grad_norm), spi, ni)
        self.m = {n: torch.zeros_like(t) for n, t in self.params.items()}
        self.v = {n: torch.zeros_like(t) for n, t in self.params.items()}
        self.state = torch.zeros(_lib.GCA_ADAM_STATE_WORDS, dtype=torch.int32, device=self.device)
        self.state[1:3] = 0x3F800000  # b1_pow = b2_pow = 1.0f before step 1
        self.count = self.state[0:1]  # the device-resident step count (ppo.permutation's `counter`)
        total = sum(t.numel() for t in self.params.values())
        lib = _lib.load_cpu() if di < 0 else _lib.load()
        need = lib.gca_adam_step_workspace(total)
        if need < 0:
            raise _lib.GCAError("gca_adam_step_workspace: " + lib.gca_last_error().decode(errors="replace"))
        self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        s = self._struct = _lib.AdamTensors()
        s.n = len(self.names)
        for i, n in enumerate(self.names):
            s.len[i] = self.params[n].numel()
            s.w[i], s.m[i], s.v[i] = self.params[n].data_ptr(), self.m[n].data_ptr(), self.v[n].data_ptr()
        self._grads, self._grad_tensors = None, ()
        fixed = (self._struct, self.state.data_ptr()) + self.hyper
        tail = (self.workspace.data_ptr(), self.workspace.numel())
        if di < 0:
            self._call = lambda info, stream: _lib.call_cpu("gca_adam_step", ctypes.byref(self._struct), *fixed[1:],
                                                            info, *tail, None)
        else:
            self._call = _lib.BoundCall("gca_adam_step", *fixed, _lib.SLOT, *tail, _lib.SLOT,
                                        keep=tuple(self.params.values()))

    def step(self, grads, info_out=None):
        """One step on `grads`, a dict with the names of `params` (contiguous float32 tensors of the parameters'
        shapes on their device; read only). Returns a float32 (2,) tensor: the gradients' global norm before clipping
        and the learning rate used (info_out if given, else a new tensor). No sync; with info_out no allocation."""
        import torch

        di = _dev_index(self.device)
        s = self._struct
        if grads is not self._grads or any(grads[n] is not g for n, g in zip(self.names, self._grad_tensors)):
            if not isinstance(grads, dict) or any(n not in grads for n in self.names):
                raise ValueError(f"Adam.step: grads must be a dict with the names {list(self.names)}")
            for i, n in enumerate(self.names):
                check_tensor(grads[n], torch.float32, self.params[n].shape, di, "Adam.step", f"grads['{n}']")
                s.g[i] = grads[n].data_ptr()
            self._grads, self._grad_tensors = grads, tuple(grads[n] for n in self.names)
        info = (torch.empty(2, dtype=torch.float32, device=self.device) if info_out is None
                else check_tensor(info_out, torch.float32, (2,), di, "Adam.step", "info_out"))
        self._call(info.data_ptr(), None if di < 0 else dev.raw_stream(di))
        return info

    def state_dict(self):
        """Copies of m, v and the state block (the count, b1 ** count, b2 ** count, the last norm and learning rate)."""
        return {"m": {n: t.clone() for n, t in self.m.items()}, "v": {n: t.clone() for n, t in self.v.items()},
                "state": self.state.clone()}

    def load_state_dict(self, sd):
        """Take a state_dict()'s values, in place (every bound address stays valid): training resumes with equal bits."""
        for k in ("m", "v"):
            for n in self.names:
                getattr(self, k)[n].copy_(sd[k][n])
        self.state.copy_(sd["state"])
        return self


def permutation(T, rows, seed, epoch0=0, counter=None, out=None, device=None):
    """int32 (rows, T): every row a permutation of [0, T), in ONE launch of gca_permutation (a keyed Feistel network
    walked cyclically, include/gca.h; every element computed on its own). Row r is keyed by (seed, epoch0 + r +
    counter[0]); counter: an int32 device tensor read at run time (Adam.count: a replayed graph then draws fresh rows),
    or None. out: a contiguous int32 (rows, T) tensor, else allocated on `device` (default: the counter's, else the
    current HIP device; "cpu" runs the host build, bit for bit the same rows). No sync; with `out` no allocation."""
    import torch

    T, rows = int(T), int(rows)
    if out is not None:
        device = out.device
    elif counter is not None:
        device = counter.device
    elif device is None or str(device) != "cpu":
        device = dev.require_device(device)
    device = torch.device(device)
    di = _dev_index(device)
    if out is None:
        if T < 1 or rows < 1:
            raise ValueError("permutation: T and rows must be positive")
        out = torch.empty((rows, T), dtype=torch.int32, device=device)
    else:
        check_tensor(out, torch.int32, (rows, T), di, "permutation", "out")
    if counter is not None and not (type(counter) is torch.Tensor and counter.dtype is torch.int32
                                    and counter.get_device() == di and counter.numel() >= 1):
        raise ValueError("permutation: counter must be an int32 tensor on the same device as out")
    args = (int(seed) & (2 ** 64 - 1), int(epoch0) & 0xFFFFFFFF, None if counter is None else counter.data_ptr(), T, rows,
            out.data_ptr())
    if di < 0:
        call_cpu("gca_permutation", *args, None)
    else:
        call("gca_permutation", *args, dev.raw_stream(di))
    return out
