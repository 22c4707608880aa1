"""BulldozerPolicy — the two-headed policy network the batched bulldozer env evaluates inside its own launches.

The helicopter policy's two-layer MLP over observe(radius, block)'s tensors (include/gca.h "bulldozer policy") with twelve
outputs: nine move logits, two shoot logits (the reference's Actor(action_dims=[9, 2])) and the value. env.act(policy)
is one launch on an observation; env.rollout_policy(policy, K) collects K closed-loop steps of every env, autoreset
included, bit for bit K x (observe, act, step [, reset]) and in one launch where the shape allows. forward_torch is the
same network in differentiable torch ops, for a learner that takes the loss through autograd
(scripts/train_bulldozer_ppo.py); the two-head loss gradient on the device is not part of this class yet.

The bookkeeping (validated assignment of the five tensors, `version`, the C struct, load) is HelicopterPolicy's, written
out here so that class stays as it is.
"""
import math

from ... import _device as dev
from ..._lib import BulldozerPolicyStruct

WEIGHTS = ("w_local", "w_coarse", "b1", "w_out", "b2")
N_MOVE = 9
N_SHOOT = 2
N_LOGITS = N_MOVE + N_SHOOT
N_OUT = N_LOGITS + 1  # the logits and the value


class BulldozerPolicy:
    def __setattr__(self, name, value):
        d = self.__dict__
        if name in WEIGHTS and "_struct" in d:
            value = self._checked(name, value)
            object.__setattr__(self, name, value)
            self._sync()
            return
        object.__setattr__(self, name, value)

    def __init__(self, env_or_shape, radius=5, block=8, hidden=64, seed=0, device=None):
        import torch

        if hasattr(env_or_shape, "nrows"):
            H, W = env_or_shape.nrows, env_or_shape.ncols
            device = env_or_shape.device if device is None else device
        else:
            H, W = (int(v) for v in env_or_shape)
        self.device = torch.device("cpu") if str(device) == "cpu" else dev.require_device(device)
        radius, block, hidden = int(radius), int(block), int(hidden)
        if H < 1 or W < 1:
            raise ValueError("BulldozerPolicy: the grid shape must be positive")
        if not 0 <= radius <= 31:
            raise ValueError("BulldozerPolicy: radius must be in [0, 31]")
        if not (1 <= block <= 64 and block & (block - 1) == 0):
            raise ValueError("BulldozerPolicy: block must be a power of two in [1, 64]")
        if not (32 <= hidden <= 256 and hidden & (hidden - 1) == 0):
            raise ValueError("BulldozerPolicy: hidden must be a power of two in [32, 256]")
        self.shape, self.radius, self.block, self.hidden = (H, W), radius, block, hidden
        self.S = 2 * radius + 1
        self.Hc, self.Wc = -(-H // block), -(-W // block)
        self.C = 2 * self.Hc * self.Wc
        self.version = 0
        # a seeded draw on the scale of the reference agent's initialisation (orthogonal(sqrt 2) hidden layers, 0.01 on
        # both policy heads, a unit value head): normal entries of that standard deviation per fan-in, zero biases
        gen = torch.Generator().manual_seed(int(seed))
        n_in = self.S * self.S + self.C
        draw = lambda shape, std: (torch.randn(shape, generator=gen, dtype=torch.float32) * std).to(self.device)
        self.w_local = draw((self.S * self.S, 4, hidden), math.sqrt(2.0 / n_in))
        self.w_coarse = draw((self.C, hidden), math.sqrt(2.0 / n_in))
        self.b1 = torch.zeros(hidden, dtype=torch.float32, device=self.device)
        w_out = torch.randn((hidden, N_OUT), generator=gen, dtype=torch.float32) / math.sqrt(hidden)
        w_out[:, :N_LOGITS] *= 0.01
        self.w_out = w_out.to(self.device)
        self.b2 = torch.zeros(N_OUT, dtype=torch.float32, device=self.device)
        self._struct = BulldozerPolicyStruct()
        self._sync()

    def weight_shapes(self):
        return {"w_local": (self.S * self.S, 4, self.hidden), "w_coarse": (self.C, self.hidden), "b1": (self.hidden,),
                "w_out": (self.hidden, N_OUT), "b2": (N_OUT,)}

    def _checked(self, name, t):
        import torch

        shape = self.weight_shapes()[name]
        if not (type(t) is torch.Tensor and t.dtype is torch.float32 and tuple(t.shape) == shape
                and t.device == self.device and t.is_contiguous()):
            raise ValueError(f"policy.{name}: a contiguous float32 {shape} tensor on {self.device} is required")
        return t.detach()

    def _sync(self):
        """The C struct follows the tensors; `version` tells the envs' pre-bound calls (which keep the tensors they
        bound alive) that they are stale."""
        s = self._struct
        s.radius, s.block, s.hidden, s.reserved = self.radius, self.block, self.hidden, 0
        for name in WEIGHTS:
            setattr(s, name, getattr(self, name).data_ptr())
        self.version += 1

    @property
    def struct(self):
        return self._struct

    def tensors(self):
        return tuple(getattr(self, name) for name in WEIGHTS)

    def state_dict(self):
        return {name: getattr(self, name) for name in WEIGHTS}

    def load(self, weights):
        """Take a trainer's weights: a dict with the five names (tensors or arrays of the shapes of weight_shapes(),
        any float dtype, any device); they are copied into new float32 tensors on the policy's device."""
        import torch

        missing = [n for n in WEIGHTS if n not in weights]
        if missing:
            raise ValueError(f"BulldozerPolicy.load: missing {missing}")
        new = {}
        for name in WEIGHTS:
            t = torch.as_tensor(weights[name]).detach()
            if tuple(t.shape) != self.weight_shapes()[name]:
                raise ValueError(f"BulldozerPolicy.load: {name} has shape {tuple(t.shape)}, "
                                 f"expected {self.weight_shapes()[name]}")
            if not t.is_floating_point():
                raise ValueError(f"BulldozerPolicy.load: {name} has dtype {t.dtype}, a float dtype is expected")
            new[name] = t.to(device=self.device, dtype=torch.float32).contiguous().clone()
        for name in WEIGHTS:
            object.__setattr__(self, name, new[name])
        self._sync()
        return self

    def forward_torch(self, local, coarse, weights=None):
        """(move_logits (..., 9), shoot_logits (..., 2), value (...)) of the same network in differentiable torch ops: an
        embedding gather over the window's classes, a sum, and two matmuls. local (..., S, S) uint8, coarse
        (..., 2, Hc, Wc) float32 with the same leading dims (for instance the (K, E) of rollout_policy's records).
        weights: a dict of the five tensors to use instead of the policy's own (a trainer's leaf tensors, which then
        receive the gradients). The summation order is torch's, not the kernels': the results agree within rounding, not
        bit for bit."""
        import torch

        w = self.state_dict() if weights is None else weights
        SS = self.S * self.S
        lead = tuple(local.shape[:-2])
        idx = local.reshape(-1, SS).long() & 3
        cell = torch.arange(SS, device=idx.device)
        hid = w["w_local"][cell, idx].sum(1) + coarse.reshape(-1, self.C).to(torch.float32) @ w["w_coarse"] + w["b1"]
        out = torch.relu(hid) @ w["w_out"] + w["b2"]
        return (out[:, :N_MOVE].reshape(lead + (N_MOVE,)), out[:, N_MOVE:N_LOGITS].reshape(lead + (N_SHOOT,)),
                out[:, N_LOGITS].reshape(lead))
