"""PolicyBase — what HelicopterPolicy and BulldozerPolicy share: the two-layer MLP of include/gca.h ("helicopter policy",
"bulldozer policy") over observe(radius, block)'s tensors, which differs between the agents only in the number of
outputs. The window's classes select rows of `w_local` (a Dense layer over the one-hot classes, done as a lookup), the
coarse map goes through `w_coarse`, a relu hidden layer of width `hidden`, then N_LOGITS logits and the value. Here live
the dims' checks, the seeded draw, the validated assignment of the five tensors, `version`, the C struct, load and the
trunk of forward_torch; a subclass names its heads in N_LOGITS and splits the outputs."""
import math

from .. import _device as dev
from .._lib import Policy

WEIGHTS = ("w_local", "w_coarse", "b1", "w_out", "b2")


class PolicyBase:
    N_LOGITS = None  # the subclass's: the outputs are N_LOGITS logits and the value

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

        who = type(self).__name__
        if hasattr(env_or_shape, "nrows"):
            H, W = env_or_shape.nrows, env_or_shape.ncols
            device = env_or_shape.device if device is None else device
        else:
            H, W = (int(v) for v in env_or_shape)
        self.device = torch.device("cpu") if str(device) == "cpu" else dev.require_device(device)
        radius, block, hidden = int(radius), int(block), int(hidden)
        if H < 1 or W < 1:
            raise ValueError(f"{who}: the grid shape must be positive")
        if not 0 <= radius <= 31:
            raise ValueError(f"{who}: radius must be in [0, 31]")
        if not (1 <= block <= 64 and block & (block - 1) == 0):
            raise ValueError(f"{who}: block must be a power of two in [1, 64]")
        if not (32 <= hidden <= 256 and hidden & (hidden - 1) == 0):
            raise ValueError(f"{who}: hidden must be a power of two in [32, 256]")
        self.shape, self.radius, self.block, self.hidden = (H, W), radius, block, hidden
        self.S = 2 * radius + 1
        self.Hc, self.Wc = -(-H // block), -(-W // block)
        self.C = 2 * self.Hc * self.Wc
        self.version = 0
        # a seeded draw on the scale of the reference agent's initialisation (orthogonal(sqrt 2) hidden layers, 0.01 on
        # the policy heads, a unit value head): normal entries of that standard deviation per fan-in, zero biases
        gen = torch.Generator().manual_seed(int(seed))
        n_in = self.S * self.S + self.C
        n_out = self.N_LOGITS + 1
        draw = lambda shape, std: (torch.randn(shape, generator=gen, dtype=torch.float32) * std).to(self.device)
        self.w_local = draw((self.S * self.S, 4, hidden), math.sqrt(2.0 / n_in))
        self.w_coarse = draw((self.C, hidden), math.sqrt(2.0 / n_in))
        self.b1 = torch.zeros(hidden, dtype=torch.float32, device=self.device)
        w_out = torch.randn((hidden, n_out), generator=gen, dtype=torch.float32) / math.sqrt(hidden)
        w_out[:, :self.N_LOGITS] *= 0.01
        self.w_out = w_out.to(self.device)
        self.b2 = torch.zeros(n_out, dtype=torch.float32, device=self.device)
        self._struct = Policy()
        self._sync()

    def weight_shapes(self):
        n_out = self.N_LOGITS + 1
        return {"w_local": (self.S * self.S, 4, self.hidden), "w_coarse": (self.C, self.hidden), "b1": (self.hidden,),
                "w_out": (self.hidden, n_out), "b2": (n_out,)}

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

        who = type(self).__name__
        missing = [n for n in WEIGHTS if n not in weights]
        if missing:
            raise ValueError(f"{who}.load: missing {missing}")
        new = {}
        for name in WEIGHTS:
            t = torch.as_tensor(weights[name]).detach()
            if tuple(t.shape) != self.weight_shapes()[name]:
                raise ValueError(f"{who}.load: {name} has shape {tuple(t.shape)}, "
                                 f"expected {self.weight_shapes()[name]}")
            if not t.is_floating_point():
                raise ValueError(f"{who}.load: {name} has dtype {t.dtype}, a float dtype is expected")
            new[name] = t.to(device=self.device, dtype=torch.float32).contiguous().clone()
        for name in WEIGHTS:
            object.__setattr__(self, name, new[name])
        self._sync()
        return self

    def _forward_torch(self, local, coarse, weights):
        """(out (n, N_LOGITS + 1), lead): the network's outputs in differentiable torch ops -- an embedding gather over
        the window's classes, a sum, and two matmuls -- on local (..., S, S) uint8 and coarse (..., 2, Hc, Wc) float32
        flattened to n rows, and their leading dims. The summation order is torch's, not the kernels'."""
        import torch

        w = self.state_dict() if weights is None else weights
        SS = self.S * self.S
        idx = local.reshape(-1, SS).long() & 3
        cell = torch.arange(SS, device=idx.device)
        hid = w["w_local"][cell, idx].sum(1) + coarse.reshape(-1, self.C).to(torch.float32) @ w["w_coarse"] + w["b1"]
        return torch.relu(hid) @ w["w_out"] + w["b2"], tuple(local.shape[:-2])
