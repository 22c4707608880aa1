"""PolicyBase — what HelicopterPolicy and BulldozerPolicy share: the two-layer MLP of include/gca.h ("helicopter policy",
"bulldozer policy") over observe(radius, block)'s tensors, which differs between the agents only in the number of
outputs. The window's classes select rows of `w_local` (a Dense layer over the one-hot classes, done as a lookup), the
coarse map goes through `w_coarse`, a relu hidden layer of width `hidden`, then N_LOGITS logits and the value. Here live
the dims' checks, the seeded draw, the validated assignment of the five tensors, `version`, the C struct, load, the
trunk of forward_torch and the learner's step: ppo_grad, the PPO loss gradient over a minibatch of rollout_policy's
records in four launches (eight with clip_vloss=True, the reference's clipped value loss), and ppo_update, the whole
update (forest_fire.ppo.permutation's shuffles, then ppo_grad and forest_fire.ppo.Adam.step per minibatch). A subclass names its heads (HEADS, N_LOGITS), its gradient entry point
(GRAD_ENTRY) and splits the outputs."""
import ctypes
import math

from .. import _device as dev
from .. import _lib
from .._lib import SLOT, BoundCall, Policy

WEIGHTS = ("w_local", "w_coarse", "b1", "w_out", "b2")


class PolicyBase:
    HEADS = None       # the subclass's: the logits of each head; a record's `action` holds len(HEADS) values per row
    N_LOGITS = None    # sum(HEADS): the outputs are N_LOGITS logits and the value; the width of a record's `logits`
    GRAD_ENTRY = None  # its gca_*_policy_grad entry point (the workspace query is GRAD_ENTRY + "_workspace")

    def __setattr__(self, name, value):
        d = self.__dict__
        if name in WEIGHTS and "_struct" in d:
            value = self._checked(name, value)
            object.__setattr__(self, name, value)
            self._sync()
            return
        object.__setattr__(self, name, value)

    def _coarse_len(self):
        """C, the floats of the network's coarse part: the coarse map's 2 Hc Wc (a subclass may widen it)."""
        return 2 * self.Hc * self.Wc

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
        self.C = self._coarse_len()
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

    # ------------------------------------------------------------------ the learner's step
    def _ppo_workspace(self, N, workspace):
        """The workspace of a minibatch of N samples: the caller's (uint8, at least the size the library asks for), or
        the policy's own. The policy keeps ONE buffer, replaced by a larger one when a call needs more (the size grows
        with N and depends on (S, C, hidden, N) only, not on the weights), so it never holds more than the largest
        minibatch needs. Calls that may overlap (two streams) or that a captured graph replays while eager calls of a
        larger N go on must pass a workspace of their own."""
        import torch

        lib = _lib.load_cpu() if self.device.type == "cpu" else _lib.load()
        need = getattr(lib, self.GRAD_ENTRY + "_workspace")(ctypes.byref(self._struct), self.C, N)
        if need < 0:
            raise _lib.GCAError(f"{self.GRAD_ENTRY}_workspace: " + lib.gca_last_error().decode(errors="replace"))
        if workspace is not None:
            if not (type(workspace) is torch.Tensor and workspace.dtype is torch.uint8 and workspace.is_contiguous()
                    and workspace.device == self.device and workspace.numel() >= need):
                raise ValueError(f"ppo_grad: workspace must be a contiguous uint8 tensor of at least {need} bytes on "
                                 f"{self.device}")
            return workspace
        ws = self.__dict__.get("_ppo_ws")
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            object.__setattr__(self, "_ppo_ws", ws)
        return ws

    def ppo_grad(self, records, advantage, returns, idx=None, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, norm_adv=True,
                 grads_out=None, stats_out=None, workspace=None, clip_vloss=False, vstats_out=None):
        """(grads, stats) of the PPO clipped-surrogate loss (agents/jax_ppo.py:987-1041; per head, as
        include/gca.h states it: with one head the usual loss, with the bulldozer's two every mean runs over the
        (sample, head) pairs) over a minibatch of rollout_policy's records, in four launches of hand-written kernels
        (gca_helicopter_policy_grad / gca_bulldozer_policy_grad).
        clip_vloss: False (the default) takes the value loss 0.5 (v - R)^2; True the reference's clipped value loss
        (its own default, args.ppo.clip_vloss: the batch mean of the unclipped loss BEFORE the maximum, include/gca.h),
        in eight launches (gca_*_policy_grad_vclip). It needs records['value'], the recorded values (contiguous float32,
        T values), which is not looked at otherwise, and returns (grads, stats, vstats): vstats float32 (3,) in the
        order of forest_fire.ppo.VSTATS, in vstats_out if given. stats' v_loss and loss are then the clipped ones.
        records: rollout_policy's dict -- `local`, `coarse`, `action`, `logits` are read -- in (K, E, ...) or
        flattened (T, ...) form, `action` with len(HEADS) and `logits` with N_LOGITS values per row;
        advantage / returns: forest_fire.ppo.gae's float32 outputs, T values each. idx: an
        int32 tensor of N rows in [0, T) (repeats allowed; a device randperm slice), None: all T rows in order. Nothing
        is gathered into a copy. grads: a dict of the five WEIGHTS names with weight_shapes(), d loss / d tensor, every
        element written; stats: float32 (8,) in the order of forest_fire.ppo.STATS. grads_out / stats_out: the caller's
        tensors (contiguous float32 of those shapes on the policy's device, distinct from the weights), else allocated;
        workspace: a uint8 tensor, else the policy's own (_ppo_workspace: one buffer, grown to the largest N seen). All
        sums run in a fixed order: equal inputs give equal bits. No sync, and with the outputs given and the workspace
        given or already large enough no allocation: capturable.
        The policy's tensors may be updated in place between calls (`w.add_(g, alpha=-lr)`): an in-place update keeps
        the addresses, so nothing is bound again; assigning a new tensor moves `version` and the next call binds it."""
        import torch

        from ._batched import _is_kernel_tensor, check_tensor

        di = -1 if self.device.type == "cpu" else self.device.index
        clip_vloss = bool(clip_vloss)
        if vstats_out is not None and not clip_vloss:
            raise ValueError("ppo_grad: vstats_out needs clip_vloss=True")
        wanted = ("local", "coarse", "action", "logits") + (("value",) if clip_vloss else ())
        missing = [n for n in wanted if n not in records]
        if missing:
            raise ValueError(f"ppo_grad: records lack {missing}")
        action = records["action"]
        if not _is_kernel_tensor(action, torch.int32, di) or action.numel() < len(self.HEADS):
            raise ValueError("ppo_grad: records['action'] must be a contiguous int32 tensor on the policy's device")
        NH = len(self.HEADS)
        T = action.numel() // NH
        rec = []
        for t, dtype, per, what in ((records["local"], torch.uint8, self.S * self.S, "records['local']"),
                                    (records["coarse"], torch.float32, self.C, "records['coarse']"),
                                    (action, torch.int32, NH, "records['action']"),
                                    (records["logits"], torch.float32, self.N_LOGITS, "records['logits']"),
                                    *(((records["value"], torch.float32, 1, "records['value']"),) if clip_vloss else ()),
                                    (advantage, torch.float32, 1, "advantage"), (returns, torch.float32, 1, "returns")):
            if not (_is_kernel_tensor(t, dtype, di) and t.numel() == T * per):
                raise ValueError(f"ppo_grad: {what} must be a contiguous {str(dtype).replace('torch.', '')} tensor of "
                                 f"{T} x {per} values on the policy's device")
            rec.append(t)
        if idx is None:
            N = T
        else:
            if not (_is_kernel_tensor(idx, torch.int32, di) and idx.dim() == 1 and idx.numel() >= 1):
                raise ValueError("ppo_grad: idx must be a contiguous int32 (N,) tensor on the policy's device")
            N = idx.numel()
        shapes = self.weight_shapes()
        if grads_out is None:
            grads = {n: torch.empty(shapes[n], dtype=torch.float32, device=self.device) for n in WEIGHTS}
        else:
            grads = {n: check_tensor(grads_out.get(n), torch.float32, shapes[n], di, "ppo_grad", f"grads_out['{n}']")
                     for n in WEIGHTS}
        stats = (torch.empty(8, dtype=torch.float32, device=self.device) if stats_out is None
                 else check_tensor(stats_out, torch.float32, (8,), di, "ppo_grad", "stats_out"))
        ws = self._ppo_workspace(N, workspace)
        args = [t.data_ptr() for t in rec] + [T, None if idx is None else idx.data_ptr(), N, float(clip_coef),
                                              float(ent_coef), float(vf_coef), 1 if norm_adv else 0]
        args += [grads[n].data_ptr() for n in WEIGHTS] + [stats.data_ptr()]
        if clip_vloss:
            vstats = (torch.empty(3, dtype=torch.float32, device=self.device) if vstats_out is None
                      else check_tensor(vstats_out, torch.float32, (3,), di, "ppo_grad", "vstats_out"))
            args += [vstats.data_ptr(), ws.data_ptr(), ws.numel()]
            if di < 0:
                _lib.call_cpu(self.GRAD_ENTRY + "_vclip", ctypes.byref(self._struct), self.C, *args, None)
                return grads, stats, vstats
            pc = self.__dict__.get("_ppo_vclip_call")
            if pc is None or pc[0] != self.version:
                pc = (self.version, BoundCall(self.GRAD_ENTRY + "_vclip", self._struct, self.C, *([SLOT] * 24),
                                              keep=self.tensors()))
                object.__setattr__(self, "_ppo_vclip_call", pc)
            pc[1](*args, dev.raw_stream(di))
            return grads, stats, vstats
        args += [ws.data_ptr(), ws.numel()]
        if di < 0:
            _lib.call_cpu(self.GRAD_ENTRY, ctypes.byref(self._struct), self.C, *args, None)
            return grads, stats
        pc = self.__dict__.get("_ppo_call")
        if pc is None or pc[0] != self.version:
            # everything but the policy is a per-call slot: the records, the minibatch and the outputs are the caller's
            pc = (self.version, BoundCall(self.GRAD_ENTRY, self._struct, self.C, *([SLOT] * 22),
                                          keep=self.tensors()))
            object.__setattr__(self, "_ppo_call", pc)
        pc[1](*args, dev.raw_stream(di))
        return grads, stats

    def ppo_update(self, opt, records, advantage, returns, epochs=4, minibatches=4, seed=0, clip_coef=0.2,
                   ent_coef=0.01, vf_coef=0.5, norm_adv=True, stats_out=None, info_out=None, perm_out=None,
                   grads_out=None, workspace=None, clip_vloss=False, vstats_out=None):
        """A whole PPO update on the device (the reference's update_ppo, agents/jax_ppo.py:1045-1114): ONE
        forest_fire.ppo.permutation launch draws the `epochs` shuffles of the T recorded samples (keyed by seed, the
        epoch and opt.count, the optimizer's device-resident step count), then every epoch walks its row in
        `minibatches` slices of T / minibatches rows: ppo_grad on the slice, opt.step on the gradients. opt: a
        forest_fire.ppo.Adam over exactly this policy's five tensors. Returns (stats (epochs * minibatches, 8), info
        (epochs * minibatches, 2)): row i holds the i-th minibatch's ppo_grad statistics and Adam.step's (pre-clip
        gradient norm, learning rate). stats_out / info_out / perm_out (int32 (epochs, T)) / grads_out / workspace: the
        caller's buffers, else allocated (the workspace: the policy's own). With all of them given the call allocates
        nothing and does not sync: it can be captured as one graph, and a replay draws new shuffles because opt.count has
        moved. clip_vloss=True: ppo_grad's clipped value loss on records['value']; returns (stats, info, vstats), vstats
        (epochs * minibatches, 3) in the order of forest_fire.ppo.VSTATS, in vstats_out if given."""
        import torch

        from . import ppo
        from ._batched import check_tensor

        di = -1 if self.device.type == "cpu" else self.device.index
        epochs, minibatches = int(epochs), int(minibatches)
        if epochs < 1 or minibatches < 1:
            raise ValueError("ppo_update: epochs and minibatches must be positive")
        if not isinstance(opt, ppo.Adam) or set(opt.names) != set(WEIGHTS):
            raise ValueError(f"ppo_update: opt must be a forest_fire.ppo.Adam over the policy's tensors {list(WEIGHTS)}")
        for n in WEIGHTS:
            if opt.params[n] is not getattr(self, n):
                raise ValueError(f"ppo_update: opt.params['{n}'] is not policy.{n} (a tensor was reassigned after the "
                                 "optimizer was built)")
        action = records.get("action") if isinstance(records, dict) else None
        if type(action) is not torch.Tensor or action.numel() < len(self.HEADS):
            raise ValueError("ppo_update: records['action'] must be a tensor")
        T = action.numel() // len(self.HEADS)
        if T % minibatches:
            raise ValueError(f"ppo_update: T = {T} samples do not divide into {minibatches} minibatches")
        N, steps = T // minibatches, epochs * minibatches
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.device)
        stats = (new((steps, 8), torch.float32) if stats_out is None
                 else check_tensor(stats_out, torch.float32, (steps, 8), di, "ppo_update", "stats_out"))
        info = (new((steps, 2), torch.float32) if info_out is None
                else check_tensor(info_out, torch.float32, (steps, 2), di, "ppo_update", "info_out"))
        perm = (new((epochs, T), torch.int32) if perm_out is None
                else check_tensor(perm_out, torch.int32, (epochs, T), di, "ppo_update", "perm_out"))
        grads = ({n: new(s, torch.float32) for n, s in self.weight_shapes().items()} if grads_out is None
                 else grads_out)
        clip_vloss = bool(clip_vloss)
        if vstats_out is not None and not clip_vloss:
            raise ValueError("ppo_update: vstats_out needs clip_vloss=True")
        vstats = None
        if clip_vloss:
            vstats = (new((steps, 3), torch.float32) if vstats_out is None
                      else check_tensor(vstats_out, torch.float32, (steps, 3), di, "ppo_update", "vstats_out"))
        ppo.permutation(T, epochs, seed, counter=opt.count, out=perm)
        for e in range(epochs):
            for mb in range(minibatches):
                i = e * minibatches + mb
                self.ppo_grad(records, advantage, returns, perm[e, mb * N:(mb + 1) * N], clip_coef=clip_coef,
                              ent_coef=ent_coef, vf_coef=vf_coef, norm_adv=norm_adv, grads_out=grads,
                              stats_out=stats[i], workspace=workspace, clip_vloss=clip_vloss,
                              vstats_out=vstats[i] if clip_vloss else None)
                opt.step(grads, info_out=info[i])
        return (stats, info, vstats) if clip_vloss else (stats, info)
