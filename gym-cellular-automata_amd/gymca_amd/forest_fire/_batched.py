"""What the batched envs (bulldozer/batched.py, helicopter/batched.py) and policy_obs share: the one test of a tensor
the kernels may address as it is, the action intake of rollout(), and the base class of the env classes."""
import numpy as np

from .. import _device as dev


def seed64(x):
    """x as the uint64 the C ABI takes for a seed (negative and oversized ints wrap)."""
    return int(x) & (2**64 - 1)


def _is_kernel_tensor(t, dtype, dev_index):
    """True where a kernel may address `t` through data_ptr() as it is: a torch.Tensor proper (no subclass) of `dtype`,
    contiguous, on the device of index `dev_index` (-1: the host). BatchedEnvBase._action writes the same test out."""
    import torch

    return type(t) is torch.Tensor and t.dtype is dtype and t.get_device() == dev_index and t.is_contiguous()


def check_tensor(t, dtype, shape, dev_index, who, what):
    """`t` if it is such a tensor (_is_kernel_tensor) of `shape`, else ValueError."""
    if not (_is_kernel_tensor(t, dtype, dev_index) and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{who}: {what} must be a contiguous {str(dtype).replace('torch.', '')} {tuple(shape)} tensor "
                         "on the env's device")
    return t


def rollout_actions(actions, K, E, tail, device, dev_index, who, convert_host_tensor):
    """The `actions` / `K` pair of a rollout() as (int32 (K, E) + tail tensor on `device` or None, K). `tail` is one
    env's action shape: () for the helicopter, (2,) for the bulldozer. A contiguous int32 tensor on the env's device is
    used as it is, any other integer array is converted; actions=None (the random policy) needs K.
    convert_host_tensor: the one point where the envs differ. True (helicopter): a torch.Tensor in host memory is
    converted like a numpy array. False (bulldozer): it is refused, as a tensor on another device is."""
    import torch

    a = actions
    if a is None:
        if K is None:
            raise ValueError(f"{who}: K is needed with actions=None")
        K = int(K)
    else:
        if _is_kernel_tensor(a, torch.int32, dev_index):
            pass  # the caller's own tensor, no torch call; its shape is checked below (K is not known yet)
        elif isinstance(a, torch.Tensor) and (a.is_cuda or dev_index < 0 or not convert_host_tensor):
            # every tensor but the one the keyword speaks of: in host memory while the env lives on a GPU
            if a.is_floating_point() or a.dtype is torch.bool:
                raise ValueError(f"{who}: actions must be integers")
            if a.get_device() != dev_index:
                raise ValueError(f"{who}: actions live on {a.device}, the env on {device}")
            a = a.to(torch.int32).contiguous()
        else:
            h = np.asarray(a)
            if h.dtype.kind not in "iu":
                raise ValueError(f"{who}: actions must be integers")
            a = dev.to_device(h.astype(np.int32), torch.int32, device)
        if tuple(a.shape[1:]) != (E,) + tuple(tail):
            want = ", ".join(map(str, ("K", E) + tuple(tail)))
            raise ValueError(f"{who}: actions must have shape ({want}), got {tuple(a.shape)}")
        if K is not None and int(K) != a.shape[0]:
            raise ValueError(f"{who}: K = {K} disagrees with actions of shape {tuple(a.shape)}")
        K = int(a.shape[0])
    if K < 0:
        raise ValueError(f"{who}: K >= 0")
    return a, K


class BatchedEnvBase:
    """E envs resident in HBM, their state tensors bound by address into pre-bound calls. A subclass names the bound
    state in `_BOUND_STATE` and the attribute whose presence says that __init__ got as far as the bound calls in
    `_BOUND_READY`, and provides rebind(), `_act_buf` / `_act_shape`, `_ctx`, buf / parity / pos and the three cell
    codes."""

    _BOUND_STATE = frozenset()
    _BOUND_READY = None

    def __setattr__(self, name, value):
        # assigning a bound state tensor validates the replacement and drops the bound calls (rebind), so the next step
        # binds the new tensor
        d = self.__dict__
        if name in self._BOUND_STATE and self._BOUND_READY in d and d.get(name) is not value:
            self._check_replacement(name, d.get(name), value)
            object.__setattr__(self, name, value)
            self.rebind()
            return
        object.__setattr__(self, name, value)

    def _check_replacement(self, name, old, value):
        """Raise unless `value` may take the place of the bound `old`; a subclass overrides it for state that is no
        tensor."""
        if not (dev.is_device_tensor(value) and value.dtype == old.dtype and value.shape == old.shape
                and value.device == old.device and value.is_contiguous()):
            raise ValueError(f"env.{name}: the replacement must be a contiguous {old.dtype} tensor of shape "
                             f"{tuple(old.shape)} on {old.device} (or update the tensor in place)")

    def grids(self):
        """(E, H, W) uint8: every env's current grid (one gather pass)."""
        import torch

        return torch.where(self.parity.bool()[:, None, None], self.buf[1], self.buf[0])

    def _obs(self):
        return (self.grids() if self.materialize_obs else None), self._ctx

    def observe(self, radius=16, block=16, local_out=None, coarse_out=None, form=0):
        """The policy observation of every env in one launch (gca_policy_observation, policy_obs.observe): `local`, uint8
        (E, 2 radius + 1, 2 radius + 1), the classes of the cells around the agent (0 other, 1 TREE, 2 FIRE, 3 outside
        the grid), and `coarse`, float32 (E, 2, ceil(H / block), ceil(W / block)), the TREE and the FIRE share of every
        block x block tile. Reads each env's current plane once: no grids() gather, no sync, and with both outputs given
        (contiguous tensors of that dtype and shape on the env's device, written in place and returned) no allocation.
        radius in [0, 31], block a power of two in [1, 64]; form 0 picks the kernel by shape."""
        from . import policy_obs

        return policy_obs.observe(self, radius, block, local_out, coarse_out, form)

    def _action(self, action):
        """action as a contiguous int32 device tensor of `_act_shape`: the caller's own tensor when it is one (checked
        on every call: a tensor retyped or reshaped in place since the last step is converted, not misread), else
        converted into the env's action buffer. _is_kernel_tensor written out, because every eager step runs it."""
        import torch

        if (type(action) is torch.Tensor and action.dtype is torch.int32 and action.get_device() == self._dev_index
                and action.shape == self._act_shape and action.is_contiguous()):
            return action
        src = action if dev.is_device_tensor(action) else torch.as_tensor(np.asarray(action))
        self._act_buf.copy_(src.reshape(self._act_shape))
        return self._act_buf

    def _out(self, t, dtype, shape, who, what):
        """The output tensor `what` of `who`: allocated here, or the caller's own after check_tensor."""
        import torch

        if t is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        return check_tensor(t, dtype, shape, self._dev_index, who, what)

    # ------------------------------------------------------------------ the policy inside the env's launches
    # A subclass names its policy class in `_POLICY_CLASS` and its records in `_POLICY_RECORDS` / _policy_spec(), and
    # keeps the dict `_policy_calls`, emptied by rebind().
    _POLICY_CLASS = None
    _POLICY_RECORDS = ()
    _POLICY_CALLS_MAX = 8

    def _check_policy(self, policy, who):
        if not isinstance(policy, self._POLICY_CLASS):
            raise ValueError(f"{who}: policy must be a {self._POLICY_CLASS.__name__}")
        if len(policy.HEADS) != len(self._POLICY_CLASS.HEADS):
            raise ValueError(f"{who}: a {type(policy).__name__} has {len(policy.HEADS)} heads; this env takes a "
                             f"{self._POLICY_CLASS.__name__} (the extension head belongs to "
                             "AdvancedForestFireBulldozerEnv(enable_extensions=True))")
        if getattr(policy, "retardant", False):
            raise ValueError(f"{who}: the policy was built with retardant=True, and this env has no retardant layer to "
                             "observe (only AdvancedForestFireBulldozerEnv keeps one)")
        if policy.shape != (self.nrows, self.ncols):
            raise ValueError(f"{who}: the policy was built for a {policy.shape} grid, the env is "
                             f"{(self.nrows, self.ncols)}")
        if policy.device != self.device:
            raise ValueError(f"{who}: the policy lives on {policy.device}, the env on {self.device}")
        return policy

    def _policy_call(self, kind, policy, make):
        """The pre-bound call of `kind` for this policy; bound again when a policy tensor was replaced (its version
        moved) or the env rebound. The entry keeps the policy, its tensors of that version and the call's scratch alive,
        so the cache is bounded: beyond _POLICY_CALLS_MAX entries the one bound longest ago is dropped (a trainer that
        builds policy after policy against one env does not keep them all; a dropped policy is simply bound again). A
        graph captured from a call replays that entry's addresses: whoever holds such a graph keeps the number of
        policies in use on this env within the bound, or captures again."""
        key = (kind, id(policy))
        calls = self._policy_calls
        pc = calls.get(key)
        if pc is None or pc[0] != policy.version or pc[1] is not policy:
            calls.pop(key, None)
            while len(calls) >= self._POLICY_CALLS_MAX:
                del calls[next(iter(calls))]
            pc = (policy.version, policy) + tuple(make())
        else:
            del calls[key]  # least recently used first: a hit moves the entry to the end
        calls[key] = pc
        return pc

    def _act_inputs(self, policy, local, coarse, action_shape, n_logits, action_out, logits_out, value_out):
        """act()'s checks up to its launch: (policy, local, coarse, action_out, logits_out, value_out), the observation
        taken here unless both `local` and `coarse` are given, the three outputs the caller's or allocated."""
        import torch

        from . import policy_obs

        policy = self._check_policy(policy, "act")
        E = self.num_envs
        ls, cs = policy_obs.output_shapes(self, policy.radius, policy.block)
        if (local is None) != (coarse is None):
            raise ValueError("act: give both local and coarse, or neither")
        if local is None:
            local, coarse = self.observe(policy.radius, policy.block)
        else:
            check_tensor(local, torch.uint8, ls, self._dev_index, "act", "local")
            check_tensor(coarse, torch.float32, cs, self._dev_index, "act", "coarse")
        action_out = self._out(action_out, torch.int32, action_shape, "act", "action_out")
        logits_out = self._out(logits_out, torch.float32, (E, n_logits), "act", "logits_out")
        value_out = self._out(value_out, torch.float32, (E,), "act", "value_out")
        return policy, local, coarse, action_out, logits_out, value_out

    def _policy_records(self, policy, K, record, given):
        """rollout_policy()'s checks up to its launch: (policy, K, recs), recs the dict of the records named in
        `record` and of every record whose output tensor is `given`, the caller's or allocated. _policy_spec(K, ls, cs)
        is the subclass's table of each record's (dtype, shape)."""
        from . import policy_obs

        policy = self._check_policy(policy, "rollout_policy")
        K = int(K)
        if K < 0:
            raise ValueError("rollout_policy: K >= 0")
        spec = self._policy_spec(K, *policy_obs.output_shapes(self, policy.radius, policy.block))
        unknown = [r for r in record if r not in spec]
        if unknown:
            raise ValueError(f"rollout_policy: unknown records {unknown}; choose from {self._POLICY_RECORDS}")
        recs = {}
        for name in self._POLICY_RECORDS:
            dtype, shape = spec[name]
            if given[name] is not None or name in record:
                recs[name] = self._out(given[name], dtype, shape, "rollout_policy", f"{name}_out")
        return policy, K, recs

    def _check_positions(self, positions):
        """positions as an int32 (E, 2) array of cells inside the grid, else ValueError."""
        E, H, W = self.num_envs, self.nrows, self.ncols
        pos = np.asarray(positions).reshape(E, 2)
        if not ((pos[:, 0] >= 0) & (pos[:, 0] < H) & (pos[:, 1] >= 0) & (pos[:, 1] < W)).all():
            raise ValueError(f"every position must lie inside the {H}x{W} grid")
        return pos.astype(np.int32)
