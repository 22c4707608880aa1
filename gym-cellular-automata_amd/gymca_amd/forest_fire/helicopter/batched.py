"""BatchedForestFireHelicopterEnv — E ForestFireHelicopter envs resident in HBM, one launch per env step.

The batched form of helicopter.py's MDP (reference helicopter.py:220-236 + ca_env.py:27-48). gca_helicopter_step
does the whole step of every env: the action (the caller's, or drawn inside the step), Move, the Drossel–Schwabl CA
when the env's freeze countdown is 0, Modify {FIRE: EMPTY} at the moved position, freeze, cell counts and reward.
rollout(actions) runs K such steps in one launch (gca_helicopter_rollout: the env's grid stays in LDS between steps);
rollout_policy(policy, K) closes the loop inside that launch: a HelicopterPolicy (policy.py) picks every step's action
from that step's observation (gca_helicopter_policy_rollout), and act(policy) is the same network as one launch.

Grids live in two buffers; env e's current grid is buf[parity[e]][e], so an env whose countdown is still running
moves no bytes beyond the one cell Modify may patch. The CA's draws are Philox keyed by (cell, global env id,
rng_step) -- the Philox mode of gca_ds_step, bit for bit -- so a sharded env (env_offset) reproduces the unsharded one
env for env. Replaying numpy's stream cell for cell stays the single-env ForestFireHelicopterEnv's role.
"""
import numpy as np

from ... import _device as dev
from ..._lib import SLOT, BoundCall, call
from .._batched import BatchedEnvBase, check_tensor, rollout_actions, seed64
from ..operators.ca_DrosselSchwabl import choice_threshold
from .policy import HelicopterPolicy


class BatchedForestFireHelicopterEnv(BatchedEnvBase):
    # state the pre-bound calls hold by address (step, step_random, sample_actions): assigning one of these attributes
    # validates the replacement and drops the bound calls (BatchedEnvBase.__setattr__)
    _BOUND_STATE = frozenset({"buf", "parity", "freeze", "pos", "counts", "rng_step", "hit", "reward", "steps_elapsed",
                              "thresholds", "_meet", "_act_buf", "_act2"})
    _BOUND_READY = "_step_call"
    _POLICY_CLASS = HelicopterPolicy

    def __init__(self, num_envs, nrows, ncols, device=None, seed=0, env_offset=0, speed=0.5, freeze=None,
                 p_fire=0.033, p_tree=0.333, materialize_obs=True):
        import torch

        self.device = dev.require_device(device)
        self.num_envs, self.nrows, self.ncols = E, H, W = int(num_envs), int(nrows), int(ncols)
        if E < 1 or H < 1 or W < 1 or H * W >= 2**30:
            raise ValueError("num_envs, nrows, ncols >= 1 and nrows * ncols < 2**30")
        self.seed_value = int(seed)
        self.env_offset = int(env_offset)
        self.materialize_obs = materialize_obs
        self._empty, self._tree, self._fire = 0, 1, 2
        self._p_fire, self._p_tree = float(p_fire), float(p_tree)
        self.max_freeze = int(speed * ((H + W) // 2)) if freeze is None else int(freeze)
        if self.max_freeze < 0:
            raise ValueError("freeze >= 0")
        kw = dict(device=self.device)
        self.buf = torch.zeros((2, E, H, W), dtype=torch.uint8, **kw)
        self.parity = torch.zeros(E, dtype=torch.uint8, **kw)
        self.freeze = torch.full((E,), self.max_freeze, dtype=torch.int32, **kw)
        self.pos = torch.zeros((E, 2), dtype=torch.int32, **kw)
        self.counts = torch.zeros((E, 3), dtype=torch.int32, **kw)
        self.rng_step = torch.zeros(E, dtype=torch.int32, **kw)  # uint32 bits
        self.hit = torch.zeros(E, dtype=torch.uint8, **kw)
        self.reward = torch.zeros(E, dtype=torch.float64, **kw)
        self.steps_elapsed = torch.zeros(E, dtype=torch.int64, **kw)
        # cdf[0] of numpy's choice([True, False], p=[p, 1 - p]) per env: what gca_ds_step takes
        thr = np.array([choice_threshold(self._p_fire), choice_threshold(self._p_tree)], dtype=np.float64)
        self.thresholds = dev.to_device(np.broadcast_to(thr, (E, 2)), torch.float64, self.device)
        self.ca_params = dev.to_device(np.broadcast_to(np.array([self._p_fire, self._p_tree]), (E, 2)), torch.float64,
                                       self.device)
        # the step's per-env meeting slots (gca_helicopter_step: several workgroups per env at small E), kept zero
        self._meet = torch.zeros(E, dtype=torch.int64, **kw)
        self._terminated = torch.zeros(E, dtype=torch.bool, **kw)
        self._truncated = torch.zeros(E, dtype=torch.bool, **kw)
        self._dev_index = dev.device_index(self.device)
        self._act_buf = torch.zeros(E, dtype=torch.int32, **kw)
        self._act2 = torch.zeros((E, 2), dtype=torch.int32, **kw)  # gca_random_actions draws (move, shoot) pairs
        self._act_shape = self._act_buf.shape
        self._step_call = None
        self.rebind()

    # ------------------------------------------------------------------ state
    def _recount(self):
        E, H, W = self.num_envs, self.nrows, self.ncols
        self.buf[0].copy_(self.grids())
        self.parity.zero_()
        call("gca_count_cells", dev.ptr(self.buf[0]), E, H, W, self._empty, self._tree, self._fire,
             dev.ptr(self.counts), dev.stream_ptr(self.device))

    def reset(self, seed=None, grids=None, positions=None):
        """Reset all envs: the grid uniform over {EMPTY, TREE, FIRE} (grid_space.sample(), helicopter.py:33-42) from
        Philox keyed by the global env id, the helicopter at the centre, freeze = max_freeze."""
        import torch

        E, H, W = self.num_envs, self.nrows, self.ncols
        if grids is not None:
            self.buf[0].copy_(dev.to_device(np.asarray(grids).reshape(E, H, W).astype(np.uint8), torch.uint8,
                                            self.device))
        else:
            cdf = torch.tensor([1.0 / 3.0, 2.0 / 3.0, 1.0], dtype=torch.float32, device=self.device)
            vals = torch.tensor([self._empty, self._tree, self._fire], dtype=torch.uint8, device=self.device)
            call("gca_fill_categorical", dev.ptr(self.buf[0]), H * W, E, self.env_offset,
                 seed64(self.seed_value if seed is None else seed), dev.ptr(cdf), dev.ptr(vals), 3,
                 dev.stream_ptr(self.device))
        if positions is not None:
            self.pos.copy_(torch.as_tensor(self._check_positions(positions), device=self.device))
        else:
            self.pos[:, 0] = H // 2
            self.pos[:, 1] = W // 2
        self.parity.zero_()
        self.freeze.fill_(self.max_freeze)
        self.hit.zero_()
        self.reward.zero_()
        self.rng_step.zero_()
        self.steps_elapsed.zero_()
        self._recount()
        return self._obs(), {"hit": self.hit}

    def set_state(self, grid=None, pos=None, freeze=None, rng_step=None):
        """Overwrite parts of the state in place (host arrays or device tensors, leading axis E); the cell counts
        are taken again from the grids."""
        import torch

        E, H, W = self.num_envs, self.nrows, self.ncols
        if grid is not None:
            g = grid if dev.is_device_tensor(grid) else np.asarray(grid).astype(np.uint8)
            self.buf[0].copy_(dev.to_device(g, torch.uint8, self.device).reshape(E, H, W))
            self.parity.zero_()
        if pos is not None:
            p = pos.cpu().numpy() if dev.is_device_tensor(pos) else pos
            self.pos.copy_(torch.as_tensor(self._check_positions(p), device=self.device))
        if freeze is not None:
            f = freeze if dev.is_device_tensor(freeze) else np.broadcast_to(np.asarray(freeze, dtype=np.int64), (E,))
            self.freeze.copy_(dev.to_device(f, torch.int32, self.device).reshape(E))
        if rng_step is not None:
            r = rng_step if dev.is_device_tensor(rng_step) else \
                np.broadcast_to(np.asarray(rng_step, dtype=np.int64), (E,)).astype(np.uint32).view(np.int32)
            self.rng_step.copy_(dev.to_device(r, torch.int32, self.device).reshape(E))
        self._recount()

    def rebind(self):
        """Drop the pre-bound calls. The state tensors are bound by address on the first step and every method here
        updates them in place; assigning a new tensor to one of them calls this by itself (__setattr__, which also
        checks the replacement's dtype / shape / device). The bound calls hold references to what they bound, so
        nothing they address is freed under them."""
        self._step_call = None
        self._random_call = None
        self._sample_call = None
        self._rollout_call = None
        self._observe_calls = {}
        self._policy_calls = {}
        self._info = {"hit": self.hit}
        self._ctx = {"ca_params": self.ca_params, "position": self.pos, "freeze": self.freeze}

    def _bound_tensors(self):
        return (self.thresholds, self.freeze, self.rng_step, self.parity, self.buf, self.pos, self.counts, self.hit,
                self.reward, self.steps_elapsed, self._meet)

    def _bind(self, action, action_seed, action_out, keep=()):
        E, H, W = self.num_envs, self.nrows, self.ncols
        return BoundCall(
            "gca_helicopter_step", self._empty, self._tree, self._fire, self.max_freeze,
            seed64(self.seed_value), self.env_offset, action, action_seed, action_out,
            dev.ptr(self.thresholds), dev.ptr(self.freeze), dev.ptr(self.rng_step), dev.ptr(self.parity),
            dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), H, W, dev.ptr(self.pos), dev.ptr(self.counts),
            dev.ptr(self.hit), dev.ptr(self.reward), dev.ptr(self.steps_elapsed), dev.ptr(self._meet), E, SLOT,
            keep=self._bound_tensors() + tuple(keep))

    def _result(self):
        return self._obs(), self.reward, self._terminated, self._truncated, self._info

    # ------------------------------------------------------------------ step
    def step(self, action):
        """action: (E,) int in [0, 9) (clamped), device tensor or numpy. Returns ((grids | None, context), reward,
        terminated, truncated, info) as device tensors that the next step overwrites in place (terminated and
        truncated are persistent all-False tensors: the env never ends, helicopter.py:137-138); clone to keep them. A
        contiguous int32 (E,) device action is used as it is. One launch, no allocation (with materialize_obs=False)
        and no sync."""
        a = self._action(action)
        sc = self._step_call
        if sc is None:
            sc = self._step_call = self._bind(SLOT, 0, None)
        sc(a.data_ptr(), dev.raw_stream(self._dev_index))
        return self._result()

    def step_random(self, seed=9, action_out=None):
        """One env step of every env under a uniform random policy, the action drawn INSIDE the step exactly as
        sample_actions(out, tag=seed) draws it before step(out): the two in one launch, bit for bit. The drawn actions
        go to `action_out` (a contiguous int32 (E,) device tensor, default the env's action buffer)."""
        import torch

        out = check_tensor(self._act_buf if action_out is None else action_out, torch.int32, self._act_shape,
                           self._dev_index, "step_random", "action_out")
        key = (seed, out.data_ptr())
        rc = self._random_call
        if rc is None or rc[0] != key or rc[1] is not out:
            rc = self._random_call = (key, out, self._bind(None, seed64(seed), dev.ptr(out), keep=(out,)))
        rc[2](dev.raw_stream(self._dev_index))
        return self._result()

    def rollout(self, actions=None, K=None, seed=9, action_out=None, reward_out=None, hit_out=None):
        """K env steps of every env in one call: exactly K step(actions[k]) calls (frame-skip / action-repeat, open-loop
        planners scoring candidate action sequences from one state, recorded trajectories), or with actions=None K
        step_random(seed) calls. actions: (K, E) ints decided before the call; a contiguous int32 device tensor on the
        env's device is used as it is, anything else is converted. Returns (reward_out, hit_out): float64 and uint8
        (K, E) device tensors, row k what step k leaves in env.reward / env.hit (allocated here unless given);
        `action_out` (int32 (K, E), only when given) receives the actions taken, unclamped. Afterwards the env is in the
        state the K calls leave (env.reward, env.hit, grids(), the context tensors), so step / step_random / rollout
        interleave freely. A grid whose two padded planes fit in 64 KiB of LDS runs the K steps in ONE launch
        (gca_helicopter_rollout), other shapes in K launches; no sync either way."""
        import torch

        E = self.num_envs
        a, K = rollout_actions(actions, K, E, (), self.device, self._dev_index, "rollout", convert_host_tensor=True)
        reward_out = self._out(reward_out, torch.float64, (K, E), "rollout", "reward_out")
        hit_out = self._out(hit_out, torch.uint8, (K, E), "rollout", "hit_out")
        if action_out is not None:
            check_tensor(action_out, torch.int32, (K, E), self._dev_index, "rollout", "action_out")
        if K == 0:
            return reward_out, hit_out
        rc = self._rollout_call
        if rc is None:
            H, W = self.nrows, self.ncols
            rc = self._rollout_call = BoundCall(
                "gca_helicopter_rollout", self._empty, self._tree, self._fire, self.max_freeze,
                seed64(self.seed_value), self.env_offset, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT,
                dev.ptr(self.thresholds), dev.ptr(self.freeze), dev.ptr(self.rng_step), dev.ptr(self.parity),
                dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), H, W, dev.ptr(self.pos), dev.ptr(self.counts),
                dev.ptr(self.hit), dev.ptr(self.reward), dev.ptr(self.steps_elapsed), E, SLOT,
                keep=self._bound_tensors())
        rc(None if a is None else a.data_ptr(), seed64(seed), K,
           None if action_out is None else action_out.data_ptr(), reward_out.data_ptr(), hit_out.data_ptr(),
           dev.raw_stream(self._dev_index))
        return reward_out, hit_out

    # ------------------------------------------------------------------ the policy inside the env's launches
    def act(self, policy, local=None, coarse=None, seed=0, greedy=False, action_out=None, logits_out=None,
            value_out=None):
        """The policy's action for every env: observe(policy.radius, policy.block) unless both `local` and `coarse` are
        given (tensors of observe's dtypes and shapes), then ONE launch of the network (gca_helicopter_policy_act).
        Returns (action int32 (E,), logits float32 (E, 9), value float32 (E,)), written into the given outputs or
        allocated. The draw is keyed by (seed, global env id, the env's rng_step); greedy=True takes the first maximum
        instead. No env state changes, so the value of the state after a rollout is free of side effects. No sync."""
        E = self.num_envs
        policy, local, coarse, action_out, logits_out, value_out = self._act_inputs(
            policy, local, coarse, (E,), 9, action_out, logits_out, value_out)
        pc = self._policy_call("act", policy, lambda: (BoundCall(
            "gca_helicopter_policy_act", policy.struct, policy.C, SLOT, SLOT, dev.ptr(self.rng_step), self.env_offset,
            SLOT, SLOT, SLOT, SLOT, SLOT, E, SLOT, keep=(self.rng_step,) + policy.tensors()),))
        pc[2](local.data_ptr(), coarse.data_ptr(), seed64(seed), 1 if greedy else 0, action_out.data_ptr(),
              logits_out.data_ptr(), value_out.data_ptr(), dev.raw_stream(self._dev_index))
        return action_out, logits_out, value_out

    _POLICY_RECORDS = ("action", "logits", "value", "reward", "hit", "local", "coarse")

    def _policy_spec(self, K, ls, cs):
        import torch

        E = self.num_envs
        return {"action": (torch.int32, (K, E)), "logits": (torch.float32, (K, E, 9)),
                "value": (torch.float32, (K, E)), "reward": (torch.float64, (K, E)), "hit": (torch.uint8, (K, E)),
                "local": (torch.uint8, (K,) + ls), "coarse": (torch.float32, (K,) + cs)}

    def rollout_policy(self, policy, K, seed=0, greedy=False, record=_POLICY_RECORDS, action_out=None,
                       logits_out=None, value_out=None, reward_out=None, hit_out=None, local_out=None,
                       coarse_out=None):
        """K closed-loop env steps of every env in one call: bit for bit K x (observe(policy.radius, policy.block),
        act(policy, seed=seed, greedy=greedy), step(action)) -- a PPO collection loop's on-policy experience. Returns a
        dict of the records named in `record` (and of every record whose output tensor is given), row k what step k
        saw and did: action int32 (K, E), logits float32 (K, E, 9), value float32 (K, E), reward float64 (K, E), hit uint8
        (K, E), local uint8 (K, E, S, S), coarse float32 (K, E, 2, Hc, Wc); step k's observation is of the state before
        step k. Given outputs must be contiguous tensors of that dtype and shape on the env's device. Afterwards the env
        is in the state the K steps leave, so step / rollout / rollout_policy interleave freely. Where the grid's two
        planes and the network's scratch fit in LDS all of it is ONE launch (gca_helicopter_policy_rollout), other shapes
        run 3 K launches with the same results; no sync either way."""
        import torch

        E = self.num_envs
        policy, K, recs = self._policy_records(policy, K, record, {
            "action": action_out, "logits": logits_out, "value": value_out, "reward": reward_out, "hit": hit_out,
            "local": local_out, "coarse": coarse_out})
        if K == 0:
            return recs

        def make():
            H, W = self.nrows, self.ncols
            # the K x 3 launch path keeps a step's action / window / coarse map here when the caller keeps no record
            scratch = torch.empty(E * (4 + 4 * policy.C + policy.S * policy.S), dtype=torch.uint8, device=self.device)
            return BoundCall(
                "gca_helicopter_policy_rollout", self._empty, self._tree, self._fire, self.max_freeze,
                seed64(self.seed_value), self.env_offset, policy.struct, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT,
                SLOT, SLOT, SLOT, dev.ptr(scratch), dev.ptr(self.thresholds), dev.ptr(self.freeze),
                dev.ptr(self.rng_step), dev.ptr(self.parity), dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), H, W,
                dev.ptr(self.pos), dev.ptr(self.counts), dev.ptr(self.hit), dev.ptr(self.reward),
                dev.ptr(self.steps_elapsed), E, SLOT,
                keep=self._bound_tensors() + policy.tensors() + (scratch,)),

        pc = self._policy_call("rollout", policy, make)
        p = lambda name: recs[name].data_ptr() if name in recs else None
        pc[2](seed64(seed), 1 if greedy else 0, K, p("action"), p("logits"), p("value"), p("reward"),
              p("hit"), p("local"), p("coarse"), dev.raw_stream(self._dev_index))
        return recs

    def sample_actions(self, out=None, tag=9):
        """Uniform random actions in [0, 9) for every env on the device -- the batched `action_space.sample()`: column
        0 of gca_random_actions (Philox keyed by (tag, global env id, the env's rng_step)) -- into `out` (a contiguous
        int32 (E,) device tensor) or the env's action buffer. Returns the tensor."""
        import torch

        out = check_tensor(self._act_buf if out is None else out, torch.int32, self._act_shape, self._dev_index,
                           "sample_actions", "out")
        sc = self._sample_call
        if sc is None or sc[0] != tag:
            sc = self._sample_call = (tag, BoundCall("gca_random_actions", dev.ptr(self._act2), self.num_envs,
                                                     self.env_offset, seed64(tag), dev.ptr(self.rng_step),
                                                     SLOT, keep=(self._act2, self.rng_step)))
        sc[1](dev.raw_stream(self._dev_index))
        out.copy_(self._act2[:, 0])
        return out
