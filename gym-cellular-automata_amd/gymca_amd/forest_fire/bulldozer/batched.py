"""BatchedForestFireBulldozerEnv — E ForestFireBulldozer envs resident in HBM.

The batched form of bulldozer.py's MDP (reference bulldozer.py:378-400 +
ca_env.py:27-62), one env per lane of the env kernels and one strip of rows per
wave of the CA kernel:

    gca_bulldozer_pre        RepeatCA time bookkeeping (repeat_ca.py:32-45), dir mask (ca_windy.py:53-77)
    gca_windy_step  x P      the CA passes (P = max repeats any action can trigger)
    gca_bulldozer_interpass  between passes (parity flip + next roll)
    gca_bulldozer_post       Move/Modify (move_modify.py:128-134), reward/done (bulldozer.py:180-216)

or, when every action takes less than one time unit (one CA pass at most per env step) and W is 256 or 512 (the
bench configs 2 and 5), the same step in ONE launch (gca_bulldozer_step_fused: a workgroup per env; envs without a CA
step this env step leave after their O(1) work). `fused=None` picks it whenever it applies; the two paths are
checked to give identical envs (tests/test_gpu_windy.py).

Episodes: `reset()` starts episode 0 of every env; `reset_where()` (gca_bulldozer_reset_where, one launch, no host work)
starts a new episode of the selected envs only, and `autoreset=True` launches it right after every step for the envs
that finished (or reached `max_episode_steps`): Gymnasium's same-step autoreset, the reference's stateless_step ->
conditional_reset pair. With both options off nothing of this runs. `rollout(actions)` runs K steps of every env, and
under autoreset the resets between them, in ONE launch (gca_bulldozer_rollout): bit for bit the K step calls.

Grids live in two buffers; env e's current grid is buf[parity[e]][e], so envs whose
RepeatCA yields 0 repeats this step (most of them: ~1 CA step per 13 env steps at
256^2 with random actions) move no bytes at all. Cell counts are
fused into the CA kernel and patched by Modify, so reward/done are O(1) per env.
"""
import math

import numpy as np

from ... import _device as dev
from ..._lib import SLOT, BoundCall, call
from .._batched import BatchedEnvBase, check_tensor, rollout_actions, seed64
from ..operators.move_modify import make_params
from .bulldozer import ACTION_SETS, DEFAULT_WIND, bulldozer_timings, parse_wind
from .policy import BulldozerPolicy


class BatchedForestFireBulldozerEnv(BatchedEnvBase):
    # state the pre-bound calls hold by address (step, step_random, sample_actions): assigning one of these attributes
    # validates the replacement and drops the bound calls (BatchedEnvBase.__setattr__)
    _BOUND_STATE = frozenset({"buf", "parity", "accu", "steps", "dir_mask", "counts", "pos", "rng_step", "done", "hit",
                              "reward", "wind", "steps_elapsed", "params", "_meet", "_act_buf", "episode",
                              "last_episode_length", "_terminated", "_truncated_u8"})
    _BOUND_READY = "_fused_call"
    _POLICY_CLASS = BulldozerPolicy

    def _check_replacement(self, name, old, value):
        # the two bound attributes that are no tensor: params keeps its type, _meet may be switched off
        if name == "params":
            if type(value) is not type(old):
                raise TypeError(f"params must stay a {type(old).__name__}")
        elif not (name == "_meet" and value is None):
            super()._check_replacement(name, old, value)

    def __init__(self, num_envs, nrows, ncols, device=None, seed=0, env_offset=0, speed_move=0.12, speed_act=0.03,
                 t_move=None, t_shoot=None, t_any=0.001, p_tree=0.90, p_empty=0.10, wind=DEFAULT_WIND,
                 materialize_obs=True, fused=None, autoreset=False, max_episode_steps=None):
        import torch

        if max_episode_steps is not None and int(max_episode_steps) <= 0:
            raise ValueError("max_episode_steps must be positive (or None: no time limit)")
        self.autoreset = bool(autoreset)
        self.max_episode_steps = None if max_episode_steps is None else int(max_episode_steps)

        self.device = dev.require_device(device)
        self.num_envs, self.nrows, self.ncols = E, H, W = int(num_envs), int(nrows), int(ncols)
        self.seed_value = int(seed)
        self.env_offset = int(env_offset)
        self.materialize_obs = materialize_obs
        self._empty, self._tree, self._fire = 0, 3, 25
        self._p_tree, self._p_empty = p_tree, p_empty
        t_act_move, t_act_shoot = bulldozer_timings(H, W, speed_move, speed_act, t_move, t_shoot, t_any)
        self.t_act_move, self.t_act_shoot, self.t_any = t_act_move, t_act_shoot, t_any
        p = make_params(ACTION_SETS, {self._tree: self._empty})
        for a in range(9):
            p.t_move[a] = 0.0 if a == 4 else t_act_move  # not_move costs _t_act_none (bulldozer.py:285)
        p.t_shoot[0], p.t_shoot[1] = 0.0, t_act_shoot
        p.t_any = t_any
        p.seed = seed64(self.seed_value)
        p.env_offset = self.env_offset
        p.empty, p.tree, p.fire = self._empty, self._tree, self._fire
        self.params = p
        max_t = max(p.t_move[a] for a in range(9)) + max(p.t_shoot[0], p.t_shoot[1]) + t_any
        self.max_passes = int(math.floor(1.0 + max_t))  # accu < 1 before the step
        # gca_bulldozer_step_fused's contract: W = 256 / 512, one pass at most, empty == 0 < tree < fire (the closed-form
        # rule's code ordering); anything else takes the three-kernel step
        fusable = (self.max_passes == 1 and W in (256, 512) and self._empty == 0
                   and self._empty < self._tree < self._fire)
        if fused and not fusable:
            raise ValueError("fused=True needs W in (256, 512), at most one CA pass per env step and codes "
                             "empty = 0 < tree < fire")
        self.fused = fusable if fused is None else bool(fused)
        kw = dict(device=self.device)
        self.buf = torch.zeros((2, E, H, W), dtype=torch.uint8, **kw)
        self.parity = torch.zeros(E, dtype=torch.uint8, **kw)
        self.accu = torch.zeros(E, dtype=torch.float64, **kw)
        self.steps = torch.zeros(E, dtype=torch.int32, **kw)
        self.dir_mask = torch.zeros(E, dtype=torch.uint8, **kw)
        self.counts = torch.zeros((E, 3), dtype=torch.int32, **kw)
        self.pos = torch.zeros((E, 2), dtype=torch.int32, **kw)
        self.rng_step = torch.zeros(E, dtype=torch.int32, **kw)  # uint32 bits
        self.done = torch.zeros(E, dtype=torch.uint8, **kw)
        self.hit = torch.zeros(E, dtype=torch.uint8, **kw)
        self.reward = torch.zeros(E, dtype=torch.float64, **kw)
        w = parse_wind(wind) if isinstance(wind, dict) else np.asarray(wind, dtype=np.float64)
        self.wind = dev.to_device(np.broadcast_to(w.reshape(-1, 9), (E, 9)), torch.float64, self.device)
        self.steps_elapsed = torch.zeros(E, dtype=torch.int64, **kw)
        # the fused step's per-env meeting slots (gca_bulldozer_step_fused: several workgroups per env), kept zero
        self._meet = torch.zeros(E, dtype=torch.int64, **kw)
        self._truncated = torch.zeros(E, dtype=torch.bool, **kw)
        # per-env episodes (reset_where / autoreset): the episode index keys the reset's draws; the two flag tensors are
        # what the reset launch saw on entry (done, and the time limit reached without done)
        self.episode = torch.zeros(E, dtype=torch.int32, **kw)  # uint32 bits
        self.last_episode_length = torch.zeros(E, dtype=torch.int64, **kw)
        self._terminated = torch.zeros(E, dtype=torch.uint8, **kw)
        self._truncated_u8 = torch.zeros(E, dtype=torch.uint8, **kw)
        self._reset_seed = p.seed
        self._reset_cdf = torch.tensor([p_empty, p_empty + p_tree, 1.0], dtype=torch.float32, device=self.device)
        self._reset_vals = torch.tensor([self._empty, self._tree, self._fire], dtype=torch.uint8, device=self.device)
        # the eager step's host path: persistent outputs and pre-bound C-ABI calls, so a step is
        # one action check, one raw-stream read and one prepared ctypes call
        self._dev_index = dev.device_index(self.device)
        self._act_buf = torch.zeros((E, 2), dtype=torch.int32, **kw)
        self._act_shape = self._act_buf.shape
        self._views()
        self._fused_call = self._bound_meet = None
        self._sample_call = None
        self._random_call = self._bound_meet_r = None
        self._reset_call = None
        self._rollout_call = None
        self._observe_calls = {}
        self._policy_calls = {}

    # ------------------------------------------------------------------ state
    def reset(self, seed=None, grids=None, positions=None):
        """Reset all envs. Initial distribution of bulldozer.py:233-275: the grid from Philox per cell, the fire /
        bulldozer noise from per-env draws keyed by the global env id (_seeding), so a sharded env reproduces the
        unsharded one env for env."""
        import torch

        from ..._seeding import env_integers

        E, H, W = self.num_envs, self.nrows, self.ncols
        st = dev.stream_ptr(self.device)
        s = self.seed_value if seed is None else int(seed)
        noise = lambda tag, n: env_integers(s, self.env_offset, E, tag, 0, max(1, int(n / 12)))
        if grids is not None:
            self.buf[0].copy_(dev.to_device(np.asarray(grids).reshape(E, H, W).astype(np.uint8), torch.uint8,
                                            self.device))
        else:
            cdf = torch.tensor([self._p_empty, self._p_empty + self._p_tree, 1.0], dtype=torch.float32,
                               device=self.device)
            vals = torch.tensor([self._empty, self._tree, self._fire], dtype=torch.uint8, device=self.device)
            call("gca_fill_categorical", dev.ptr(self.buf[0]), H * W, E, self.env_offset,
                 seed64(s), dev.ptr(cdf), dev.ptr(vals), 3, st)
            # one FIRE around the lower-left quadrant, noise in [0, N/12) (bulldozer.py:221-253)
            fr = 3 * H // 4 + noise(1, H)
            fc = W // 4 + noise(2, W)
            idx = torch.arange(E, device=self.device)
            self.buf[0][idx, torch.as_tensor(fr, device=self.device), torch.as_tensor(fc, device=self.device)] = \
                self._fire
        if positions is not None:
            pos = self._check_positions(positions)
        else:
            pos = np.stack([H // 4 + noise(3, H), 3 * W // 4 + noise(4, W)], axis=1)
        self.pos.copy_(torch.as_tensor(pos.astype(np.int32), device=self.device))
        self.parity.zero_()
        self.accu.zero_()
        self.done.zero_()
        self.hit.zero_()
        self.rng_step.zero_()
        self.steps_elapsed.zero_()
        self.episode.zero_()
        self._reset_seed = seed64(s)  # reset_where draws the later episodes from the same seed
        call("gca_count_cells", dev.ptr(self.buf[0]), E, H, W, self._empty, self._tree, self._fire,
             dev.ptr(self.counts), st)
        return self._obs(), {"hit": self.hit}

    def rebind(self):
        """Drop the pre-bound step calls. The env's state tensors (buf, accu, steps, done, wind, rng_step, parity, pos,
        counts, hit, reward, steps_elapsed) and params are bound by address on the first fused step; every method here
        updates them in place. Assigning a new tensor to one of them (env.wind = w) calls this by itself
        (__setattr__, which also checks the replacement's dtype / shape / device); the bound calls hold references to
        what they bound, so nothing they address is ever freed under them."""
        self._fused_call = self._bound_meet = None
        self._sample_call = None
        self._random_call = self._bound_meet_r = None
        self._reset_call = None
        self._rollout_call = None
        self._observe_calls = {}
        self._policy_calls = {}
        self._views()

    def _views(self):
        """The persistent objects a step returns: bool views of the flag tensors and the info / context dicts."""
        import torch

        self._done_bool = self.done.view(torch.bool)
        self._info = {"hit": self.hit, "ca_steps": self.steps}
        self._ctx = {"wind": self.wind, "position": self.pos, "time": self.accu}
        if self.autoreset:
            self._info.update(episode=self.episode, last_episode_length=self.last_episode_length)
        self._term_bool = self._terminated.view(torch.bool)
        self._trunc_bool = self._truncated_u8.view(torch.bool)

    # ------------------------------------------------------------------ per-env reset
    def _launch_reset(self, mask_ptr, max_steps, set_episode):
        rc = self._reset_call
        if rc is None:
            E, H, W = self.num_envs, self.nrows, self.ncols
            rc = self._reset_call = BoundCall(
                "gca_bulldozer_reset_where", self.params, SLOT, SLOT, SLOT, SLOT, dev.ptr(self._reset_cdf),
                dev.ptr(self._reset_vals), dev.ptr(self.done), dev.ptr(self._terminated), dev.ptr(self._truncated_u8),
                dev.ptr(self.episode), dev.ptr(self.last_episode_length), dev.ptr(self.accu), dev.ptr(self.parity),
                dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), H, W, dev.ptr(self.pos), dev.ptr(self.counts),
                dev.ptr(self.hit), dev.ptr(self.steps_elapsed), E, SLOT,
                keep=self._bound_tensors() + (self._reset_cdf, self._reset_vals, self._terminated, self._truncated_u8,
                                              self.episode, self.last_episode_length))
        rc(self._reset_seed, mask_ptr, max_steps, set_episode, dev.raw_stream(self._dev_index))

    def _autoreset(self):
        """The reset launch that follows a step under autoreset=True: the envs that are done, or at their time limit,
        start their next episode; the step's return values are the terminal step's reward, the flags the launch saw
        and the new episode's observation."""
        self._launch_reset(None, self.max_episode_steps or 0, -1)
        return self._obs(), self.reward, self._term_bool, self._trunc_bool, self._info

    def reset_where(self, mask=None, episode=None):
        """Start a new episode of the selected envs in one launch on the device (gca_bulldozer_reset_where); every
        other env is left untouched, bit for bit. mask: a uint8 / bool (E,) device tensor or numpy array, non-zero =
        reset; None selects the envs that are done and, with max_episode_steps, those at their time limit. episode:
        None moves each selected env to its next episode index; an int replays that index (0 = the state reset() gave
        with the same seed). The grid, the fire cell and the bulldozer's position are keyed by (the last reset()'s
        seed, global env id, episode index), so a sharded env resets like the unsharded one; rng_step runs on, so the
        new episode's Windy rolls and sampled actions do not replay the last episode's. Returns (obs, info)."""
        import torch

        E = self.num_envs
        if mask is None:
            mask_ptr, max_steps = None, self.max_episode_steps or 0
        else:
            if isinstance(mask, torch.Tensor):
                if mask.device != self.done.device:
                    raise ValueError(f"reset_where: mask must be on {self.done.device} (or a numpy array)")
                m = mask
            else:
                m = np.asarray(mask)
            if str(m.dtype).replace("torch.", "") not in ("uint8", "bool") or tuple(m.shape) != (E,):
                raise ValueError(f"reset_where: mask must be a uint8 or bool array of shape ({E},)")
            if not isinstance(m, torch.Tensor):
                m = dev.to_device(m.astype(np.uint8), torch.uint8, self.device)
            m = m.contiguous()
            m = m.view(torch.uint8) if m.dtype is torch.bool else m
            mask_ptr, max_steps = m.data_ptr(), 0
        if episode is None:
            set_episode = -1
        else:
            set_episode = int(episode)
            if set_episode != episode or not 0 <= set_episode < 2**32:
                raise ValueError("reset_where: episode must be an int in [0, 2**32) (or None: the next episode)")
        # `m` stays alive until the launch is enqueued; its memory is reused in stream order only
        self._launch_reset(mask_ptr, max_steps, set_episode)
        return self._obs(), {"hit": self.hit, "episode": self.episode,
                             "last_episode_length": self.last_episode_length}

    def _bound_tensors(self):
        return (self.params, self.accu, self.steps, self.done, self.wind, self.rng_step, self.parity, self.buf,
                self.pos, self.counts, self.hit, self.reward, self.steps_elapsed, self._meet)

    def _bind_fused(self):
        E, H, W = self.num_envs, self.nrows, self.ncols
        meet = self._meet
        self._fused_call = BoundCall(
            "gca_bulldozer_step_fused", self.params, SLOT, dev.ptr(self.accu), dev.ptr(self.steps), dev.ptr(self.done),
            dev.ptr(self.wind), 9, dev.ptr(self.rng_step), dev.ptr(self.parity), dev.ptr(self.buf[0]),
            dev.ptr(self.buf[1]), H, W, dev.ptr(self.pos), dev.ptr(self.counts), dev.ptr(self.hit),
            dev.ptr(self.reward), dev.ptr(self.steps_elapsed), dev.ptr(meet) if meet is not None else None, E, SLOT,
            keep=self._bound_tensors())
        self._bound_meet = meet
        return self._fused_call

    def step_random(self, seed=9, action_out=None):
        """One env step of every env under a uniform random policy, the action drawn INSIDE the fused step
        (gca_bulldozer_step_fused_random) exactly as sample_actions(out, tag=seed) draws it before step(out): the two
        launches in one, bit for bit. The drawn actions go to `action_out` (a contiguous int32 (E, 2) device tensor,
        default the env's action buffer). Fused step only (W = 256 / 512, one CA pass at most per env step)."""
        if not self.fused:
            raise ValueError("step_random needs the fused step (W in (256, 512), at most one CA pass per env step)")
        import torch

        out = self._act_buf if action_out is None else action_out
        check_tensor(out, torch.int32, self._act_shape, self._dev_index, "step_random", "action_out")
        key = (seed, out.data_ptr())
        rc = self._random_call
        if rc is None or rc[0] != key or rc[1] is not out or self._bound_meet_r is not self._meet:
            E, H, W = self.num_envs, self.nrows, self.ncols
            meet = self._meet
            self._random_call = (key, out, BoundCall(
                "gca_bulldozer_step_fused_random", self.params, seed64(seed), dev.ptr(out),
                dev.ptr(self.accu), dev.ptr(self.steps), dev.ptr(self.done), dev.ptr(self.wind), 9,
                dev.ptr(self.rng_step), dev.ptr(self.parity), dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), H, W,
                dev.ptr(self.pos), dev.ptr(self.counts), dev.ptr(self.hit), dev.ptr(self.reward),
                dev.ptr(self.steps_elapsed), dev.ptr(meet) if meet is not None else None, E, SLOT,
                keep=self._bound_tensors() + (out,)))
            self._bound_meet_r = meet
        self._random_call[2](dev.raw_stream(self._dev_index))
        if self.autoreset:
            return self._autoreset()
        return self._obs(), self.reward, self._done_bool, self._truncated, self._info

    def rollout_random(self, K, seed=9, action_out=None, reward_out=None, done_out=None):
        """K env steps of every env in ONE launch under the random policy of step_random (gca_bulldozer_rollout_random):
        bit for bit K calls of step_random(seed), the env's state kept in registers across the steps. Optional per-step
        records, device tensors: action_out int32 (K, E, 2), reward_out float64 (K, E), done_out uint8 (K, E). Returns
        (reward_out, done_out). Fused step only (W = 256 / 512, one CA pass at most per env step)."""
        import torch

        if not self.fused:
            raise ValueError("rollout_random needs the fused step (W in (256, 512), at most one CA pass per env step)")
        if self.autoreset or self.max_episode_steps is not None:
            raise ValueError("rollout_random runs no per-env reset: not available with autoreset or max_episode_steps")
        K, E = int(K), self.num_envs
        if K < 0:
            raise ValueError("rollout_random: K >= 0")
        for name, t, dt, shape in (("action_out", action_out, torch.int32, (K, E, 2)),
                                   ("reward_out", reward_out, torch.float64, (K, E)),
                                   ("done_out", done_out, torch.uint8, (K, E))):
            if t is not None:
                check_tensor(t, dt, shape, self._dev_index, "rollout_random", name)
        H, W = self.nrows, self.ncols
        call("gca_bulldozer_rollout_random", self.params, seed64(seed), K, dev.ptr(action_out),
             dev.ptr(reward_out), dev.ptr(done_out), dev.ptr(self.accu), dev.ptr(self.steps), dev.ptr(self.done),
             dev.ptr(self.wind), 9, dev.ptr(self.rng_step), dev.ptr(self.parity), dev.ptr(self.buf[0]),
             dev.ptr(self.buf[1]), H, W, dev.ptr(self.pos), dev.ptr(self.counts), dev.ptr(self.hit), dev.ptr(self.reward),
             dev.ptr(self.steps_elapsed), E, dev.stream_ptr(self.device))
        return reward_out, done_out

    def rollout(self, actions=None, K=None, seed=9, action_out=None, reward_out=None, terminated_out=None,
                truncated_out=None):
        """K env steps of every env in one call: exactly K step(actions[k]) calls (frame-skip / action-repeat, open-loop
        planners, recorded trajectories), or with actions=None K step_random(seed) calls, under the env's own
        `autoreset` and `max_episode_steps`: with autoreset=True an env that finishes (or reaches its time limit) at step
        k starts its next episode before step k + 1, as the reset launch after an eager step does; with autoreset=False
        finished envs take the no-op step and max_episode_steps is ignored, as step ignores it. actions: (K, E, 2) ints
        decided before the call (clamped as step clamps them); a contiguous int32 tensor on the env's device is used as
        it is, anything else is converted. Returns (reward_out, terminated_out, truncated_out): float64 / uint8 / uint8
        (K, E) device tensors, allocated here unless given; row k holds what step k leaves in env.reward (the terminal
        step's reward where an episode ended) and the flags of step k (under autoreset what the reset saw, otherwise
        `done` and zeros). `action_out` (int32 (K, E, 2), only when given) receives the actions taken, unclamped.
        Afterwards every state tensor, both grid planes and env.reward are what the K calls leave, so step / step_random /
        reset_where / rollout interleave freely. With the fused step (W = 256 / 512, one CA pass at most per env step)
        the K steps and the resets between them are ONE launch (gca_bulldozer_rollout), a resetting env overlapping the
        other envs' steps; otherwise K x (the launches of a step). No sync either way, and with every record given and
        device int32 actions no allocation: the call can be captured in a graph."""
        import torch

        E = self.num_envs
        a, K = rollout_actions(actions, K, E, (2,), self.device, self._dev_index, "rollout", convert_host_tensor=False)
        reward_out = self._out(reward_out, torch.float64, (K, E), "rollout", "reward_out")
        terminated_out = self._out(terminated_out, torch.uint8, (K, E), "rollout", "terminated_out")
        truncated_out = self._out(truncated_out, torch.uint8, (K, E), "rollout", "truncated_out")
        if action_out is not None:
            check_tensor(action_out, torch.int32, (K, E, 2), self._dev_index, "rollout", "action_out")
        if K == 0:
            return reward_out, terminated_out, truncated_out
        if not self.fused:
            # K x (the launches of a step): each step's results copied into the records on the device
            for k in range(K):
                ak = self.sample_actions(tag=seed) if a is None else a[k]
                self.step(ak)
                if action_out is not None:
                    action_out[k].copy_(ak)
                reward_out[k].copy_(self.reward)
                if self.autoreset:
                    terminated_out[k].copy_(self._terminated)
                    truncated_out[k].copy_(self._truncated_u8)
                else:
                    terminated_out[k].copy_(self.done)
                    truncated_out[k].zero_()
            return reward_out, terminated_out, truncated_out
        rc = self._rollout_call
        if rc is None:
            H, W = self.nrows, self.ncols
            rc = self._rollout_call = BoundCall(
                "gca_bulldozer_rollout", self.params, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT,
                dev.ptr(self._reset_cdf), dev.ptr(self._reset_vals), dev.ptr(self.episode),
                dev.ptr(self.last_episode_length), dev.ptr(self._terminated), dev.ptr(self._truncated_u8),
                dev.ptr(self.accu), dev.ptr(self.steps), dev.ptr(self.done), dev.ptr(self.wind), 9,
                dev.ptr(self.rng_step), dev.ptr(self.parity), dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), H, W,
                dev.ptr(self.pos), dev.ptr(self.counts), dev.ptr(self.hit), dev.ptr(self.reward),
                dev.ptr(self.steps_elapsed), E, SLOT,
                keep=self._bound_tensors() + (self._reset_cdf, self._reset_vals, self._terminated, self._truncated_u8,
                                              self.episode, self.last_episode_length))
        rc(None if a is None else a.data_ptr(), seed64(seed), K,
           None if action_out is None else action_out.data_ptr(), reward_out.data_ptr(), terminated_out.data_ptr(),
           truncated_out.data_ptr(), 1 if self.autoreset else 0, self._reset_seed,
           (self.max_episode_steps or 0) if self.autoreset else 0, dev.raw_stream(self._dev_index))
        return reward_out, terminated_out, truncated_out

    # ------------------------------------------------------------------ the policy inside the env's launches
    def act(self, policy, local=None, coarse=None, seed=0, greedy=False, action_out=None, logits_out=None,
            value_out=None):
        """The policy's (move, shoot) for every env: observe(policy.radius, policy.block) unless both `local` and
        `coarse` are given (tensors of observe's dtypes and shapes), then ONE launch of the network
        (gca_bulldozer_policy_act). Returns (action int32 (E, 2), logits float32 (E, 11): nine move logits then two shoot
        logits, value float32 (E,)), written into the given outputs or allocated. The draw is keyed by (seed, global env
        id, the env's steps_elapsed and episode); greedy=True takes the first maximum of each head instead. No env state
        changes, so the value of the state after a rollout (the bootstrap) is free of side effects. No sync."""
        E = self.num_envs
        policy, local, coarse, action_out, logits_out, value_out = self._act_inputs(
            policy, local, coarse, (E, 2), 11, action_out, logits_out, value_out)
        pc = self._policy_call("act", policy, lambda: (BoundCall(
            "gca_bulldozer_policy_act", policy.struct, policy.C, SLOT, SLOT, dev.ptr(self.steps_elapsed),
            dev.ptr(self.episode), self.env_offset, SLOT, SLOT, SLOT, SLOT, SLOT, E, SLOT,
            keep=(self.steps_elapsed, self.episode) + policy.tensors()),))
        pc[2](local.data_ptr(), coarse.data_ptr(), seed64(seed), 1 if greedy else 0, action_out.data_ptr(),
              logits_out.data_ptr(), value_out.data_ptr(), dev.raw_stream(self._dev_index))
        return action_out, logits_out, value_out

    _POLICY_RECORDS = ("action", "logits", "value", "reward", "terminated", "truncated", "local", "coarse")

    def _policy_spec(self, K, ls, cs):
        import torch

        E = self.num_envs
        return {"action": (torch.int32, (K, E, 2)), "logits": (torch.float32, (K, E, 11)),
                "value": (torch.float32, (K, E)), "reward": (torch.float64, (K, E)),
                "terminated": (torch.uint8, (K, E)), "truncated": (torch.uint8, (K, E)),
                "local": (torch.uint8, (K,) + ls), "coarse": (torch.float32, (K,) + cs)}

    def rollout_policy(self, policy, K, seed=0, greedy=False, record=_POLICY_RECORDS, action_out=None,
                       logits_out=None, value_out=None, reward_out=None, terminated_out=None, truncated_out=None,
                       local_out=None, coarse_out=None):
        """K closed-loop env steps of every env in one call: bit for bit K x (observe(policy.radius, policy.block),
        act(policy, seed=seed, greedy=greedy), step(action)) under the env's own `autoreset` / `max_episode_steps` -- a
        PPO collection loop's on-policy experience, episode ends included. Returns a dict of the records named in
        `record` (and of every record whose output tensor is given), row k what step k saw and did: action int32
        (K, E, 2), logits float32 (K, E, 11), value float32 (K, E), reward float64 (K, E), terminated / truncated uint8
        (K, E) as rollout() defines them, local uint8 (K, E, S, S), coarse float32 (K, E, 2, Hc, Wc); step k's observation
        is of the state before step k, so under autoreset row k + 1 after an episode's end is the new episode's. An env
        that is done without autoreset keeps observing, acting and recording its no-op step. Given outputs must be
        contiguous tensors of that dtype and shape on the env's device. Afterwards the env is in the state the K steps
        leave, so step / rollout / rollout_policy interleave freely. With the fused step, block 8 / 16 / 32 dividing H
        and a coarse map that fits in LDS everything is ONE launch (gca_bulldozer_policy_rollout); other fused shapes run
        the K x 3 (+ reset) launches inside that call, a non-fused env K x (observe, act, step) from here with device
        copies into the records. No sync, and with every record given no allocation: capturable."""
        import torch

        E = self.num_envs
        policy, K, recs = self._policy_records(policy, K, record, {
            "action": action_out, "logits": logits_out, "value": value_out, "reward": reward_out,
            "terminated": terminated_out, "truncated": truncated_out, "local": local_out, "coarse": coarse_out})
        if K == 0:
            return recs
        if not self.fused:
            return self._rollout_policy_steps(policy, K, seed, greedy, recs)

        def make():
            H, W = self.nrows, self.ncols
            # the K x 3 launch path keeps a step's action / window / coarse map here when the caller keeps no record
            scratch = torch.empty(E * (8 + 4 * policy.C + policy.S * policy.S), dtype=torch.uint8, device=self.device)
            return BoundCall(
                "gca_bulldozer_policy_rollout", self.params, policy.struct, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT, SLOT,
                SLOT, SLOT, SLOT, SLOT, dev.ptr(scratch), SLOT, SLOT, SLOT, dev.ptr(self._reset_cdf),
                dev.ptr(self._reset_vals), dev.ptr(self.episode), dev.ptr(self.last_episode_length),
                dev.ptr(self._terminated), dev.ptr(self._truncated_u8), dev.ptr(self.accu), dev.ptr(self.steps),
                dev.ptr(self.done), dev.ptr(self.wind), 9, dev.ptr(self.rng_step), dev.ptr(self.parity),
                dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), H, W, dev.ptr(self.pos), dev.ptr(self.counts),
                dev.ptr(self.hit), dev.ptr(self.reward), dev.ptr(self.steps_elapsed), E, SLOT,
                keep=self._bound_tensors() + policy.tensors() + (
                    scratch, self._reset_cdf, self._reset_vals, self._terminated, self._truncated_u8, self.episode,
                    self.last_episode_length)),

        pc = self._policy_call("rollout", policy, make)
        p = lambda name: recs[name].data_ptr() if name in recs else None
        pc[2](seed64(seed), 1 if greedy else 0, K, p("action"), p("logits"), p("value"), p("reward"), p("terminated"),
              p("truncated"), p("local"), p("coarse"), 1 if self.autoreset else 0, self._reset_seed,
              (self.max_episode_steps or 0) if self.autoreset else 0, dev.raw_stream(self._dev_index))
        return recs

    def _rollout_policy_steps(self, policy, K, seed, greedy, recs):
        """rollout_policy of a non-fused env: K x (observe, act, step), each step's results copied into the records on
        the device. The observation and the network's outputs go straight into their record rows where those exist."""
        import torch

        from .. import policy_obs

        E = self.num_envs
        ls, cs = policy_obs.output_shapes(self, policy.radius, policy.block)
        tmp = {"local": torch.empty(ls, dtype=torch.uint8, device=self.device),
               "coarse": torch.empty(cs, dtype=torch.float32, device=self.device),
               "action": torch.empty((E, 2), dtype=torch.int32, device=self.device),
               "logits": torch.empty((E, 11), dtype=torch.float32, device=self.device),
               "value": torch.empty(E, dtype=torch.float32, device=self.device)}
        row = lambda name, k: recs[name][k] if name in recs else tmp[name]
        for k in range(K):
            lo, co = self.observe(policy.radius, policy.block, row("local", k), row("coarse", k))
            a, _, _ = self.act(policy, lo, co, seed, greedy, row("action", k), row("logits", k), row("value", k))
            self.step(a)
            if "reward" in recs:
                recs["reward"][k].copy_(self.reward)
            if "terminated" in recs:
                recs["terminated"][k].copy_(self._terminated if self.autoreset else self.done)
            if "truncated" in recs:
                if self.autoreset:
                    recs["truncated"][k].copy_(self._truncated_u8)
                else:
                    recs["truncated"][k].zero_()
        return recs

    def sample_actions(self, out=None, tag=9):
        """Uniform random actions for every env on the device -- the batched `action_space.sample()` (move in [0, 9),
        shoot in {0, 1}; Philox keyed by (tag, global env id, the env's rng_step)) -- into `out` (a contiguous int32
        (E, 2) device tensor) or the env's action buffer. Returns the tensor."""
        import torch

        out = self._act_buf if out is None else out
        check_tensor(out, torch.int32, self._act_shape, self._dev_index, "sample_actions", "out")
        sc = self._sample_call
        if sc is None or sc[0] is not out or sc[1] != tag or sc[2] != out.data_ptr():
            self._sample_call = (out, tag, out.data_ptr(),
                                 BoundCall("gca_random_actions", dev.ptr(out), self.num_envs, self.env_offset,
                                           seed64(tag), dev.ptr(self.rng_step), SLOT, keep=(out, self.rng_step)))
        self._sample_call[3](dev.raw_stream(self._dev_index))
        return out

    # ------------------------------------------------------------------ step
    def step(self, action):
        """action: (E, 2) int (move in [0,9), shoot in {0,1}); device tensor or numpy. Returns (obs, reward,
        terminated, truncated, info) as device tensors that the next step overwrites in place (terminated is a bool
        view of `done`, truncated a persistent all-False tensor, info one persistent dict: no kernel launch and no
        allocation per step); clone to keep them. A contiguous int32 (E, 2) device action is used as it is.
        autoreset=True: one more launch resets the envs this step finished (or that reached max_episode_steps): reward
        is the terminal step's, terminated / truncated are bool views of what that launch saw, the observation is
        already the new episode's, and info carries `episode` and `last_episode_length` (persistent tensors)."""
        a = self._action(action)
        if self.fused:
            fc = self._fused_call if self._bound_meet is self._meet else None
            if fc is None:
                fc = self._bind_fused()
            fc(a.data_ptr(), dev.raw_stream(self._dev_index))
            if self.autoreset:
                return self._autoreset()
            # done is 0 / 1 bytes: a bool view, no kernel; truncated is a persistent all-False tensor
            return self._obs(), self.reward, self._done_bool, self._truncated, self._info
        import torch

        E, H, W = self.num_envs, self.nrows, self.ncols
        st = dev.stream_ptr(self.device)
        p = self.params
        call("gca_bulldozer_pre", p, dev.ptr(a), dev.ptr(self.accu), dev.ptr(self.steps), dev.ptr(self.done),
             dev.ptr(self.wind), 9, dev.ptr(self.rng_step), dev.ptr(self.dir_mask), dev.ptr(self.counts), E, st)
        P = self.max_passes
        for pss in range(P):
            call("gca_windy_step", dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), dev.ptr(self.parity),
                 dev.ptr(self.steps), pss, dev.ptr(self.dir_mask), E, H, W, self._empty, self._tree, self._fire, 0,
                 dev.ptr(self.counts), st)
            if pss < P - 1:
                call("gca_bulldozer_interpass", p, pss, dev.ptr(self.steps), dev.ptr(self.parity),
                     dev.ptr(self.wind), 9, dev.ptr(self.rng_step), dev.ptr(self.dir_mask), dev.ptr(self.counts), E,
                     st)
        call("gca_bulldozer_post", p, P - 1, dev.ptr(a), dev.ptr(self.steps), dev.ptr(self.parity),
             dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), H, W, dev.ptr(self.pos), dev.ptr(self.counts),
             dev.ptr(self.rng_step), dev.ptr(self.done), dev.ptr(self.hit), dev.ptr(self.reward), E, st)
        self.steps_elapsed += (self.steps >= 0).to(torch.int64)
        if self.autoreset:
            return self._autoreset()
        return self._obs(), self.reward, self._done_bool, self._truncated, self._info

    def ca_step_all(self, dir_mask=None):
        """One forced WindyForestFire step of every env (bench 'CA-only' mode, steps[E] = 1)."""
        E, H, W = self.num_envs, self.nrows, self.ncols
        st = dev.stream_ptr(self.device)
        call("gca_windy_step", dev.ptr(self.buf[0]), dev.ptr(self.buf[1]), dev.ptr(self.parity), None, 0,
             dev.ptr(self.dir_mask if dir_mask is None else dir_mask), E, H, W, self._empty, self._tree, self._fire,
             0, None, st)
        self.parity ^= 1
