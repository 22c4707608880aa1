"""HelicopterPolicy — the small policy network the batched helicopter env evaluates inside its own launches.

A two-layer MLP over observe(radius, block)'s tensors (include/gca.h "helicopter policy"): the window's classes select
rows of `w_local` (a Dense layer over the one-hot classes, done as a lookup), the coarse map goes through `w_coarse`, a
relu hidden layer of width `hidden`, then ten outputs: nine action logits and the value. env.act(policy) is one launch
on an observation; env.rollout_policy(policy, K) collects K closed-loop steps of every env in one launch, bit for bit
K x (observe, act, step). forward_torch is the same network in differentiable torch ops. ppo_grad is the learner's step
on rollout_policy's records: the PPO clipped-surrogate loss, its statistics and its gradient with respect to the five
tensors in four launches (gca_helicopter_policy_grad), with forest_fire.ppo.gae for the advantages. ppo_update is the
whole update: forest_fire.ppo.permutation's shuffles, then ppo_grad and forest_fire.ppo.Adam.step per minibatch.
"""
from .._policy import WEIGHTS, PolicyBase  # WEIGHTS: importers of this module find it here

N_ACTIONS = 9
N_OUT = 10  # the logits and the value


class HelicopterPolicy(PolicyBase):
    """The dims, the five tensors, `version`, the C struct, load and the learner's step (ppo_grad, ppo_update) are
    PolicyBase's (_policy.py); here are the head, the entry point and forward_torch."""

    HEADS = (N_ACTIONS,)
    N_LOGITS = N_ACTIONS
    GRAD_ENTRY = "gca_helicopter_policy_grad"

    def forward_torch(self, local, coarse, weights=None):
        """(logits (..., 9), value (...)) of the same network in differentiable torch ops: an embedding gather over the
        window's classes, a sum, and two matmuls. local (..., S, S) uint8, coarse (..., 2, Hc, Wc) float32 with the same
        leading dims (for instance the (K, E) of rollout_policy's records). weights: a dict of the five tensors to use
        instead of the policy's own (a trainer's leaf tensors, which then receive the gradients). The summation order is
        torch's, not the kernels': the results agree within rounding, not bit for bit."""
        out, lead = self._forward_torch(local, coarse, weights)
        return out[:, :N_ACTIONS].reshape(lead + (N_ACTIONS,)), out[:, N_ACTIONS].reshape(lead)
