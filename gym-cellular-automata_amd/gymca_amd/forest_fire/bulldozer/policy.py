"""BulldozerPolicy — the two-headed policy network the batched bulldozer env evaluates inside its own launches.

The helicopter policy's two-layer MLP over observe(radius, block)'s tensors (include/gca.h "bulldozer policy") with twelve
outputs: nine move logits, two shoot logits (the reference's Actor(action_dims=[9, 2])) and the value. env.act(policy)
is one launch on an observation; env.rollout_policy(policy, K) collects K closed-loop steps of every env, autoreset
included, bit for bit K x (observe, act, step [, reset]) and in one launch where the shape allows. forward_torch is the
same network in differentiable torch ops, for a learner that takes the loss through autograd
(scripts/train_bulldozer_ppo.py); the two-head loss gradient on the device is not part of this class yet.

The bookkeeping (validated assignment of the five tensors, `version`, the C struct, load) is PolicyBase's (_policy.py),
shared with HelicopterPolicy.
"""
from .._policy import WEIGHTS, PolicyBase  # WEIGHTS: the trainers import it from here

N_MOVE = 9
N_SHOOT = 2
N_LOGITS = N_MOVE + N_SHOOT
N_OUT = N_LOGITS + 1  # the logits and the value


class BulldozerPolicy(PolicyBase):
    N_LOGITS = N_LOGITS

    def forward_torch(self, local, coarse, weights=None):
        """(move_logits (..., 9), shoot_logits (..., 2), value (...)) of the same network in differentiable torch ops: an
        embedding gather over the window's classes, a sum, and two matmuls. local (..., S, S) uint8, coarse
        (..., 2, Hc, Wc) float32 with the same leading dims (for instance the (K, E) of rollout_policy's records).
        weights: a dict of the five tensors to use instead of the policy's own (a trainer's leaf tensors, which then
        receive the gradients). The summation order is torch's, not the kernels': the results agree within rounding, not
        bit for bit."""
        out, lead = self._forward_torch(local, coarse, weights)
        return (out[:, :N_MOVE].reshape(lead + (N_MOVE,)), out[:, N_MOVE:N_LOGITS].reshape(lead + (N_SHOOT,)),
                out[:, N_LOGITS].reshape(lead))
