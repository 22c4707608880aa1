"""BulldozerPolicy — the two-headed policy network the batched bulldozer env evaluates inside its own launches.

The helicopter policy's two-layer MLP over observe(radius, block)'s tensors (include/gca.h "bulldozer policy") with twelve
outputs: nine move logits, two shoot logits (the reference's Actor(action_dims=[9, 2])) and the value. env.act(policy)
is one launch on an observation; env.rollout_policy(policy, K) collects K closed-loop steps of every env, autoreset
included, bit for bit K x (observe, act, step [, reset]) and in one launch where the shape allows. forward_torch is the
same network in differentiable torch ops. ppo_grad is the learner's step on rollout_policy's records: the PPO
clipped-surrogate loss taken per head (include/gca.h gca_bulldozer_policy_grad: the reference's ppo_loss, every mean over
the (sample, head) pairs), its statistics and its gradient with respect to the five tensors in four launches, with
forest_fire.ppo.gae for the advantages; ppo_update is the whole update (scripts/train_bulldozer_ppo.py).

The bookkeeping (validated assignment of the five tensors, `version`, the C struct, load) and ppo_grad / ppo_update are
PolicyBase's (_policy.py), shared with HelicopterPolicy; a record's `action` holds T x 2 int32 values (move, shoot) and
its `logits` T x 11 float32 values.
"""
from .._policy import WEIGHTS, PolicyBase  # WEIGHTS: the trainers import it from here

N_MOVE = 9
N_SHOOT = 2
N_LOGITS = N_MOVE + N_SHOOT
N_OUT = N_LOGITS + 1  # the logits and the value


class BulldozerPolicy(PolicyBase):
    HEADS = (N_MOVE, N_SHOOT)
    N_LOGITS = N_LOGITS
    GRAD_ENTRY = "gca_bulldozer_policy_grad"

    def __init__(self, env_or_shape, radius=5, block=8, hidden=64, seed=0, device=None, retardant=False):
        """retardant=True: the policy of the Advanced env that sees the env's retardant. Its coarse part is the feature
        vector of AdvancedForestFireBulldozerEnv.observe(radius, block, retardant=True) (include/gca.h
        gca_advanced_policy_observation): C = C2 = 3 Hc Wc + S*S rounded up to even -- the coarse map, the retardant
        share of every block, the window's retardant flags -- and w_coarse is (C2, hidden). Everything else, the learner
        included, goes through `C` unchanged. With False nothing differs, down to the drawn weights."""
        self.retardant = bool(retardant)
        super().__init__(env_or_shape, radius, block, hidden, seed, device)

    def _coarse_len(self):
        if not self.retardant:
            return super()._coarse_len()
        return (3 * self.Hc * self.Wc + self.S * self.S + 1) & ~1

    def forward_torch(self, local, coarse, weights=None):
        """(move_logits (..., 9), shoot_logits (..., 2), value (...)) of the same network in differentiable torch ops: an
        embedding gather over the window's classes, a sum, and two matmuls. local (..., S, S) uint8, coarse
        (..., 2, Hc, Wc) float32 -- (..., C2) for a retardant policy -- with the same leading dims (for instance the
        (K, E) of rollout_policy's records).
        weights: a dict of the five tensors to use instead of the policy's own (a trainer's leaf tensors, which then
        receive the gradients). The summation order is torch's, not the kernels': the results agree within rounding, not
        bit for bit."""
        out, lead = self._forward_torch(local, coarse, weights)
        return (out[:, :N_MOVE].reshape(lead + (N_MOVE,)), out[:, N_MOVE:N_LOGITS].reshape(lead + (N_SHOOT,)),
                out[:, N_LOGITS].reshape(lead))


N_EXTENSION = 3


class ExtensionBulldozerPolicy(BulldozerPolicy):
    """The three-headed agent the reference trains on the Advanced bulldozer env (Actor(action_dims=[9, 2],
    choose_k=[(2, 1)]), agents/jax_ppo.py:305-356, 708-710): the bulldozer policy's network with fifteen outputs -- nine
    move logits, two shoot logits, three extension logits and the value (include/gca.h "extension policy"). On an
    AdvancedForestFireBulldozerEnv(enable_extensions=True) it observes the DISPLAYED plane (env.display(): the blurred,
    visibility-filtered grid, or the extension channel its own previous choice switched on), not the true grid, and its
    third action column is the env's extension choice. A record's `action` holds T x 3 int32 values and its `logits`
    T x 14 float32 values; ppo_grad / ppo_update are PolicyBase's over gca_extension_policy_grad, every mean over the
    (sample, head) pairs of three heads. The retardant observation cannot be combined with the display yet."""
    HEADS = (N_MOVE, N_SHOOT, N_EXTENSION)
    N_LOGITS = N_MOVE + N_SHOOT + N_EXTENSION
    GRAD_ENTRY = "gca_extension_policy_grad"

    def __init__(self, env_or_shape, radius=5, block=8, hidden=64, seed=0, device=None, retardant=False):
        if retardant:
            raise ValueError("ExtensionBulldozerPolicy: retardant=True is not supported (the retardant observation and "
                             "the displayed plane are not combined in one observation)")
        super().__init__(env_or_shape, radius, block, hidden, seed, device)

    def forward_torch(self, local, coarse, weights=None):
        """(move_logits (..., 9), shoot_logits (..., 2), extension_logits (..., 3), value (...)) of the same network in
        differentiable torch ops; see BulldozerPolicy.forward_torch."""
        out, lead = self._forward_torch(local, coarse, weights)
        a, b, c = N_MOVE, N_MOVE + N_SHOOT, self.N_LOGITS
        return (out[:, :a].reshape(lead + (N_MOVE,)), out[:, a:b].reshape(lead + (N_SHOOT,)),
                out[:, b:c].reshape(lead + (N_EXTENSION,)), out[:, c].reshape(lead))
