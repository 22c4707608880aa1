#!/usr/bin/env python
"""An example, not a test: PPO on the batched ForestFireBulldozer env with the agent inside the env's launch.

    python scripts/train_bulldozer_ppo.py --envs 256 --iterations 20

Per iteration: env.rollout_policy(policy, K) collects K closed-loop steps of every env (one launch where the shape
allows, autoreset included), env.act gives the bootstrap value of the state after it without side effects,
forest_fire.ppo.gae turns rewards and values into advantages with terminal = terminated | truncated (nothing is
bootstrapped across an episode's end), and the clipped-surrogate loss over both heads is taken through
BulldozerPolicy.forward_torch and autograd; forest_fire.ppo.Adam.step applies the reference's clipped, annealed
optimizer to the policy's five tensors in place, so the env's bound calls keep their addresses. (The two-head loss
gradient as a device kernel is not in the library yet; the helicopter's ppo_grad shows what it will look like.)
Needs a HIP device."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--cols", type=int, default=256)
    ap.add_argument("--steps", type=int, default=64, help="K: env steps per rollout")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--max-episode-steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=2.5e-4)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--ent-coef", type=float, default=0.01)
    ap.add_argument("--vf-coef", type=float, default=0.5)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("train_bulldozer_ppo.py needs a HIP device")
    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv, BulldozerPolicy
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    device = torch.device("cuda", 0)
    E, K = args.envs, args.steps
    env = BatchedForestFireBulldozerEnv(E, args.rows, args.cols, device=device, seed=1, materialize_obs=False,
                                        autoreset=True, max_episode_steps=args.max_episode_steps)
    env.reset()
    policy = BulldozerPolicy(env, radius=5, block=8, hidden=64, seed=0)
    steps_per_iteration = args.epochs * args.minibatches
    opt = ppo.Adam(policy.state_dict(), lr=args.lr, anneal=(steps_per_iteration, args.iterations))
    T = K * E
    if T % args.minibatches:
        sys.exit("envs * steps must divide into the minibatches")
    N = T // args.minibatches

    def logp_and_entropy(logits, action):
        lp = torch.log_softmax(logits, -1)
        return lp.gather(-1, action.long().unsqueeze(-1)).squeeze(-1), -(lp.exp() * lp).sum(-1)

    for it in range(args.iterations):
        rec = env.rollout_policy(policy, K, seed=it)
        _, _, next_value = env.act(policy, seed=it)
        terminal = rec["terminated"] | rec["truncated"]
        adv, ret = ppo.gae(rec["reward"], rec["value"], next_value, terminal=terminal)
        flat = lambda t: t.reshape((T,) + tuple(t.shape[2:]))
        local, coarse, action, adv, ret = (flat(t) for t in (rec["local"], rec["coarse"], rec["action"], adv, ret))
        old_logits = flat(rec["logits"])
        with torch.no_grad():
            lm, _ = logp_and_entropy(old_logits[:, :9], action[:, 0])
            ls, _ = logp_and_entropy(old_logits[:, 9:], action[:, 1])
            old_logp = lm + ls
        perm = ppo.permutation(T, args.epochs, seed=7, counter=opt.count).long()
        for epoch in range(args.epochs):
            for mb in range(args.minibatches):
                idx = perm[epoch, mb * N:(mb + 1) * N]
                leaves = {n: getattr(policy, n).clone().requires_grad_(True) for n in WEIGHTS}
                move, shoot, value = policy.forward_torch(local[idx], coarse[idx], weights=leaves)
                lpm, ent_m = logp_and_entropy(move, action[idx, 0])
                lps, ent_s = logp_and_entropy(shoot, action[idx, 1])
                ratio = (lpm + lps - old_logp[idx]).exp()
                a = adv[idx]
                a = (a - a.mean()) / (a.std(unbiased=False) + 1e-8)
                pg = torch.maximum(-a * ratio, -a * ratio.clamp(1 - args.clip, 1 + args.clip)).mean()
                v_loss = 0.5 * (value - ret[idx]).pow(2).mean()
                entropy = (ent_m + ent_s).mean()
                loss = pg - args.ent_coef * entropy + args.vf_coef * v_loss
                loss.backward()
                info = opt.step({n: leaves[n].grad.contiguous() for n in WEIGHTS})  # the policy's tensors, in place
        ended = int(terminal.sum().item())
        print(f"iteration {it}: mean reward {rec['reward'].mean().item():+.5f}  episodes ended {ended}  "
              f"terminated {int(rec['terminated'].sum().item())}  loss {loss.item():+.5f}  "
              f"entropy {entropy.item():.4f}  grad norm {info[0].item():.4f}  lr {info[1].item():.3e}")


if __name__ == "__main__":
    main()
