#!/usr/bin/env python
"""An example, not a test: PPO on the batched ForestFireBulldozer env with the agent inside the env's launch and the
learner's update on the device.

    python scripts/train_bulldozer_ppo.py --envs 256 --iterations 20 [--graph | --autograd]

Per iteration: env.rollout_policy(policy, K) collects K closed-loop steps of every env (one launch where the shape
allows, autoreset included), env.act gives the bootstrap value of the state after it without side effects,
forest_fire.ppo.gae turns rewards and values into advantages with terminal = terminated | truncated (nothing is
bootstrapped across an episode's end), and BulldozerPolicy.ppo_update runs the whole update: one permutation launch,
then per minibatch ppo_grad (the clipped-surrogate loss per head, include/gca.h gca_bulldozer_policy_grad, in four
launches) and forest_fire.ppo.Adam.step on the policy's five tensors in place, so the env's bound calls keep their
addresses. --graph captures one update as a graph and replays it. --autograd keeps the former loop for comparison: the
same loss through BulldozerPolicy.forward_torch and autograd, all five tensors cloned as leaves per minibatch.

The loss is the reference's, per head (agents/jax_ppo.py:902-930, :987-1041): a ratio, a clipped term and an entropy
per head, every mean over the (sample, head) pairs. Earlier versions of this script used a joint ratio, the sum of both
heads' log-probabilities; that was a stand-in until the library had the two-head gradient.
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
    ap.add_argument("--graph", action="store_true", help="capture one update as a graph and replay it")
    ap.add_argument("--autograd", action="store_true", help="the former loop: the per-head loss through autograd")
    ap.add_argument("--clip-vloss", action="store_true",
                    help="the reference's clipped value loss (args.ppo.clip_vloss, on by default THERE; off here)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("train_bulldozer_ppo.py needs a HIP device")
    if args.graph and args.autograd:
        sys.exit("train_bulldozer_ppo.py: --graph captures the device update; it does not go with --autograd")
    if args.clip_vloss and args.autograd:
        sys.exit("train_bulldozer_ppo.py: --clip-vloss is the device update's; it does not go with --autograd")
    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv, BulldozerPolicy
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    device = torch.device("cuda", 0)
    E, K = args.envs, args.steps
    env = BatchedForestFireBulldozerEnv(E, args.rows, args.cols, device=device, seed=1, materialize_obs=False,
                                        autoreset=True, max_episode_steps=args.max_episode_steps)
    env.reset()
    policy = BulldozerPolicy(env, radius=5, block=8, hidden=64, seed=0)
    steps = args.epochs * args.minibatches
    opt = ppo.Adam(policy.state_dict(), lr=args.lr, anneal=(steps, args.iterations))
    T = K * E
    if T % args.minibatches:
        sys.exit("envs * steps must divide into the minibatches")
    N = T // args.minibatches
    hyper = dict(clip_coef=args.clip, ent_coef=args.ent_coef, vf_coef=args.vf_coef)
    # persistent buffers: the update allocates nothing
    adv, ret = torch.empty((K, E), device=device), torch.empty((K, E), device=device)
    bufs = dict(stats_out=torch.empty((steps, 8), device=device), info_out=torch.empty((steps, 2), device=device),
                perm_out=torch.empty((args.epochs, T), dtype=torch.int32, device=device),
                grads_out={n: torch.empty_like(getattr(policy, n)) for n in WEIGHTS},
                workspace=torch.empty_like(policy._ppo_workspace(N, None)))
    records = ("local", "coarse", "action", "logits")
    if args.clip_vloss:
        bufs.update(clip_vloss=True, vstats_out=torch.empty((steps, 3), device=device))
        records += ("value",)

    def autograd_update(rec):
        """The former loop: per minibatch the per-head loss through forward_torch, backward, Adam.step."""
        flat = lambda t: t.reshape((T,) + tuple(t.shape[2:]))
        local, coarse, action, old, a_all, r_all = (flat(t) for t in (rec["local"], rec["coarse"], rec["action"],
                                                                      rec["logits"], adv, ret))
        perm = ppo.permutation(T, args.epochs, seed=7, counter=opt.count, out=bufs["perm_out"]).long()
        for epoch in range(args.epochs):
            for mb in range(args.minibatches):
                i = epoch * args.minibatches + mb
                idx = perm[epoch, mb * N:(mb + 1) * N]
                leaves = {n: getattr(policy, n).clone().requires_grad_(True) for n in WEIGHTS}
                move, shoot, value = policy.forward_torch(local[idx], coarse[idx], weights=leaves)
                logratio, ent = [], []
                for h, (new, prev) in enumerate(((move, old[idx, :9]), (shoot, old[idx, 9:]))):
                    lp, lo = torch.log_softmax(new, -1), torch.log_softmax(prev, -1)
                    act = action[idx, h].long().unsqueeze(-1)
                    logratio.append((lp.gather(-1, act) - lo.gather(-1, act)).squeeze(-1))
                    ent.append(-(lp.exp() * lp).sum(-1))
                logratio, ent = torch.stack(logratio, 1), torch.stack(ent, 1)  # (N, heads): nothing summed over heads
                ratio = logratio.exp()
                a = a_all[idx]
                a = ((a - a.mean()) / (a.std(unbiased=False) + 1e-8)).unsqueeze(1)
                pg = torch.maximum(-a * ratio, -a * ratio.clamp(1 - args.clip, 1 + args.clip)).mean()
                v_loss = 0.5 * (value - r_all[idx]).pow(2).mean()
                loss = pg - args.ent_coef * ent.mean() + args.vf_coef * v_loss
                loss.backward()
                opt.step({n: leaves[n].grad.contiguous() for n in WEIGHTS}, info_out=bufs["info_out"][i])
                with torch.no_grad():
                    clipped = ((ratio < 1 - args.clip) | (ratio > 1 + args.clip)).float().mean()
                    bufs["stats_out"][i] = torch.stack([loss, pg, v_loss, ent.mean(), ((ratio - 1) - logratio).mean(),
                                                        clipped, a_all[idx].mean(), a_all[idx].std(unbiased=False)])

    graph = rec0 = None
    for it in range(args.iterations):
        rec = env.rollout_policy(policy, K, seed=it)
        _, _, next_value = env.act(policy, seed=it)
        terminal = rec["terminated"] | rec["truncated"]
        ppo.gae(rec["reward"], rec["value"], next_value, terminal=terminal, adv_out=adv, ret_out=ret)
        run = lambda r: policy.ppo_update(opt, r, adv, ret, epochs=args.epochs, minibatches=args.minibatches, seed=7,
                                          **hyper, **bufs)
        if args.autograd:
            autograd_update(rec)
        elif not args.graph:
            run(rec)
        else:
            if graph is None:
                # the graph reads the records at fixed addresses: the first rollout's tensors, refilled every iteration
                rec0 = {k: rec[k] for k in records}
                torch.cuda.synchronize(device)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    run(rec0)
            else:
                for k, t in rec0.items():
                    t.copy_(rec[k])
            graph.replay()  # opt.count has moved since the last replay: new shuffles, the next learning rate
        s, info = bufs["stats_out"][-1].tolist(), bufs["info_out"][-1].tolist()  # the update's one sync
        print(f"iteration {it}: mean reward {rec['reward'].mean().item():+.5f}  "
              f"episodes ended {int(terminal.sum().item())}  terminated {int(rec['terminated'].sum().item())}  "
              f"loss {s[0]:+.5f}  pg {s[1]:+.5f}  entropy {s[3]:.4f}  kl {s[4]:.2e}  clip {s[5]:.3f}  "
              f"grad norm {info[0]:.4f}  lr {info[1]:.3e}" +
              ("  U {:.4f}  u-share {:.3f}  v-clip {:.3f}".format(*bufs["vstats_out"][-1].tolist()) if args.clip_vloss
               else ""))


if __name__ == "__main__":
    main()
