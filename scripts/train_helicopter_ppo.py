#!/usr/bin/env python
"""PPO on the batched helicopter env, the whole loop on the public surface and on the device: env.rollout_policy collects
K steps of every env in one launch, env.act gives the bootstrap value, forest_fire.ppo.gae the advantages, and
HelicopterPolicy.ppo_update runs the update: one forest_fire.ppo.permutation launch shuffles the samples for all epochs,
then every minibatch goes through ppo_grad (loss, statistics and the five gradients in four launches) and
forest_fire.ppo.Adam.step (global-norm clip and Adam in two launches, the step count on the device). The optimizer is
the reference's: clip_by_global_norm(--max-grad-norm), adam(eps=1e-5), and with --anneal its linear learning-rate
schedule. With --graph the update is captured once and replayed: sixteen minibatches in one graph launch. The only sync
of an update is its print. An example, not a test.

    python scripts/train_helicopter_ppo.py --updates 20 --anneal --graph
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=64, help="K: env steps per update")
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=2.5e-4)
    ap.add_argument("--max-grad-norm", type=float, default=0.5, help="global-norm clip; 0 turns it off")
    ap.add_argument("--anneal", action="store_true", help="the reference's linear schedule over --updates")
    ap.add_argument("--graph", action="store_true", help="capture one update as a graph and replay it")
    ap.add_argument("--clip-vloss", action="store_true",
                    help="the reference's clipped value loss (args.ppo.clip_vloss, on by default THERE; off here)")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("train_helicopter_ppo.py needs a HIP device (no CPU fallback)")
    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv, HelicopterPolicy
    from gymca_amd.forest_fire.helicopter.policy import WEIGHTS

    device = torch.device("cuda", 0)
    E, K = args.envs, args.steps
    T = E * K
    steps = args.epochs * args.minibatches
    env = BatchedForestFireHelicopterEnv(E, 42, 42, device=device, seed=args.seed, materialize_obs=False)
    env.reset()
    pol = HelicopterPolicy(env, radius=5, block=8, hidden=64, seed=args.seed)
    opt = ppo.Adam({n: getattr(pol, n) for n in WEIGHTS}, lr=args.lr, max_grad_norm=args.max_grad_norm,
                   anneal=(steps, args.updates) if args.anneal else None)
    # persistent buffers: the update allocates nothing
    adv, ret = torch.empty((K, E), device=device), torch.empty((K, E), device=device)
    bufs = dict(stats_out=torch.empty((steps, 8), device=device), info_out=torch.empty((steps, 2), device=device),
                perm_out=torch.empty((args.epochs, T), dtype=torch.int32, device=device),
                grads_out={n: torch.empty_like(getattr(pol, n)) for n in WEIGHTS},
                workspace=torch.empty_like(pol._ppo_workspace(T // args.minibatches, None)))
    records = ("local", "coarse", "action", "logits")
    if args.clip_vloss:
        bufs.update(clip_vloss=True, vstats_out=torch.empty((steps, 3), device=device))
        records += ("value",)
    graph = rec0 = None
    for update in range(args.updates):
        rec = env.rollout_policy(pol, K, seed=args.seed + update)
        _, _, next_value = env.act(pol, seed=args.seed + update)
        ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95, adv_out=adv, ret_out=ret)
        run = lambda r: pol.ppo_update(opt, r, adv, ret, epochs=args.epochs, minibatches=args.minibatches,
                                       seed=args.seed, **bufs)
        if not args.graph:
            run(rec)
        else:
            if graph is None:
                # the graph reads the records at fixed addresses: the first rollout's tensors, refilled every update
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
        print(f"update {update:3d}  mean reward {rec['reward'].mean().item():+.4f}  loss {s[0]:+.4f}  "
              f"pg {s[1]:+.5f}  v {s[2]:.4f}  entropy {s[3]:.4f}  kl {s[4]:.2e}  clip {s[5]:.3f}  "
              f"|g| {info[0]:.3f}  lr {info[1]:.2e}" +
              ("  U {:.4f}  u-share {:.3f}  v-clip {:.3f}".format(*bufs["vstats_out"][-1].tolist()) if args.clip_vloss
               else ""))


if __name__ == "__main__":
    main()
