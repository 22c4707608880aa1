#!/usr/bin/env python
"""An example, not a test: PPO on the Advanced (Alexandridis) bulldozer env, the env the reference's agent trains on
(agents/jax_ppo.py), with observation and network in one launch per step and the learner's update on the device.

    python scripts/train_advanced_ppo.py --envs 256 --iterations 20 [--graph]

Per iteration: env.rollout_policy(policy, K) collects K closed-loop steps of every env (per step: the fused
observe-and-act launch, the env's own step, the record rows, conditional_reset), env.policy_act gives the bootstrap
value of the state after it without side effects, forest_fire.ppo.gae turns rewards and values into advantages with
terminal = terminated (the reference never truncates), and BulldozerPolicy.ppo_update runs the whole update on the policy's five
tensors in place. --graph captures the rollout (K must be even: the env's current plane alternates per step) and one
update as two graphs and replays them; the draw is keyed by the env's time_step, which only grows, so a replayed rollout
draws new actions.

The defaults are the reference's PPOArgs (lr 2.5e-4, clip 0.1, 4 epochs x 4 minibatches, 128 steps) but for clip_vloss, which
is off unless --clip-vloss asks for the reference's clipped value loss. Without --extension the extension choice is not
the agent's (rollout_policy's `extension`). --extension trains the agent the reference trains: an ExtensionBulldozerPolicy
on an env with enable_extensions=True, whose third head picks the extension and which observes the displayed plane its
previous choice shaped; per iteration it also prints the reference's two rates (jax_ppo.py:524-538,
extensions/day_correct_rate): the share of day steps with extension 2 and the share of night steps with extension 1, from
the `action[..., 2]` and `is_night` records.
--retardant builds the policy with retardant=True: its observation then holds the env's dousing layer (the share of doused
cells per block and a flag per window cell), so the shoot head sees where it has doused, as the reference's agent does in
its RGB frame; without it the agent reads the grid alone. Needs a HIP device."""
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
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--cols", type=int, default=256)
    ap.add_argument("--steps", type=int, default=128, help="K: env steps per rollout")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--lr", type=float, default=2.5e-4)
    ap.add_argument("--clip", type=float, default=0.1)
    ap.add_argument("--ent-coef", type=float, default=0.01)
    ap.add_argument("--vf-coef", type=float, default=0.5)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--graph", action="store_true", help="capture the rollout and one update as graphs and replay them")
    ap.add_argument("--retardant", action="store_true", help="the policy sees the env's retardant (dousing) layer")
    ap.add_argument("--extension", action="store_true",
                    help="the three-headed agent on the displayed plane (enable_extensions=True); not with --retardant")
    ap.add_argument("--clip-vloss", action="store_true",
                    help="the reference's clipped value loss (args.ppo.clip_vloss, on by default THERE; off here)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("train_advanced_ppo.py needs a HIP device")
    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer import (AdvancedForestFireBulldozerEnv, BulldozerPolicy,
                                                 ExtensionBulldozerPolicy)
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    device = torch.device("cuda", 0)
    E, K = args.envs, args.steps
    T = K * E
    if T % args.minibatches:
        sys.exit("envs * steps must divide into the minibatches")
    if args.graph and K % 2:
        sys.exit("--graph needs an even number of steps")
    if args.extension and args.retardant:
        sys.exit("--extension and --retardant are not combined")
    env = AdvancedForestFireBulldozerEnv(args.rows, args.cols, key=1, num_envs=E, device=device, observation="grid",
                                         hidden_rng="philox", enable_extensions=args.extension)
    env.reset()
    if args.extension:
        policy = ExtensionBulldozerPolicy(env, radius=5, block=8, hidden=64, seed=0)
    else:
        policy = BulldozerPolicy(env, radius=5, block=8, hidden=64, seed=0, retardant=args.retardant)
    steps = args.epochs * args.minibatches
    opt = ppo.Adam(policy.state_dict(), lr=args.lr, anneal=(steps, args.iterations))
    N = T // args.minibatches
    hyper = dict(clip_coef=args.clip, ent_coef=args.ent_coef, vf_coef=args.vf_coef)
    # persistent buffers: the rollout and the update issue launches only
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=device)
    rec = {k: new(shape, dtype) for k, (dtype, shape) in env.policy_record_shapes(policy, K).items()}
    outs = {f"{k}_out": t for k, t in rec.items()}
    adv, ret = new((K, E)), new((K, E))
    bufs = dict(stats_out=new((steps, 8)), info_out=new((steps, 2)), perm_out=new((args.epochs, T), torch.int32),
                grads_out={n: torch.empty_like(getattr(policy, n)) for n in WEIGHTS},
                workspace=torch.empty_like(policy._ppo_workspace(N, None)))
    if args.clip_vloss:
        bufs.update(clip_vloss=True, vstats_out=new((steps, 3)))
    rollout = lambda seed: env.rollout_policy(policy, K, seed=seed, **outs)
    update = lambda: policy.ppo_update(opt, rec, adv, ret, epochs=args.epochs, minibatches=args.minibatches, seed=7,
                                       **hyper, **bufs)

    def capture(fn):
        torch.cuda.synchronize(device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g

    g_rollout = g_update = None
    for it in range(args.iterations):
        if not args.graph:
            rollout(it)
        elif it == 0:
            rollout(0)  # eager once: it warms the bound calls, and its records are iteration 0's
        else:
            if g_rollout is None:
                g_rollout = capture(lambda: rollout(0))
            g_rollout.replay()
        _, _, next_value = env.policy_act(policy, seed=it)
        ppo.gae(rec["reward"], rec["value"], next_value, args.gamma, args.gae_lambda, terminal=rec["terminated"],
                adv_out=adv, ret_out=ret)
        if not args.graph:
            update()
        else:
            if g_update is None:
                g_update = capture(update)
            g_update.replay()  # opt.count has moved since the last replay: new shuffles, the next learning rate
        s, info = bufs["stats_out"][-1].tolist(), bufs["info_out"][-1].tolist()  # the update's one sync
        print(f"iteration {it}: mean reward {rec['reward'].mean().item():+.5f}  "
              f"episodes ended {int(rec['terminated'].sum().item())}  "
              f"loss {s[0]:+.5f}  pg {s[1]:+.5f}  entropy {s[3]:.4f}  kl {s[4]:.2e}  clip {s[5]:.3f}  "
              f"grad norm {info[0]:.4f}  lr {info[1]:.3e}" +
              ("  U {:.4f}  u-share {:.3f}  v-clip {:.3f}".format(*bufs["vstats_out"][-1].tolist()) if args.clip_vloss
               else "") + (_extension_rates(rec) if args.extension else ""))


def _extension_rates(rec):
    """The reference's two rates on one rollout's records (torch ops, not a hot path): the share of day steps whose
    extension choice is 2 and the share of night steps whose choice is 1; n/a where the rollout has no such step."""
    choice, night = rec["action"][..., 2], rec["is_night"] != 0
    day_n, night_n = int((~night).sum().item()), int(night.sum().item())
    day = f"{int(((choice == 2) & ~night).sum().item()) / day_n:.3f}" if day_n else "n/a"
    ngt = f"{int(((choice == 1) & night).sum().item()) / night_n:.3f}" if night_n else "n/a"
    return f"  day ext-2 rate {day}  night ext-1 rate {ngt}"


if __name__ == "__main__":
    main()
