#!/usr/bin/env python
"""Batched ForestFireBulldozer env, K closed-loop steps under a BulldozerPolicy with autoreset: env.rollout_policy (ONE
launch of gca_bulldozer_policy_rollout: observation, network, both heads' draw, env step and reset inside the resident
rollout) against the ways an agent loop could be written without it. Prints one JSON line; --out also writes it.

    python scripts/bench_bulldozer_policy_rollout.py --out profiles/bulldozer_policy_rollout.json

Per shape (1024 x 256^2 and 1024 x 512^2; K = 128, radius 5, block 8, 64 hidden units, autoreset=True with
max_episode_steps=100 and staggered episode clocks), microseconds per env step of all E envs:
  a  rollout_policy          env.rollout_policy with every record (the observation records are the bulk of its stores:
                             K x E x (S*S + 4 C) bytes); rollout_policy_small: without the local / coarse records
  b  graph                   a captured graph of the 4 K launches observe, act, step, reset
  c  torch                   what a user of the library before this entry point writes: observe + the same MLP in torch
                             ops (BulldozerPolicy.forward_torch) + two torch.multinomial + step, eager
  d  rollout_actions         env.rollout(actions) on pre-decided actions: the floor without a policy
Every way starts from the same mid-episode state (reset + 64 random-policy steps, restored in place before its warm-up
call and before its timed calls); `rounds` rounds alternate the ways, the median is reported and every round's figure
kept in `*_rounds`. The claim under test is c against a: `torch_over_rollout_policy` is the ratio of the medians,
`torch_over_rollout_policy_worst` the slowest a against the fastest c, and `claim_holds` says whether even that exceeds
1, i.e. whether a beats c by more than the run-to-run spread. `graph_over_rollout_policy` (b against a) is reported,
not gated; `policy_us_per_step` is a - d. Needs a HIP device; there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ({"name": "1024x256x256", "E": 1024, "H": 256, "W": 256}, {"name": "1024x512x512", "E": 1024, "H": 512, "W": 512})
CONFIG = {"K": 128, "radius": 5, "block": 8, "hidden": 64}
LIMIT = 100  # max_episode_steps
SEED = 9     # the warm-up's random policy


def timed(fn, reps, prepare):
    """Mean microseconds per call over `reps` calls between two HIP events; `prepare` restores the starting state
    before one warm-up call and again before the timed calls."""
    import torch

    prepare()
    fn()
    prepare()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def snapshot(env):
    """Restore-in-place of every tensor attribute of the env (addresses stay: bound calls and graphs keep working)."""
    import torch

    saved = {k: v.clone() for k, v in vars(env).items() if isinstance(v, torch.Tensor)}

    def restore():
        for k, v in saved.items():
            getattr(env, k).copy_(v)

    return restore


def bench_shape(cfg, device, K, reps, rounds):
    import torch

    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv, BulldozerPolicy

    E, H, W = cfg["E"], cfg["H"], cfg["W"]
    r, B = CONFIG["radius"], CONFIG["block"]
    env = BatchedForestFireBulldozerEnv(E, H, W, device=device, seed=0x5EED, materialize_obs=False, autoreset=True,
                                        max_episode_steps=LIMIT)
    act1 = torch.zeros((E, 2), dtype=torch.int32, device=device)
    env.reset()
    for _ in range(64):  # the mid-episode state: reset + 64 steps of the random policy
        env.step_random(SEED, act1)
    env.steps_elapsed.copy_(torch.arange(E, device=device) % LIMIT)  # one env in a hundred is due on every step
    restore = snapshot(env)
    ep0 = int(env.episode.sum().item())
    pol = BulldozerPolicy(env, r, B, CONFIG["hidden"], seed=3)
    kw = dict(device=device)
    S = pol.S
    rec = {"action_out": torch.empty((K, E, 2), dtype=torch.int32, **kw),
           "logits_out": torch.empty((K, E, 11), dtype=torch.float32, **kw),
           "value_out": torch.empty((K, E), dtype=torch.float32, **kw),
           "reward_out": torch.empty((K, E), dtype=torch.float64, **kw),
           "terminated_out": torch.empty((K, E), dtype=torch.uint8, **kw),
           "truncated_out": torch.empty((K, E), dtype=torch.uint8, **kw),
           "local_out": torch.empty((K, E, S, S), dtype=torch.uint8, **kw),
           "coarse_out": torch.empty((K, E, 2, pol.Hc, pol.Wc), dtype=torch.float32, **kw)}
    small = {k: v for k, v in rec.items() if k not in ("local_out", "coarse_out")}
    lo = torch.empty((E, S, S), dtype=torch.uint8, **kw)
    co = torch.empty((E, 2, pol.Hc, pol.Wc), dtype=torch.float32, **kw)
    act = torch.empty((E, 2), dtype=torch.int32, **kw)
    lg = torch.empty((E, 11), dtype=torch.float32, **kw)
    va = torch.empty(E, dtype=torch.float32, **kw)
    gen = torch.Generator(device="cpu").manual_seed(K)
    actions = torch.stack([torch.randint(0, 9, (K, E), generator=gen, dtype=torch.int32),
                           torch.randint(0, 2, (K, E), generator=gen, dtype=torch.int32)], dim=2).to(device)

    def k_launches():
        for _ in range(K):
            env.observe(r, B, lo, co)
            env.act(pol, lo, co, seed=5, action_out=act, logits_out=lg, value_out=va)
            env.step(act)

    def k_torch():
        with torch.no_grad():
            for _ in range(K):
                env.observe(r, B, lo, co)
                move, shoot, _ = pol.forward_torch(lo, co)
                a = torch.cat([torch.multinomial(torch.softmax(move, -1), 1),
                               torch.multinomial(torch.softmax(shoot, -1), 1)], 1).to(torch.int32)
                env.step(a)

    restore()
    k_launches()  # warm the bound calls before the capture, which itself runs nothing
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        k_launches()
    fns = {"rollout_policy": lambda: env.rollout_policy(pol, K, seed=5, **rec),
           "rollout_policy_small": lambda: env.rollout_policy(pol, K, seed=5, record=(), **small),
           "graph": graph.replay,
           "torch": k_torch,
           "rollout_actions": lambda: env.rollout(actions, reward_out=rec["reward_out"],
                                                  terminated_out=rec["terminated_out"],
                                                  truncated_out=rec["truncated_out"])}
    runs = {w: [] for w in fns}
    extra = {}
    for _ in range(rounds):
        for w, fn in fns.items():
            runs[w].append(timed(fn, reps, restore) / K)
            extra[w] = {"done_after": int(env.done.sum().item()),
                        "resets_per_step": (int(env.episode.sum().item()) - ep0) / (reps * K)}
    out = {"name": cfg["name"], "E": E, "H": H, "W": W, "C": pol.C, "fused": bool(env.fused)}
    for w, v in runs.items():
        out[f"{w}_us"] = statistics.median(v)
        out[f"{w}_rounds"] = v
        out[f"{w}_state"] = extra[w]
    a, a_s = out["rollout_policy_us"], out["rollout_policy_small_us"]
    out["torch_over_rollout_policy"] = out["torch_us"] / a
    out["torch_over_rollout_policy_worst"] = min(runs["torch"]) / max(runs["rollout_policy"])
    out["claim_holds"] = bool(out["torch_over_rollout_policy_worst"] > 1.0)
    out["graph_over_rollout_policy"] = out["graph_us"] / a
    out["graph_over_rollout_policy_small"] = out["graph_us"] / a_s
    out["policy_us_per_step"] = a - out["rollout_actions_us"]
    out["policy_small_us_per_step"] = a_s - out["rollout_actions_us"]
    out["env_steps_per_second_rollout_policy"] = E / (a * 1e-6)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=2, help="timed repetitions of K env steps per round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds that alternate the ways (>= 5); the median is reported")
    ap.add_argument("--steps", type=int, default=CONFIG["K"])
    ap.add_argument("--shapes", default=",".join(s["name"] for s in SHAPES))
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.reps < 1 or args.rounds < 5 or args.steps < 1:
        sys.exit("bench_bulldozer_policy_rollout.py: --reps and --steps must be >= 1, --rounds >= 5")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_bulldozer_policy_rollout.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    device = torch.device("cuda", 0)
    shapes = [s for s in SHAPES if s["name"] in args.shapes.split(",")]
    res = {"bench": "bulldozer_policy_rollout", "device": torch.cuda.get_device_name(0), **CONFIG, "K": args.steps,
           "max_episode_steps": LIMIT, "reps": args.reps, "rounds": args.rounds,
           "timing": "HIP events around `reps` repetitions of K env steps from one restored mid-episode state, mean us "
                     "per env step of all E envs; median over alternating rounds",
           "shapes": [bench_shape(c, device, args.steps, args.reps, args.rounds) for c in shapes]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
