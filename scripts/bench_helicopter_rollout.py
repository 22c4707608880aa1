#!/usr/bin/env python
"""Batched ForestFireHelicopter env, K env steps with the caller's actions: env.rollout(actions) (one launch of
gca_helicopter_rollout, the grid resident in LDS) against K eager env.step(actions[k]) calls and against a captured
graph of those K step calls, timed in the same run with HIP events. Prints one JSON line; --out also writes it.

    python scripts/bench_helicopter_rollout.py --reps 100 --warmup 3 --out profiles/helicopter_rollout.json

The three ways start from the same reset and take the same actions for the same number of steps, so they do the same
work (their final cell counts are compared: `same_counts`). Per shape and K: microseconds per env step of all E envs
(`*_us`), env-steps per second (`*_sps`, E envs x steps), and the ratios `eager_over_rollout` / `graph_over_rollout`
(> 1: the rollout is faster). Needs a HIP device; there is no CPU fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = (
    {"name": "4096x42x42_default_freeze", "E": 4096, "H": 42, "W": 42, "freeze": None, "judged": True},
    {"name": "4096x42x42_freeze0", "E": 4096, "H": 42, "W": 42, "freeze": 0, "judged": True},
    {"name": "4096x64x64_freeze0", "E": 4096, "H": 64, "W": 64, "freeze": 0, "judged": True},
    {"name": "256x42x42_default_freeze", "E": 256, "H": 42, "W": 42, "freeze": None, "judged": False},
)
KS = (32, 128)


def timed(fn, reps, warmup):
    """Mean microseconds per call over `reps` calls between two HIP events, after `warmup` calls."""
    import torch

    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def bench_case(cfg, K, device, reps, warmup):
    import torch

    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv

    E, H, W = cfg["E"], cfg["H"], cfg["W"]

    def make():
        env = BatchedForestFireHelicopterEnv(E, H, W, device=device, seed=1, freeze=cfg["freeze"],
                                             materialize_obs=False)
        env.reset()
        return env

    gen = torch.Generator(device="cpu").manual_seed(K)
    actions = torch.randint(0, 9, (K, E), generator=gen, dtype=torch.int32).to(device)
    rows = [actions[k] for k in range(K)]  # contiguous int32 (E,) views: step uses them as they are
    rew_o = torch.empty((K, E), dtype=torch.float64, device=device)
    hit_o = torch.empty((K, E), dtype=torch.uint8, device=device)

    roll, eager, graphed = make(), make(), make()

    def k_steps(env):
        for a in rows:
            env.step(a)

    out = {"K": K, "max_freeze": roll.max_freeze}
    us = {}
    us["rollout"] = timed(lambda: roll.rollout(actions, reward_out=rew_o, hit_out=hit_o), reps, warmup)
    us["eager"] = timed(lambda: k_steps(eager), reps, warmup)
    k_steps(graphed)  # the first of the warm-up runs, eager; the capture itself runs nothing
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        k_steps(graphed)
    us["graph"] = timed(graph.replay, reps, warmup - 1)
    torch.cuda.synchronize(device)
    out["same_counts"] = bool(torch.equal(roll.counts, eager.counts) and torch.equal(roll.counts, graphed.counts)
                              and torch.equal(roll.steps_elapsed, graphed.steps_elapsed))
    for name, v in us.items():
        out[f"{name}_us"] = v / K
        out[f"{name}_sps"] = E * K / (v * 1e-6)
    out["eager_over_rollout"] = us["eager"] / us["rollout"]
    out["graph_over_rollout"] = us["graph"] / us["rollout"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=100, help="timed repetitions of K env steps")
    ap.add_argument("--warmup", type=int, default=3, help="untimed repetitions before them (>= 1)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.warmup < 1 or args.reps < 1:
        sys.exit("bench_helicopter_rollout.py: --reps and --warmup must be >= 1")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_helicopter_rollout.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    device = torch.device("cuda", 0)
    shapes = []
    for cfg in SHAPES:
        cases = [bench_case(cfg, K, device, args.reps, args.warmup) for K in KS]
        row = {"name": cfg["name"], "E": cfg["E"], "H": cfg["H"], "W": cfg["W"], "judged": cfg["judged"],
               "cases": cases}
        if cfg["judged"]:
            row["rollout_not_slower_than_eager"] = all(c["eager_over_rollout"] >= 1.0 for c in cases)
        shapes.append(row)
    res = {"bench": "helicopter_rollout", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "warmup": args.warmup,
           "timing": "HIP events around `reps` repetitions of K env steps, mean us per env step of all E envs",
           "shapes": shapes}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
