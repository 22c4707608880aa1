#!/usr/bin/env python
"""What it costs the bulldozer agent on the Advanced (Alexandridis) bulldozer env to see the retardant: observe-and-act in
one launch with the dousing layer in the observation (gca_advanced_policy_act_retardant) against the two launches it is
defined by and against the launch of the agent that reads the grid alone. Prints one JSON line; --out also writes it.

    python scripts/bench_advanced_policy_retardant.py --out profiles/advanced_policy_retardant.json

The method is scripts/bench_advanced_policy.py's (its state, its timing, its rounds). Per shape (4096 x 256^2 and
1024 x 512^2; radius 5, block 8, 64 hidden units, observation="grid", use_hidden=False, bench.py's mid-episode state plus
a dousing layer with one cell in twenty doused), in microseconds per call of all E envs:
  fused_bits          (a) env.policy_act(retardant policy): one launch, the retardant from the env's dousing bits
  fused_bits_records  the same with local_out / coarse_out, as rollout_policy calls it
  fused_u8            (b) the same launch from the u8 layer (dous_bits = NULL, as an env without the packed layout
                      passes it)
  pair                (c) env.policy_act(retardant policy, fused=False): gca_advanced_policy_observation,
                      time_step.to(int64), gca_bulldozer_policy_act; it writes local / feat by construction
  parent              (d) env.policy_act(a policy without the keyword) on the same state: gca_advanced_policy_act
No way changes the state. `rounds` rounds alternate the ways; the median is reported, every round's figure kept in
`*_rounds`, `*_spread` is (max - min) / median of the rounds.
`feature_costs_us` is fused_bits - parent and `feature_over_parent` their ratio: the price of the feature.
`fused_saves_us` is pair - fused_bits_records (like for like: both write the records); `fused_faster` says whether even
the slowest fused round beats the fastest pair round, `fused_slower` whether every fused round is above every pair round
-- the condition under which policy_act would take the pair for retardant policies. Anything in between is no measured
difference. Needs a HIP device; there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_advanced_policy import SHAPES, mid_episode, timed  # noqa: E402  (the same state and the same clock)

CONFIG = {"radius": 5, "block": 8, "hidden": 64, "doused": 0.05}


def bench_shape(cfg, device, act_reps, rounds):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import SLOT, BoundCall
    from gymca_amd.forest_fire.bulldozer import AdvancedForestFireBulldozerEnv, BulldozerPolicy

    E, N = cfg["E"], cfg["N"]
    env = AdvancedForestFireBulldozerEnv(N, N, key=1, num_envs=E, use_hidden=False, device=device, observation="grid")
    env.reset()
    mid_episode(env, device)
    gen = torch.Generator(device=device).manual_seed(0xD0)
    env.set_state(dousing=(torch.rand((E, N, N), device=device, generator=gen) < CONFIG["doused"]).to(torch.uint8))
    assert env.dous_bits is not None
    pol = BulldozerPolicy(env, CONFIG["radius"], CONFIG["block"], CONFIG["hidden"], seed=3, retardant=True)
    old = BulldozerPolicy(env, CONFIG["radius"], CONFIG["block"], CONFIG["hidden"], seed=3)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)
    one = {f"{k}_out": new(shape[1:], dtype) for k, (dtype, shape) in env.policy_record_shapes(pol, 1).items()}
    small = dict(action_out=one["action_out"], logits_out=one["logits_out"], value_out=one["value_out"])
    full = dict(small, local_out=one["local_out"], coarse_out=one["coarse_out"])
    cur, di = env.cur, env._dev_index
    u8 = BoundCall("gca_advanced_policy_act_retardant", pol.struct, dev.ptr(env.grid[cur]), dev.ptr(env.dousing), None,
                   dev.ptr(env.pos), dev.ptr(env.time_step), E, N, N, env._empty, env._tree, env._fire, env.env_offset,
                   5, 0, dev.ptr(one["action_out"]), 2, dev.ptr(one["logits_out"]), dev.ptr(one["value_out"]), None,
                   None, SLOT, keep=(env.grid, env.dousing, env.pos, env.time_step) + pol.tensors())
    ways = {"fused_bits": lambda: env.policy_act(pol, seed=5, fused=True, **small),
            "fused_bits_records": lambda: env.policy_act(pol, seed=5, fused=True, **full),
            "fused_u8": lambda: u8(dev.raw_stream(di)),
            "pair": lambda: env.policy_act(pol, seed=5, fused=False, **full),
            "parent": lambda: env.policy_act(old, seed=5, **small)}
    # the two routes to the retardant give the same bits before anything is timed
    ways["fused_bits"]()
    a = {k: v.clone() for k, v in small.items()}
    ways["fused_u8"]()
    torch.cuda.synchronize(device)
    assert all(torch.equal(a[k].view(torch.uint8), small[k].view(torch.uint8)) for k in small)
    runs = {w: [] for w in ways}
    for _ in range(rounds):
        for w, fn in ways.items():
            runs[w].append(timed(fn, act_reps))
    out = {"name": cfg["name"], "E": E, "H": N, "W": N, "C": old.C, "C2": pol.C, "plane_bytes": E * N * N,
           "bits_bytes": E * N * N // 8, "doused_cells": int(env.dousing.sum().item())}
    for w, v in runs.items():
        med = statistics.median(v)
        out[f"{w}_us"] = med
        out[f"{w}_rounds"] = v
        out[f"{w}_spread"] = (max(v) - min(v)) / med
    out["feature_costs_us"] = out["fused_bits_us"] - out["parent_us"]
    out["feature_over_parent"] = out["fused_bits_us"] / out["parent_us"]
    out["u8_over_bits"] = out["fused_u8_us"] / out["fused_bits_us"]
    out["fused_saves_us"] = out["pair_us"] - out["fused_bits_records_us"]
    out["pair_over_fused"] = out["pair_us"] / out["fused_bits_records_us"]
    out["fused_faster"] = bool(max(runs["fused_bits_records"]) < min(runs["pair"]))
    out["fused_slower"] = bool(min(runs["fused_bits_records"]) > max(runs["pair"]))
    del u8, env
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--act-reps", type=int, default=50, help="timed calls per way and round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds that alternate the ways (>= 5); the median is reported")
    ap.add_argument("--shapes", default=",".join(s["name"] for s in SHAPES))
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.act_reps < 1 or args.rounds < 5:
        sys.exit("bench_advanced_policy_retardant.py: --act-reps >= 1, --rounds >= 5")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_advanced_policy_retardant.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    device = torch.device("cuda", 0)
    shapes = [s for s in SHAPES if s["name"] in args.shapes.split(",")]
    res = {"bench": "advanced_policy_retardant", "device": torch.cuda.get_device_name(0), **CONFIG,
           "act_reps": args.act_reps, "rounds": args.rounds,
           "timing": "HIP events around the timed calls after one warm-up call, mean us per call of all E envs; median "
                     "over alternating rounds, spread = (max - min) / median",
           "shapes": [bench_shape(c, device, args.act_reps, args.rounds) for c in shapes]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
