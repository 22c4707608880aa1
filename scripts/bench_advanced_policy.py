#!/usr/bin/env python
"""The bulldozer agent on the Advanced (Alexandridis) bulldozer env: what observe-and-act in one launch
(gca_advanced_policy_act) costs against the two launches it replaces, against the env step, and what a recorded
closed-loop step costs in all. Prints one JSON line; --out also writes it.

    python scripts/bench_advanced_policy.py --out profiles/advanced_policy.json

Per shape (4096 x 256^2 and 1024 x 512^2; radius 5, block 8, 64 hidden units, observation="grid", use_hidden=False,
the mid-episode state of bench.py: grid iid {EMPTY .1, TREE .8, FIRE .1}, fire ages iid [1, 672], wind iid), in
microseconds per call of all E envs:
  act_fused          env.policy_act(policy): one launch, no observation record
  act_fused_records  the same with local_out / coarse_out, as rollout_policy calls it
  act_pair           env.policy_act(policy, fused=False): gca_policy_observation, time_step.to(int64),
                     gca_bulldozer_policy_act; it writes local / coarse by construction
  step               env.step(action) on a fixed action
  rollout_eager      env.rollout_policy(policy, K) with every record given, per env step
  rollout_graph      the same call captured once and replayed, per env step
No way restores the state: act changes none, and step / the rollouts move the env on from mid-episode to mid-episode
(autoreset on), so later rounds see somewhat later fires. `rounds` rounds alternate the ways; the median is reported and
every round's figure kept in `*_rounds`; `*_spread` is (max - min) / median of the rounds.
`fused_saves_us` is act_pair - act_fused_records (like for like: both write the records), `fused_faster` says whether
even the slowest fused round beats the fastest pair round, i.e. whether the gain exceeds the run-to-run spread.
Needs a HIP device; there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ({"name": "4096x256x256", "E": 4096, "N": 256}, {"name": "1024x512x512", "E": 1024, "N": 512})
CONFIG = {"K": 128, "radius": 5, "block": 8, "hidden": 64}


def timed(fn, reps):
    """Mean microseconds per call over `reps` calls between two HIP events, after one warm-up call."""
    import torch

    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def mid_episode(env, device):
    import torch

    E, N = env.num_envs, env.nrows
    gen = torch.Generator(device=device).manual_seed(0xC3)
    u = torch.rand((E, N, N), device=device, generator=gen)
    grid = torch.where(u < 0.1, 0, torch.where(u < 0.9, 1, 2)).to(torch.uint8)
    age = torch.where(grid == 2, torch.randint(1, 673, (E, N, N), device=device, generator=gen, dtype=torch.int16),
                      torch.zeros((), dtype=torch.int16, device=device))
    widx = torch.randint(0, 8, (E,), device=device, generator=gen, dtype=torch.int32)
    env.set_state(grid=grid, fire_age=age, wind_index=widx)


def bench_shape(cfg, device, K, reps, act_reps, rounds):
    import torch

    from gymca_amd.forest_fire.bulldozer import AdvancedForestFireBulldozerEnv, BulldozerPolicy

    E, N = cfg["E"], cfg["N"]
    env = AdvancedForestFireBulldozerEnv(N, N, key=1, num_envs=E, use_hidden=False, device=device, observation="grid")
    env.reset()
    mid_episode(env, device)
    pol = BulldozerPolicy(env, CONFIG["radius"], CONFIG["block"], CONFIG["hidden"], seed=3)
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=device)
    rec = {f"{k}_out": new(shape, dtype) for k, (dtype, shape) in env.policy_record_shapes(pol, K).items()}
    one = {k: v[0] for k, v in rec.items()}
    small = dict(action_out=one["action_out"], logits_out=one["logits_out"], value_out=one["value_out"])
    full = dict(small, local_out=one["local_out"], coarse_out=one["coarse_out"])
    gen = torch.Generator(device="cpu").manual_seed(K)
    action = torch.stack([torch.randint(0, 9, (E,), generator=gen, dtype=torch.int32),
                          torch.randint(0, 2, (E,), generator=gen, dtype=torch.int32)], dim=1).to(device)
    rollout = lambda: env.rollout_policy(pol, K, seed=5, **rec)
    rollout()  # warms the bound calls before the capture, which itself runs nothing
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rollout()
    # (callable, timed calls per round, env steps per call)
    ways = {"act_fused": (lambda: env.policy_act(pol, seed=5, **small), act_reps, 1),
            "act_fused_records": (lambda: env.policy_act(pol, seed=5, **full), act_reps, 1),
            "act_pair": (lambda: env.policy_act(pol, seed=5, fused=False, **full), act_reps, 1),
            # two steps per call: the env's current plane is back where the captured graph expects it
            "step": (lambda: (env.step(action), env.step(action)), max(act_reps // 2, 1), 2),
            "rollout_eager": (rollout, reps, K),
            "rollout_graph": (graph.replay, reps, K)}
    runs = {w: [] for w in ways}
    for _ in range(rounds):
        for w, (fn, n, per) in ways.items():
            runs[w].append(timed(fn, n) / per)
    out = {"name": cfg["name"], "E": E, "H": N, "W": N, "C": pol.C, "march": bool(env.march),
           "plane_bytes": E * N * N, "episodes_ended_last_rollout": int(rec["terminated_out"].sum().item())}
    for w, v in runs.items():
        med = statistics.median(v)
        out[f"{w}_us"] = med
        out[f"{w}_rounds"] = v
        out[f"{w}_spread"] = (max(v) - min(v)) / med
    out["plane_read_gbs_act_fused"] = out["plane_bytes"] / (out["act_fused_us"] * 1e-6) / 1e9
    out["fused_saves_us"] = out["act_pair_us"] - out["act_fused_records_us"]
    out["pair_over_fused"] = out["act_pair_us"] / out["act_fused_records_us"]
    out["fused_faster"] = bool(max(runs["act_fused_records"]) < min(runs["act_pair"]))
    out["act_over_step"] = out["act_fused_us"] / out["step_us"]
    out["graph_over_eager"] = out["rollout_graph_us"] / out["rollout_eager_us"]
    out["env_steps_per_second_rollout_graph"] = E / (out["rollout_graph_us"] * 1e-6)
    del graph, rec, env
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=2, help="timed rollouts of K env steps per round")
    ap.add_argument("--act-reps", type=int, default=50, help="timed calls of act / step per round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds that alternate the ways (>= 5); the median is reported")
    ap.add_argument("--steps", type=int, default=CONFIG["K"], help="K, even (the rollout is captured as a graph)")
    ap.add_argument("--shapes", default=",".join(s["name"] for s in SHAPES))
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.reps < 1 or args.act_reps < 1 or args.rounds < 5 or args.steps < 2 or args.steps % 2:
        sys.exit("bench_advanced_policy.py: --reps and --act-reps >= 1, --rounds >= 5, --steps even and >= 2")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_advanced_policy.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    device = torch.device("cuda", 0)
    shapes = [s for s in SHAPES if s["name"] in args.shapes.split(",")]
    res = {"bench": "advanced_policy", "device": torch.cuda.get_device_name(0), **CONFIG, "K": args.steps,
           "reps": args.reps, "act_reps": args.act_reps, "rounds": args.rounds,
           "timing": "HIP events around the timed calls after one warm-up call, mean us per call (rollouts: per env "
                     "step) of all E envs; median over alternating rounds, spread = (max - min) / median",
           "shapes": [bench_shape(c, device, args.steps, args.reps, args.act_reps, args.rounds) for c in shapes]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
