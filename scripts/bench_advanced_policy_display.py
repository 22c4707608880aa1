#!/usr/bin/env python
"""A measurement, not a test: the extension agent's observe-and-act on the Advanced bulldozer env, the fused launch
(gca_advanced_policy_act_display) against the triple it is defined by (gca_advanced_display -> gca_policy_observation ->
gca_extension_policy_act), and against gca_advanced_policy_act on the true grid of the same state (the price of the
display).

    python scripts/bench_advanced_policy_display.py [--rounds 5] [--iters 20] [--quick]

Shapes 4096 x 256^2 and 1024 x 512^2 (radius 5, block 8, hidden 64); three choice mixes per shape -- all 0 (the blurred
base), all 1 (the raw grid), the three choices in equal thirds -- with and without the observation records. Per
configuration: `rounds` rounds of `iters` back-to-back calls between two events; the medians and every round go to
profiles/advanced_policy_display.json. policy_act keeps the fused launch as its default only if every fused round is
below every triple round at both shapes in the mixed case (`fused_default` in the file). Needs a HIP device."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="an eighth of the envs (a check that the script runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "advanced_policy_display.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_advanced_policy_display.py needs a HIP device")
    from gymca_amd.forest_fire.bulldozer import (AdvancedForestFireBulldozerEnv, BulldozerPolicy,
                                                 ExtensionBulldozerPolicy)

    device = torch.device("cuda", 0)

    def timed(fn):
        fn()
        torch.cuda.synchronize(device)
        rounds = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize(device)
            rounds.append(a.elapsed_time(b) * 1e3 / args.iters)  # microseconds per call
        return rounds

    results = []
    for E, N in ((4096, 256), (1024, 512)):
        E = max(E // 8, 3) if args.quick else E
        env = AdvancedForestFireBulldozerEnv(N, N, key=1, num_envs=E, device=device, observation="grid",
                                             hidden_rng="philox", enable_extensions=True)
        env.reset()
        for _ in range(4):  # a few steps into the episode: fire fronts, bulldozers off their start cells
            env.step(torch.randint(0, 2, (E, 3), dtype=torch.int32, device=device) * torch.tensor([4, 1, 0], device=device,
                                                                                                 dtype=torch.int32))
        pol = ExtensionBulldozerPolicy(env, radius=5, block=8, hidden=64, seed=0)
        two = BulldozerPolicy(env, radius=5, block=8, hidden=64, seed=0)
        spec = env.policy_record_shapes(pol, 1)
        new = lambda k: torch.empty(spec[k][1][1:], dtype=spec[k][0], device=device)
        action, logits, value, local, coarse = new("action"), new("logits"), new("value"), new("local"), new("coarse")
        a2, l2 = torch.empty((E, 2), dtype=torch.int32, device=device), torch.empty((E, 11), device=device)
        mixes = {"all0": torch.zeros(E, dtype=torch.int32, device=device),
                 "all1": torch.ones(E, dtype=torch.int32, device=device),
                 "mixed": (torch.arange(E, device=device) % 3).to(torch.int32)}
        for mix, choice in mixes.items():
            for records in (False, True):
                rec = dict(local_out=local, coarse_out=coarse) if records else {}
                row = dict(envs=E, rows=N, cols=N, mix=mix, records=records)
                for name, fused in (("fused", True), ("triple", False)):
                    row[name] = timed(lambda: env.policy_act(pol, seed=3, action_out=action, logits_out=logits,
                                                             value_out=value, fused=fused, choice=choice, **rec))
                row["true_grid"] = timed(lambda: env.policy_act(two, seed=3, action_out=a2, logits_out=l2,
                                                                value_out=value, **rec))
                row["median_us"] = {k: statistics.median(row[k]) for k in ("fused", "triple", "true_grid")}
                print(f"{E} x {N}^2 {mix:5s} records={records!s:5s} " +
                      "  ".join(f"{k} {v:8.1f} us" for k, v in row["median_us"].items()))
                results.append(row)
        del env
    mixed = [r for r in results if r["mix"] == "mixed"]
    fused_default = all(max(r["fused"]) < min(r["triple"]) for r in mixed)
    print("fused_default:", fused_default)
    if not args.quick:
        with open(args.out, "w") as f:
            json.dump(dict(rounds=args.rounds, iters=args.iters, unit="microseconds per policy_act call",
                           fused_default=fused_default, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
