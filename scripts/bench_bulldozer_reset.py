#!/usr/bin/env python
"""Per-env reset of the batched ForestFireBulldozer env (gca_bulldozer_reset_where): what the launch costs, timed in one
run with HIP events. Prints one JSON line; --out also writes it to a file.

    python scripts/bench_bulldozer_reset.py --steps 200 --warmup 20 --out profiles/bulldozer_reset.json

Per shape (1024 x 256^2 and 1024 x 512^2), microseconds per call, the median of --rounds rounds that alternate the
variants (every round's figure is kept in `*_rounds`):
  reset_us            today's full-batch reset(): fill launch, host draws, fancy-index write, copies, count launch
  reset_where_all_us  reset_where(all-ones mask): the same result in one launch
  copy_us / copy_gbs  gca_bench_copy of one grid set (E*H*W bytes read and written): the store floor's yardstick
  step_us             env.step, autoreset=False, on a state where no env is done
  step_idle_us        env.step, autoreset=True, same state: the step plus a reset launch that selects nothing
  step_1pct_us        env.step, autoreset=True with max_episode_steps=100 and staggered episode clocks, so about 1 % of
                      the envs reset on every step (`resets_per_step` is what was counted)
  step_graph_us, step_idle_graph_us, step_1pct_graph_us   the same three replayed from a HIP graph of 8 steps, per env
                      step: the device's share, without the host's launch work
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

SHAPES = ({"name": "1024x256x256", "E": 1024, "H": 256, "W": 256}, {"name": "1024x512x512", "E": 1024, "H": 512, "W": 512})
LIMIT = 100  # the 1 % variant's time limit


def timed(fn, steps, warmup):
    """Mean microseconds per call over `steps` calls between two HIP events, after `warmup` calls."""
    import torch

    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / steps


def bench_shape(cfg, device, steps, warmup, rounds):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv
    from gymca_amd.graph import StepGraph

    E, H, W = cfg["E"], cfg["H"], cfg["W"]
    mk = lambda **kw: BatchedForestFireBulldozerEnv(E, H, W, device=device, seed=1, materialize_obs=False, **kw)
    plain, idle, busy = mk(), mk(autoreset=True), mk(autoreset=True, max_episode_steps=LIMIT)
    for env in (plain, idle, busy):
        env.reset(seed=2)
    busy.steps_elapsed.copy_(torch.arange(E, device=device) % LIMIT)  # one env in a hundred is due on every step
    act = plain.sample_actions().clone()
    ones = torch.ones(E, dtype=torch.uint8, device=device)
    scratch = mk()  # the two full-batch resets run on an env of their own
    scratch.reset(seed=2)
    nbytes = E * H * W  # a multiple of 16 for both shapes
    st = dev.stream_ptr(device)
    src, dst = scratch.buf[1], plain.buf[1].clone()
    variants = {
        "reset_us": (lambda: scratch.reset(seed=2), max(5, steps // 10), 2),
        "reset_where_all_us": (lambda: scratch.reset_where(ones), max(5, steps // 10), 2),
        "copy_us": (lambda: call("gca_bench_copy", dev.ptr(src), dev.ptr(dst), nbytes, 0, st), max(5, steps // 10), 2),
        "step_us": (lambda: plain.step(act), steps, warmup),
        "step_idle_us": (lambda: idle.step(act), steps, warmup),
        "step_1pct_us": (lambda: busy.step(act), steps, warmup),
    }
    # the same three steps replayed from a HIP graph of G steps (no host work between launches): us per env step
    G = 8
    for k, env in (("step_graph_us", plain), ("step_idle_graph_us", idle), ("step_1pct_graph_us", busy)):
        g = StepGraph(lambda env=env: env.step(act), n_steps=G, device=device, warmup=1)
        variants[k] = (g.replay, max(5, steps // G), max(1, warmup // G))
    per_call = {k: (G if k.endswith("graph_us") else 1) for k in variants}
    runs = {k: [] for k in variants}
    torch.cuda.synchronize(device)
    ep0 = busy.episode.sum().item()
    busy_steps = 0
    for _ in range(rounds):
        for k, (fn, n, w) in variants.items():
            runs[k].append(timed(fn, n, w) / per_call[k])
            busy_steps += (n + w) * per_call[k] if k.startswith("step_1pct") else 0
    out = {"name": cfg["name"], "E": E, "H": H, "W": W, "fused": bool(plain.fused)}
    for k, v in runs.items():
        out[k] = statistics.median(v)
        out[k.replace("_us", "_rounds")] = v
    out["copy_gbs"] = 2.0 * nbytes / (out["copy_us"] * 1e-6) / 1e9
    out["reset_where_all_store_gbs"] = nbytes / (out["reset_where_all_us"] * 1e-6) / 1e9
    out["reset_where_all_over_copy"] = out["reset_where_all_us"] / out["copy_us"]
    out["reset_over_reset_where_all"] = out["reset_us"] / out["reset_where_all_us"]
    out["idle_launch_us"] = out["step_idle_us"] - out["step_us"]
    out["idle_launch_frac_of_step"] = out["idle_launch_us"] / out["step_us"]
    out["one_pct_over_step"] = out["step_1pct_us"] / out["step_us"]
    out["idle_launch_graph_us"] = out["step_idle_graph_us"] - out["step_graph_us"]
    out["idle_launch_graph_frac_of_step"] = out["idle_launch_graph_us"] / out["step_graph_us"]
    out["one_pct_graph_over_step"] = out["step_1pct_graph_us"] / out["step_graph_us"]
    out["resets_per_step"] = (busy.episode.sum().item() - ep0) / busy_steps
    # the step variants must have run on live envs: a finished env's step is a no-op and would flatter the figure
    out["done_envs_after"] = {"plain": int(plain.done.sum().item()), "idle_episodes": int(idle.episode.sum().item())}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_bulldozer_reset.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    device = torch.device("cuda", 0)
    res = {"bench": "bulldozer_reset", "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds,
           "timing": "HIP events around consecutive eager calls, mean us per call; median over alternating rounds",
           "shapes": [bench_shape(c, device, args.steps, args.warmup, args.rounds) for c in SHAPES]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
