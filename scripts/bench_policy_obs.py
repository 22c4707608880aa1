#!/usr/bin/env python
"""env.observe() of the batched bulldozer / helicopter envs (gca_policy_observation): what a closed-loop agent pays to
look at its envs, timed in one run with HIP events. Prints one JSON line; --out also writes it to a file.

    python scripts/bench_policy_obs.py --steps 200 --warmup 20 --out profiles/policy_obs.json

Per shape (bulldozer 1024 x 256^2 and 1024 x 512^2 with radius 16, block 16; helicopter 4096 x 42 x 42 with radius 16,
block 8), microseconds per call, the median of --rounds rounds that alternate the variants (every round's figure is kept
in `*_rounds`):
  step_us            env.step alone, materialize_obs=False
  step_observe_us    env.step then env.observe into pre-allocated outputs
  observe_us         env.observe alone (form 0: the kernel the shape picks); observe_generic_us / observe_rows_us: forms 1
                     and 2 where they apply
  step_torch_us      env.step then the same observation built from the public surface that existed before observe():
                     env.grids(), two compares, avg_pool2d, and the window by an index gather on a class tensor padded
                     with 3. The yardstick: what a user could do without observe(). Checked once against observe().
  copy_us / copy_gbs gca_bench_copy of E*H*W bytes (read and written): the read floor's yardstick
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

SHAPES = ({"name": "bulldozer_1024x256x256", "env": "bulldozer", "E": 1024, "H": 256, "W": 256, "radius": 16, "block": 16},
          {"name": "bulldozer_1024x512x512", "env": "bulldozer", "E": 1024, "H": 512, "W": 512, "radius": 16, "block": 16},
          {"name": "helicopter_4096x42x42", "env": "helicopter", "E": 4096, "H": 42, "W": 42, "radius": 16, "block": 8})


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


def torch_observation(grid, pos, tree, fire, r, B):
    """(local, coarse) of grid (E, H, W) uint8 / pos (E, 2) with torch ops only: the observation a user of the env's
    public surface builds from env.grids()."""
    import torch
    import torch.nn.functional as F

    E, H, W = grid.shape
    S = 2 * r + 1
    is_tree, is_fire = grid == tree, grid == fire
    planes = torch.stack([is_tree, is_fire], dim=1).float()
    planes = F.pad(planes, (0, -W % B, 0, -H % B))  # a block that sticks out counts its in-grid cells only
    coarse = F.avg_pool2d(planes, B)
    cls = F.pad(is_tree.to(torch.uint8) + 2 * is_fire.to(torch.uint8), (r, r, r, r), value=3)
    ar = torch.arange(S, device=grid.device)
    rows = (pos[:, 0:1].long() + ar)[:, :, None]
    cols = (pos[:, 1:2].long() + ar)[:, None, :]
    local = cls[torch.arange(E, device=grid.device)[:, None, None], rows, cols]
    return local, coarse


def bench_shape(cfg, device, steps, warmup, rounds):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call
    from gymca_amd.forest_fire import policy_obs

    E, H, W, r, B = cfg["E"], cfg["H"], cfg["W"], cfg["radius"], cfg["block"]
    if cfg["env"] == "bulldozer":
        from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv as Env
    else:
        from gymca_amd.forest_fire.helicopter.batched import BatchedForestFireHelicopterEnv as Env
    env = Env(E, H, W, device=device, seed=1, materialize_obs=False)
    env.reset(seed=2)
    act = env.sample_actions().clone()
    ls, cs = policy_obs.output_shapes(env, r, B)
    lo = torch.empty(ls, dtype=torch.uint8, device=device)
    co = torch.empty(cs, dtype=torch.float32, device=device)
    rows_apply = W in (256, 512) and B in (8, 16, 32) and H % B == 0
    nbytes = E * H * W  # a multiple of 16 for the three shapes
    st = dev.stream_ptr(device)
    src, dst = env.buf[1].clone(), torch.empty_like(env.buf[1])
    tree, fire = env._tree, env._fire

    def step_torch():
        env.step(act)
        return torch_observation(env.grids(), env.pos, tree, fire, r, B)

    def step_observe():
        env.step(act)
        env.observe(r, B, lo, co)

    # the yardstick builds the same observation (checked once, on a stepped state)
    for _ in range(3):
        env.step(act)
    tl, tc = torch_observation(env.grids(), env.pos, tree, fire, r, B)
    env.observe(r, B, lo, co)
    torch_equal = bool(torch.equal(tl, lo) and torch.equal(tc, co))

    few = max(5, steps // 10)
    variants = {
        "step_us": (lambda: env.step(act), steps, warmup),
        "step_observe_us": (step_observe, steps, warmup),
        "observe_us": (lambda: env.observe(r, B, lo, co), steps, warmup),
        "observe_generic_us": (lambda: env.observe(r, B, lo, co, form=1), few if rows_apply else steps, 2),
        "step_torch_us": (step_torch, few, 2),
        "copy_us": (lambda: call("gca_bench_copy", dev.ptr(src), dev.ptr(dst), nbytes, 0, st), steps, warmup),
    }
    if rows_apply:
        variants["observe_rows_us"] = (lambda: env.observe(r, B, lo, co, form=2), steps, warmup)
    runs = {k: [] for k in variants}
    torch.cuda.synchronize(device)
    for _ in range(rounds):
        for k, (fn, n, w) in variants.items():
            runs[k].append(timed(fn, n, w))
    out = {"name": cfg["name"], "env": cfg["env"], "E": E, "H": H, "W": W, "radius": r, "block": B,
           "form_picked": "rows" if rows_apply else "generic", "torch_path_equals_observe": torch_equal}
    for k, v in runs.items():
        out[k] = statistics.median(v)
        out[k.replace("_us", "_rounds")] = v
    out["copy_gbs"] = 2.0 * nbytes / (out["copy_us"] * 1e-6) / 1e9
    out["observe_read_gbs"] = nbytes / (out["observe_us"] * 1e-6) / 1e9
    out["observe_over_copy"] = out["observe_us"] / out["copy_us"]
    out["observe_in_step_us"] = out["step_observe_us"] - out["step_us"]
    out["torch_obs_in_step_us"] = out["step_torch_us"] - out["step_us"]
    out["torch_obs_over_observe"] = out["torch_obs_in_step_us"] / out["observe_us"]
    out["step_torch_over_step_observe"] = out["step_torch_us"] / out["step_observe_us"]
    if cfg["env"] == "bulldozer":  # the step variants must have run on live envs: a finished env's step is a no-op
        out["done_envs_after"] = int(env.done.sum().item())
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
        sys.exit("bench_policy_obs.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    device = torch.device("cuda", 0)
    res = {"bench": "policy_obs", "device": torch.cuda.get_device_name(0), "steps": args.steps,
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
