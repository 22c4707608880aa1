#!/usr/bin/env python
"""Batched ForestFireHelicopter env step: the fused gca_helicopter_step against the same work done with the entry
points that existed before it (gca_ds_step in Philox mode over all E envs + gca_move_modify + gca_count_cells on the
same kind of buffers), timed in the same run with HIP events. Prints one JSON line; --out also writes it to a file.

    python scripts/bench_helicopter.py --steps 200 --warmup 20 --out profiles/helicopter_batched.json

Per shape: `fused_us` (env.step with a device action tensor), `fused_random_us` (env.step_random: the action drawn in
the step), `sequence_us` (the three-launch sequence; on a countdown step it skips the CA like the single env's host
logic does, and its reward stays on the host side of a read-back that is NOT timed here), `copy_us` / `copy_gbs`
(gca_bench_copy of one grid set, E*H*W bytes in and out) and the fused CA step's algorithmic traffic (1 B read + 1 B
written per cell) as a fraction of that copy's rate. Needs a HIP device; there is no CPU fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = (
    {"name": "1024x256x256_freeze0", "E": 1024, "H": 256, "W": 256, "freeze": 0},
    {"name": "1024x256x256_default_freeze", "E": 1024, "H": 256, "W": 256, "freeze": None},
    {"name": "4096x64x64_freeze0", "E": 4096, "H": 64, "W": 64, "freeze": 0},
)


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


def bench_shape(cfg, device, steps, warmup):
    import torch

    from gymca_amd import _device as dev
    from gymca_amd._lib import call
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv
    from gymca_amd.forest_fire.operators.move_modify import make_params

    E, H, W = cfg["E"], cfg["H"], cfg["W"]
    env = BatchedForestFireHelicopterEnv(E, H, W, device=device, seed=1, freeze=cfg["freeze"], materialize_obs=False)
    env.reset()
    act = env.sample_actions().clone()
    out = {"name": cfg["name"], "E": E, "H": H, "W": W, "max_freeze": env.max_freeze}
    out["fused_us"] = timed(lambda: env.step(act), steps, warmup)
    out["fused_random_us"] = timed(lambda: env.step_random(seed=9), steps, warmup)

    # the same work with the entry points that predate the fused step, on buffers of the same shape
    st = dev.stream_ptr(device)
    sets = {"up": {0, 1, 2}, "down": {6, 7, 8}, "left": {0, 3, 6}, "right": {2, 5, 8}}
    params = make_params(sets, {2: 0})
    buf = env.buf.clone()
    pos = env.pos.clone()
    counts = torch.zeros((E, 3), dtype=torch.int32, device=device)
    hit = torch.zeros(E, dtype=torch.uint8, device=device)
    rng_step = torch.zeros(E, dtype=torch.int32, device=device)
    act2 = torch.stack([act, torch.ones_like(act)], dim=1).contiguous()
    state = {"cur": 0, "freeze": env.max_freeze}

    def sequence():
        cur = state["cur"]
        if state["freeze"] == 0:  # the single env's host countdown (helicopter.py:220-236), all envs in lockstep
            call("gca_ds_step", dev.ptr(buf[cur]), dev.ptr(buf[cur ^ 1]), E, H, W, 0, 1, 2, dev.ptr(env.thresholds),
                 None, None, 1, dev.ptr(rng_step), 0, None, st)
            cur = state["cur"] = cur ^ 1
            state["freeze"] = env.max_freeze
        else:
            state["freeze"] -= 1
        call("gca_move_modify", params, dev.ptr(act2), dev.ptr(pos), dev.ptr(buf[cur]), H, W, dev.ptr(hit), E, st)
        call("gca_count_cells", dev.ptr(buf[cur]), E, H, W, 0, 1, 2, dev.ptr(counts), st)
        rng_step.add_(1)

    out["sequence_us"] = timed(sequence, steps, warmup)
    out["sequence_over_fused"] = out["sequence_us"] / out["fused_us"]

    nbytes = E * H * W  # a multiple of 16 for every shape here
    src, dst = buf[0], buf[1]
    out["copy_us"] = timed(lambda: call("gca_bench_copy", dev.ptr(src), dev.ptr(dst), nbytes, 0, st), steps, warmup)
    out["copy_gbs"] = 2.0 * nbytes / (out["copy_us"] * 1e-6) / 1e9
    if env.max_freeze == 0:  # every step is a CA step: 1 B read + 1 B written per cell
        out["fused_bytes_per_cell"] = 2.0
        out["fused_gbs"] = 2.0 * nbytes / (out["fused_us"] * 1e-6) / 1e9
        out["fused_frac_of_copy_rate"] = out["fused_gbs"] / out["copy_gbs"]
        out["fused_ns_per_kcell"] = out["fused_us"] * 1e3 / (nbytes / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_helicopter.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    device = torch.device("cuda", 0)
    res = {"bench": "helicopter_batched", "device": torch.cuda.get_device_name(0), "steps": args.steps,
           "warmup": args.warmup, "timing": "HIP events around `steps` consecutive calls, mean us per env step",
           "shapes": [bench_shape(c, device, args.steps, args.warmup) for c in SHAPES]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
