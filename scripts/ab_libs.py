"""Same-process interleaved A/B of the march step between builds of libgca_hip.so (scripts/build_variant.sh) on the
bench's config-3 state (4096 x 256^2, R = 6): every library is loaded into this one process, the outputs of three
chained launches are compared bit for bit against the first library's (grid, ages, counts), then `passes` passes, each
timing every library in turn from the same restored state (K launches between HIP events, median of `reps`).
The spread between a library's passes is the session's noise floor; a difference counts only well outside it.
Usage (GPU box): python scripts/ab_libs.py [--mode flat_uniform|flat|general|rgb] [--passes N] [--K N] [--reps N]
name=path.so ...
Prints one JSON line."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")]


def main(libs, mode="flat_uniform", passes=3, E=4096, N=256, K=10, reps=5):
    import torch

    import bench
    from gymca_amd import _device as dev
    from gymca_amd import _lib
    from gymca_amd.forest_fire.bulldozer import AdvancedForestFireBulldozerEnv

    device = torch.device("cuda", 0)
    env = AdvancedForestFireBulldozerEnv(N, N, key=1, num_envs=E, use_hidden=False, device=device, observation="rgb")
    env.reset()
    st = dev.stream_ptr(device)
    assert env.uniform_layers and bool((env.slope_data.abs() == 1.0).all())
    rgb = mode == "rgb"
    sym = "gca_alex_step_march_rgb" if rgb else "gca_alex_step_march"
    fns = {}
    for name, path in libs:
        lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        fn = getattr(lib, sym)
        fn.argtypes, fn.restype = _lib._SIGNATURES[sym]
        fns[name] = (fn, lib)

    def launch(name):
        a, b = env.cur, 1 - env.cur
        flat = mode in ("flat", "flat_uniform", "rgb")
        args = [env.alex_params, E, N, N, dev.ptr(env.grid[a]), dev.ptr(env.grid[b]), dev.ptr(env.age[a]),
                dev.ptr(env.age[b]), None if mode in ("flat_uniform", "rgb") else dev.ptr(env.vd),
                dev.ptr(env.dous_bits), None if flat else dev.ptr(env.slope_data), dev.ptr(env.wind_index),
                dev.ptr(env.rng_step), dev.ptr(env.counts), None, None]
        if rgb:
            args += [dev.ptr(env.obs_colors), dev.ptr(env.is_night), dev.ptr(env.rgb)]
        fn, lib = fns[name]
        if fn(*args, st) != 0:
            raise RuntimeError(f"{name}: {lib.gca_last_error()}")
        env.cur = b

    out = {"E": E, "N": N, "K": K, "reps": reps, "mode": mode, "libs": {n: os.path.relpath(p, ROOT) for n, p in libs}}
    ref = None
    same = {}
    for name, _ in libs:
        bench.synthetic_state(env, 0, device)
        for _ in range(3):
            launch(name)
        torch.cuda.synchronize()
        got = (env.grid[env.cur].clone(), env.age[env.cur].clone(), env.counts.clone(), env.rgb.clone() if rgb else None)
        if ref is None:
            ref = got
        same[name] = all(torch.equal(x, y) for x, y in zip(ref, got) if x is not None)
    out["bit_exact_vs_first"] = same
    del ref, got
    ms = {name: [] for name, _ in libs}
    for _ in range(passes):
        for name, _ in libs:
            times = []
            for _ in range(reps):
                bench.synthetic_state(env, 0, device)
                launch(name)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(K):
                    launch(name)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1) / K)
            times.sort()
            ms[name].append(round(times[len(times) // 2], 4))
    out["ms"] = ms
    first = libs[0][0]
    base = sorted(ms[first])[len(ms[first]) // 2]
    out["spread_pct"] = {n: round(100.0 * (max(v) - min(v)) / min(v), 2) for n, v in ms.items()}
    out["vs_first_pct"] = {n: round(100.0 * (sorted(v)[len(v) // 2] / base - 1.0), 2) for n, v in ms.items()}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    kw = {}
    for key, conv in (("--mode", str), ("--passes", int), ("--K", int), ("--reps", int)):
        if key in argv:
            i = argv.index(key)
            kw[key[2:]] = conv(argv[i + 1])
            del argv[i:i + 2]
    main([tuple(a.split("=", 1)) for a in argv], **kw)
