#!/usr/bin/env python
"""The optimizer's half of the helicopter PPO update: forest_fire.ppo.Adam.step (gca_adam_step: global-norm clip and Adam
over all five tensors in two launches), forest_fire.ppo.permutation (one launch) and HelicopterPolicy.ppo_update (4 epochs
x 4 minibatches of ppo_grad + Adam.step, eager and as one replayed graph) at 4096 x 42 x 42 envs, K = 128, against
  (a) Adam as scripts/train_helicopter_ppo.py spelled it in torch before (four ops per tensor), alone and with a
      no-sync torch global-norm clip (torch.nn.utils.clip_grad_norm_'s formulation) in front of it,
  (b) torch.randperm(T).to(int32) per epoch,
  (c) that script's loop: randperm, ppo_grad and the torch Adam per minibatch.
The optimizer step alone is also timed on the largest policy (hidden 256, radius 31: about 4 M parameters), where it is
bound by memory: the 28 B per parameter it must move (read g, read and write w, m, v) over its time, beside the rate of
the library's own copy kernel (gca_bench_copy) on the same number of bytes in the same run.
All in one process, timed with HIP events. Prints one JSON line; --out also writes it.

    python scripts/bench_helicopter_ppo_update.py --out profiles/helicopter_ppo_update.json

Protocol (scripts/bench_helicopter_policy_grad.py's): every variant is warmed up, then `passes` passes visit the variants
in turn (interleaved), each timing `reps` repetitions between two events; the figure of a variant is the median over
its passes, in microseconds per call, and the spread (min, max) is recorded. No ratio is fixed in advance. Needs a HIP
device; there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIG = {"E": 4096, "H": 42, "W": 42, "K": 128, "radius": 5, "block": 8, "hidden": 64, "epochs": 4, "minibatches": 4,
          "big_radius": 31, "big_hidden": 256}
HYPER = dict(lr=2.5e-4, b1=0.9, b2=0.999, eps=1e-5, max_norm=0.5)


def time_once(fn, reps):
    import torch

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


class TorchAdam:
    """Adam as the training script wrote it out in torch: the step count is a Python integer."""

    def __init__(self, params):
        import torch

        self.params = params
        self.m = {n: torch.zeros_like(p) for n, p in params.items()}
        self.v = {n: torch.zeros_like(p) for n, p in params.items()}
        self.t = 0

    def clip(self, grads):
        import torch

        norms = torch.stack([torch.linalg.vector_norm(g) for g in grads.values()])
        coef = (HYPER["max_norm"] / (torch.linalg.vector_norm(norms) + 1e-6)).clamp(max=1.0)
        for g in grads.values():
            g.mul_(coef)

    def step(self, grads, clip=False):
        b1, b2 = HYPER["b1"], HYPER["b2"]
        if clip:
            self.clip(grads)
        self.t += 1
        for n, w in self.params.items():
            g, m, v = grads[n], self.m[n], self.v[n]
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (v / (1 - b2 ** self.t)).sqrt_().add_(HYPER["eps"])
            w.addcdiv_(m, denom, value=-HYPER["lr"] / (1 - b1 ** self.t))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=CONFIG["E"])
    ap.add_argument("--steps", type=int, default=CONFIG["K"])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if min(args.reps, args.passes, args.warmup, args.envs, args.steps) < 1:
        sys.exit("bench_helicopter_ppo_update.py: every count must be >= 1")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_helicopter_ppo_update.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    from gymca_amd import _lib
    from gymca_amd import _device as dev
    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv, HelicopterPolicy
    from gymca_amd.forest_fire.helicopter.policy import WEIGHTS

    device = torch.device("cuda", 0)
    E, K, epochs, mbs = args.envs, args.steps, CONFIG["epochs"], CONFIG["minibatches"]
    T = E * K
    if T % mbs:
        sys.exit("bench_helicopter_ppo_update.py: envs * steps must divide into the minibatches")
    N, steps = T // mbs, epochs * mbs
    env = BatchedForestFireHelicopterEnv(E, CONFIG["H"], CONFIG["W"], device=device, seed=1, materialize_obs=False)
    env.reset()
    pol = HelicopterPolicy(env, CONFIG["radius"], CONFIG["block"], CONFIG["hidden"], seed=3)
    rec = env.rollout_policy(pol, K, seed=5)
    _, _, next_value = env.act(pol, seed=5)
    adv, ret = ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95)
    gen = torch.Generator(device=device).manual_seed(7)
    w0 = {n: getattr(pol, n).clone() for n in WEIGHTS}

    def optimizers(policy):
        """(Adam, TorchAdam on a copy of the weights, gradients of a realistic scale, a copy for the clip to scale)."""
        params = {n: getattr(policy, n) for n in WEIGHTS}
        g = {n: torch.randn(p.shape, generator=gen, device=device) * 1e-2 for n, p in params.items()}
        return (ppo.Adam(params, lr=HYPER["lr"], max_grad_norm=HYPER["max_norm"]),
                TorchAdam({n: p.clone() for n, p in params.items()}), g, {n: t.clone() for n, t in g.items()})

    opt, topt, g, g_t = optimizers(pol)
    big = HelicopterPolicy((CONFIG["H"], CONFIG["W"]), CONFIG["big_radius"], CONFIG["block"], CONFIG["big_hidden"],
                           seed=3, device=device)
    bopt, btopt, bg, bg_t = optimizers(big)
    n_big = sum(p.numel() for p in bopt.params.values())
    n_small = sum(p.numel() for p in opt.params.values())
    info = torch.empty(2, device=device)
    # the copy yardstick: as many bytes through the copy kernel as the big step must move (28 B per parameter)
    copy_bytes = (14 * n_big) // 16 * 16
    src, dst = torch.empty(copy_bytes, dtype=torch.uint8, device=device), torch.empty(copy_bytes, dtype=torch.uint8,
                                                                                       device=device)
    di = device.index
    copy = lambda: _lib.call("gca_bench_copy", src.data_ptr(), dst.data_ptr(), copy_bytes, 0, dev.raw_stream(di))

    # the whole update: ours eager, ours as a graph (a second policy and optimizer), the former loop
    bufs = dict(stats_out=torch.empty((steps, 8), device=device), info_out=torch.empty((steps, 2), device=device),
                perm_out=torch.empty((epochs, T), dtype=torch.int32, device=device),
                grads_out={n: torch.empty_like(getattr(pol, n)) for n in WEIGHTS},
                workspace=torch.empty_like(pol._ppo_workspace(N, None)))
    update = lambda: pol.ppo_update(opt, rec, adv, ret, epochs=epochs, minibatches=mbs, seed=1, **bufs)
    gpol = HelicopterPolicy(env, CONFIG["radius"], CONFIG["block"], CONFIG["hidden"], seed=3)
    gopt = ppo.Adam({n: getattr(gpol, n) for n in WEIGHTS}, lr=HYPER["lr"], max_grad_norm=HYPER["max_norm"])
    gbufs = dict(stats_out=torch.empty((steps, 8), device=device), info_out=torch.empty((steps, 2), device=device),
                 perm_out=torch.empty((epochs, T), dtype=torch.int32, device=device),
                 grads_out={n: torch.empty_like(getattr(gpol, n)) for n in WEIGHTS},
                 workspace=torch.empty_like(bufs["workspace"]))
    gpol.ppo_update(gopt, rec, adv, ret, epochs=1, minibatches=mbs, seed=1)  # binds its calls outside the capture
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gpol.ppo_update(gopt, rec, adv, ret, epochs=epochs, minibatches=mbs, seed=1, **gbufs)
    lpol = HelicopterPolicy(env, CONFIG["radius"], CONFIG["block"], CONFIG["hidden"], seed=3)
    lopt = TorchAdam({n: getattr(lpol, n) for n in WEIGHTS})
    lgrads = {n: torch.empty_like(getattr(lpol, n)) for n in WEIGHTS}
    lstats = torch.empty(8, device=device)

    def former_loop():
        for _ in range(epochs):
            perm = torch.randperm(T, generator=gen, device=device).to(torch.int32)
            for mb in range(mbs):
                lpol.ppo_grad(rec, adv, ret, perm[mb * N:(mb + 1) * N], grads_out=lgrads, stats_out=lstats)
                lopt.step(lgrads)

    def randperms():
        for _ in range(epochs):
            torch.randperm(T, generator=gen, device=device).to(torch.int32)

    fns = {"adam_step": lambda: opt.step(g, info_out=info),
           "torch_adam": lambda: topt.step(g_t),
           "torch_clip_adam": lambda: topt.step(g_t, clip=True),
           "adam_step_big": lambda: bopt.step(bg, info_out=info),
           "torch_adam_big": lambda: btopt.step(bg_t),
           "torch_clip_adam_big": lambda: btopt.step(bg_t, clip=True),
           "copy_big": copy,
           "permutation": lambda: ppo.permutation(T, epochs, seed=1, counter=opt.count, out=bufs["perm_out"]),
           "torch_randperm": randperms,
           "ppo_update": update, "ppo_update_graph": graph.replay, "former_loop": former_loop}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize(device)
    samples = {n: [] for n in fns}
    for _ in range(args.passes):
        for n, fn in fns.items():
            samples[n].append(time_once(fn, args.reps))
    us = {n: statistics.median(v) for n, v in samples.items()}
    # checks in the run: one step of ours against the torch formulation from the same state; the rows are permutations
    for n in WEIGHTS:
        getattr(pol, n).copy_(w0[n])
    copt = ppo.Adam({n: getattr(pol, n) for n in WEIGHTS}, lr=HYPER["lr"], max_grad_norm=HYPER["max_norm"])
    ctopt = TorchAdam({n: w0[n].clone() for n in WEIGHTS})
    cg = {n: torch.randn(w0[n].shape, generator=gen, device=device) for n in WEIGHTS}
    norm_lr = copt.step(cg).tolist()
    ctopt.step({n: t.clone() for n, t in cg.items()}, clip=True)
    err = max(float((getattr(pol, n) - ctopt.params[n]).abs().max()) for n in WEIGHTS)
    perm_ok = bool((bufs["perm_out"].sort(1).values == torch.arange(T, device=device, dtype=torch.int32)).all())
    finite = bool(torch.isfinite(bufs["stats_out"]).all() and torch.isfinite(gbufs["stats_out"]).all())
    res = {"bench": "helicopter_ppo_update", "device": torch.cuda.get_device_name(0), **CONFIG, "E": E, "K": K, "T": T,
           "N": N, "params": n_small, "params_big": n_big, "reps": args.reps, "passes": args.passes,
           "warmup": args.warmup,
           "timing": "HIP events around `reps` calls; median over interleaved passes; us per call",
           "adam_workspace_bytes": int(opt.workspace.numel()), "check_norm_lr": norm_lr,
           "check_step_max_abs_diff_vs_torch": err, "permutation_rows_are_permutations": perm_ok,
           "last_stats": dict(zip(ppo.STATS, [float(x) for x in bufs["stats_out"][-1].cpu()]))}
    for n, v in us.items():
        res[f"{n}_us"] = v
        res[f"{n}_spread"] = [min(samples[n]), max(samples[n])]
    spread = lambda n: max(samples[n]) - min(samples[n])
    res["torch_adam_over_adam_step"] = us["torch_adam"] / us["adam_step"]
    res["torch_clip_adam_over_adam_step"] = us["torch_clip_adam"] / us["adam_step"]
    # the claim: ours beats the like-for-like torch formulation (clip + Adam) by more than that baseline's own spread
    res["adam_step_beats_torch_clip_adam_beyond_its_spread"] = bool(
        us["torch_clip_adam"] - us["adam_step"] > spread("torch_clip_adam"))
    res["adam_step_beats_torch_adam_beyond_its_spread"] = bool(us["torch_adam"] - us["adam_step"] > spread("torch_adam"))
    res["adam_step_big_bytes_per_s"] = 28.0 * n_big / (us["adam_step_big"] * 1e-6)
    res["copy_big_bytes_per_s"] = 2.0 * copy_bytes / (us["copy_big"] * 1e-6)
    res["adam_step_big_over_copy_rate"] = res["adam_step_big_bytes_per_s"] / res["copy_big_bytes_per_s"]
    res["torch_randperm_over_permutation"] = us["torch_randperm"] / us["permutation"]
    res["former_loop_over_ppo_update"] = us["former_loop"] / us["ppo_update"]
    res["former_loop_over_ppo_update_graph"] = us["former_loop"] / us["ppo_update_graph"]
    res["checked"] = bool(err < 1e-5 and perm_ok and finite)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not res["checked"]:
        sys.exit("bench_helicopter_ppo_update.py: the step disagrees with the torch formulation, a row is no "
                 "permutation, or the statistics are not finite")


if __name__ == "__main__":
    main()
