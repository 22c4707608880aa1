#!/usr/bin/env python
"""The bulldozer learner's step on the device against the same step through autograd, at the headline workload: 1024
envs x 256 x 256, K = 128 recorded steps (T = 131072 samples), radius 5, block 8, 64 hidden units (C = 2048 coarse
values), 4 epochs x 4 minibatches of N = 32768 samples.
  ppo_grad          BulldozerPolicy.ppo_grad on one minibatch (gca_bulldozer_policy_grad: four launches)
  autograd_grad     the same per-head loss through BulldozerPolicy.forward_torch and backward(), the five tensors cloned
                    as leaves, as scripts/train_bulldozer_ppo.py --autograd does it
  ppo_update        BulldozerPolicy.ppo_update, 16 x (ppo_grad + Adam.step) after one permutation launch, eager
  ppo_update_graph  the same captured once and replayed
  autograd_loop     the former loop: permutation, then 16 x (autograd_grad + Adam.step)
and the gradients of the two routes on one minibatch, as max |difference| over each tensor's max |gradient|.
All in one process, timed with HIP events. Prints one JSON line; --out also writes it.

    python scripts/bench_bulldozer_ppo_update.py --out profiles/bulldozer_ppo_update.json

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

CONFIG = {"E": 1024, "H": 256, "W": 256, "K": 128, "radius": 5, "block": 8, "hidden": 64, "epochs": 4, "minibatches": 4}
HYPER = dict(clip_coef=0.2, ent_coef=0.01, vf_coef=0.5)


def time_once(fn, reps):
    import torch

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def per_head_loss(policy, leaves, local, coarse, action, old_logits, adv, ret):
    """The loss of include/gca.h (gca_bulldozer_policy_grad) in torch ops: per head, every mean over (sample, head)."""
    import torch

    move, shoot, value = policy.forward_torch(local, coarse, weights=leaves)
    logratio, ent = [], []
    for h, (new, old) in enumerate(((move, old_logits[:, :9]), (shoot, old_logits[:, 9:]))):
        lp, lo = torch.log_softmax(new, -1), torch.log_softmax(old, -1)
        a = action[:, h].long().unsqueeze(-1)
        logratio.append((lp.gather(-1, a) - lo.gather(-1, a)).squeeze(-1))
        ent.append(-(lp.exp() * lp).sum(-1))
    ratio, ent = torch.stack(logratio, 1).exp(), torch.stack(ent, 1)
    a = ((adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)).unsqueeze(1)
    c = HYPER["clip_coef"]
    pg = torch.maximum(-a * ratio, -a * ratio.clamp(1 - c, 1 + c)).mean()
    v_loss = 0.5 * (value - ret).pow(2).mean()
    return pg - HYPER["ent_coef"] * ent.mean() + HYPER["vf_coef"] * v_loss


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--envs", type=int, default=CONFIG["E"])
    ap.add_argument("--steps", type=int, default=CONFIG["K"])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if min(args.reps, args.passes, args.warmup, args.envs, args.steps) < 1:
        sys.exit("bench_bulldozer_ppo_update.py: every count must be >= 1")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_bulldozer_ppo_update.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv, BulldozerPolicy
    from gymca_amd.forest_fire.bulldozer.policy import WEIGHTS

    device = torch.device("cuda", 0)
    E, K, epochs, mbs = args.envs, args.steps, CONFIG["epochs"], CONFIG["minibatches"]
    T = E * K
    if T % mbs:
        sys.exit("bench_bulldozer_ppo_update.py: envs * steps must divide into the minibatches")
    N, steps = T // mbs, epochs * mbs
    env = BatchedForestFireBulldozerEnv(E, CONFIG["H"], CONFIG["W"], device=device, seed=1, materialize_obs=False,
                                        autoreset=True, max_episode_steps=200)
    env.reset()
    make = lambda: BulldozerPolicy(env, CONFIG["radius"], CONFIG["block"], CONFIG["hidden"], seed=3)
    pol = make()
    rec = env.rollout_policy(pol, K, seed=5)
    _, _, next_value = env.act(pol, seed=5)
    adv, ret = ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95, terminal=rec["terminated"] | rec["truncated"])
    flat = lambda t: t.reshape((T,) + tuple(t.shape[2:]))
    local, coarse, action, old_logits = (flat(rec[k]) for k in ("local", "coarse", "action", "logits"))
    adv_f, ret_f = flat(adv), flat(ret)
    # the policy has moved a little since the rollout, as in every minibatch after the first
    gen = torch.Generator(device=device).manual_seed(7)
    for n in WEIGHTS:
        getattr(pol, n).add_(torch.randn(getattr(pol, n).shape, generator=gen, device=device) * 1e-3)
    w0 = {n: getattr(pol, n).clone() for n in WEIGHTS}
    perm = ppo.permutation(T, 1, seed=1, device=device)
    idx = perm[0, :N].contiguous()
    grads = {n: torch.empty_like(getattr(pol, n)) for n in WEIGHTS}
    stats = torch.empty(8, device=device)
    ws = torch.empty_like(pol._ppo_workspace(N, None))
    grad = lambda: pol.ppo_grad(rec, adv, ret, idx, grads_out=grads, stats_out=stats, workspace=ws, **HYPER)

    def autograd_grad(policy=pol, rows=idx):
        rows = rows.long()
        leaves = {n: getattr(policy, n).clone().requires_grad_(True) for n in WEIGHTS}
        loss = per_head_loss(policy, leaves, local[rows], coarse[rows], action[rows], old_logits[rows], adv_f[rows],
                             ret_f[rows])
        loss.backward()
        return {n: leaves[n].grad for n in WEIGHTS}, loss

    def update_setup():
        p = make()
        for n in WEIGHTS:
            getattr(p, n).copy_(w0[n])
        o = ppo.Adam({n: getattr(p, n) for n in WEIGHTS}, lr=2.5e-4)
        bufs = dict(stats_out=torch.empty((steps, 8), device=device), info_out=torch.empty((steps, 2), device=device),
                    perm_out=torch.empty((epochs, T), dtype=torch.int32, device=device),
                    grads_out={n: torch.empty_like(getattr(p, n)) for n in WEIGHTS}, workspace=torch.empty_like(ws))
        return p, o, bufs

    epol, eopt, ebufs = update_setup()
    update = lambda: epol.ppo_update(eopt, rec, adv, ret, epochs=epochs, minibatches=mbs, seed=1, **HYPER, **ebufs)
    gpol, gopt, gbufs = update_setup()
    gpol.ppo_update(gopt, rec, adv, ret, epochs=1, minibatches=mbs, seed=1, **HYPER)  # binds its calls before the capture
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gpol.ppo_update(gopt, rec, adv, ret, epochs=epochs, minibatches=mbs, seed=1, **HYPER, **gbufs)
    lpol, lopt, lbufs = update_setup()

    def autograd_loop():
        p = ppo.permutation(T, epochs, seed=1, counter=lopt.count, out=lbufs["perm_out"])
        for e in range(epochs):
            for mb in range(mbs):
                g, _ = autograd_grad(lpol, p[e, mb * N:(mb + 1) * N])
                lopt.step({n: g[n].contiguous() for n in WEIGHTS})

    fns = {"ppo_grad": grad, "autograd_grad": autograd_grad, "ppo_update": update, "ppo_update_graph": graph.replay,
           "autograd_loop": autograd_loop}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize(device)
    samples = {n: [] for n in fns}
    for _ in range(args.passes):
        for n, fn in fns.items():
            samples[n].append(time_once(fn, args.reps))
    us = {n: statistics.median(v) for n, v in samples.items()}
    # agreement of the two routes on one minibatch, and of the loss
    grad()
    ag, aloss = autograd_grad()
    agree = {n: float((grads[n] - ag[n]).abs().max() / ag[n].abs().max()) for n in WEIGHTS}
    loss_diff = abs(float(stats[0]) - float(aloss.detach()))
    finite = bool(torch.isfinite(ebufs["stats_out"]).all() and torch.isfinite(gbufs["stats_out"]).all())
    res = {"bench": "bulldozer_ppo_update", "device": torch.cuda.get_device_name(0), **CONFIG, "E": E, "K": K, "T": T,
           "N": N, "C": pol.C, "params": sum(getattr(pol, n).numel() for n in WEIGHTS), "reps": args.reps,
           "passes": args.passes, "warmup": args.warmup,
           "timing": "HIP events around `reps` calls; median over interleaved passes; us per call",
           "grad_max_err_over_max": agree, "loss_abs_diff": loss_diff, "ppo_workspace_bytes": int(ws.numel()),
           "last_stats": dict(zip(ppo.STATS, [float(x) for x in ebufs["stats_out"][-1].cpu()]))}
    for n, v in us.items():
        res[f"{n}_us"] = v
        res[f"{n}_spread"] = [min(samples[n]), max(samples[n])]
    res["autograd_grad_over_ppo_grad"] = us["autograd_grad"] / us["ppo_grad"]
    res["autograd_loop_over_ppo_update"] = us["autograd_loop"] / us["ppo_update"]
    res["autograd_loop_over_ppo_update_graph"] = us["autograd_loop"] / us["ppo_update_graph"]
    # the two matvec passes over the coarse map, N C Hd fma each in the forward and in the weight gradient
    res["coarse_fma_per_grad"] = 2 * N * pol.C * CONFIG["hidden"]
    res["ppo_grad_coarse_tflops"] = 2.0 * res["coarse_fma_per_grad"] / (us["ppo_grad"] * 1e-6) / 1e12
    res["checked"] = bool(max(agree.values()) < 1e-3 and loss_diff < 1e-4 and finite)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not res["checked"]:
        sys.exit("bench_bulldozer_ppo_update.py: the two routes' gradients or losses disagree, or the statistics are "
                 "not finite")


if __name__ == "__main__":
    main()
