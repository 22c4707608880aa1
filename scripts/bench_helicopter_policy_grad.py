#!/usr/bin/env python
"""The learner's side of the helicopter PPO loop on rollout_policy's records: forest_fire.ppo.gae (one launch of gca_gae)
and HelicopterPolicy.ppo_grad (gca_helicopter_policy_grad: loss, statistics and the five gradients in four launches) at
N = 131072 samples under a permuted index, against
  (a) the same loss in torch from forward_torch with leaf weights plus backward(), at the largest N <= 131072 that fits
      (reported per sample, and checked against ppo_grad in the run),
  (b) a K-step torch GAE loop.
All in one process, timed with HIP events. Prints one JSON line; --out also writes it.

    python scripts/bench_helicopter_policy_grad.py --out profiles/helicopter_policy_grad.json

Protocol: every variant is warmed up, then `passes` passes visit the variants in turn (interleaved), each timing `reps`
repetitions between two events; the figure of a variant is the median over its passes, in microseconds per call. No
ratio is fixed in advance: the measured ones are recorded. Needs a HIP device; there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIG = {"E": 4096, "H": 42, "W": 42, "K": 128, "radius": 5, "block": 8, "hidden": 64, "N": 131072}
COEF = dict(clip_coef=0.2, ent_coef=0.01, vf_coef=0.5)


def time_once(fn, reps):
    import torch

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def torch_loss(pol, leaves, rec, adv, ret, idx):
    """gca.h's loss in torch ops on rows idx, from forward_torch with the trainer's leaf weights."""
    import torch

    flat = lambda t: t.reshape((-1,) + tuple(t.shape[2:]))
    i = idx.long()
    logits, value = pol.forward_torch(flat(rec["local"])[i], flat(rec["coarse"])[i], weights=leaves)
    act = flat(rec["action"])[i].long()[:, None]
    logp = torch.log_softmax(logits, 1)
    logratio = logp.gather(1, act)[:, 0] - torch.log_softmax(flat(rec["logits"])[i], 1).gather(1, act)[:, 0]
    ratio = torch.exp(logratio)
    A = adv.reshape(-1)[i]
    A = (A - A.mean()) / (A.std(unbiased=False) + 1e-8)
    c = COEF["clip_coef"]
    pg = torch.maximum(-A * ratio, -A * torch.clamp(ratio, 1 - c, 1 + c)).mean()
    vl = (0.5 * (value - ret.reshape(-1)[i]) ** 2).mean()
    ent = (-(torch.exp(logp) * logp).sum(1)).mean()
    return pg - COEF["ent_coef"] * ent + COEF["vf_coef"] * vl


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--envs", type=int, default=CONFIG["E"])
    ap.add_argument("--steps", type=int, default=CONFIG["K"])
    ap.add_argument("--samples", type=int, default=CONFIG["N"], help="minibatch size N (at most envs * steps)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if min(args.reps, args.passes, args.warmup, args.envs, args.steps, args.samples) < 1:
        sys.exit("bench_helicopter_policy_grad.py: every count must be >= 1")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_helicopter_policy_grad.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv, HelicopterPolicy
    from gymca_amd.forest_fire.helicopter.policy import WEIGHTS

    device = torch.device("cuda", 0)
    E, K = args.envs, args.steps
    T = E * K
    N = min(args.samples, T)
    env = BatchedForestFireHelicopterEnv(E, CONFIG["H"], CONFIG["W"], device=device, seed=1, materialize_obs=False)
    env.reset()
    pol = HelicopterPolicy(env, CONFIG["radius"], CONFIG["block"], CONFIG["hidden"], seed=3)
    rec = env.rollout_policy(pol, K, seed=5)
    _, _, next_value = env.act(pol, seed=5)
    # the learner is a little ahead of the collector: the ratios are off 1
    gen = torch.Generator(device=device).manual_seed(7)
    for n in WEIGHTS:
        w = getattr(pol, n)
        w.add_(torch.randn(w.shape, generator=gen, device=device) * w.abs().mean() * 0.05)
    adv, ret = torch.empty((K, E), device=device), torch.empty((K, E), device=device)
    idx = torch.randperm(T, generator=gen, device=device)[:N].to(torch.int32).contiguous()
    grads = {n: torch.empty_like(getattr(pol, n)) for n in WEIGHTS}
    stats = torch.empty(8, device=device)

    def torch_gae():
        A = torch.zeros(E, device=device)
        out = torch.empty((K, E), device=device)
        nv = next_value
        for k in range(K - 1, -1, -1):
            delta = rec["reward"][k].float() + 0.99 * nv - rec["value"][k]
            A = delta + 0.99 * 0.95 * A
            out[k] = A
            nv = rec["value"][k]
        return out, out + rec["value"]

    # the torch yardstick at the largest N that fits
    leaves = {n: getattr(pol, n).clone().requires_grad_(True) for n in WEIGHTS}
    n_torch = N
    while True:
        try:
            torch_loss(pol, leaves, rec, adv.zero_(), ret.zero_(), idx[:n_torch]).backward()
            torch.cuda.synchronize(device)
            break
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            n_torch //= 2
            if n_torch < 1:
                sys.exit("bench_helicopter_policy_grad.py: the torch yardstick fits at no N")
    idx_t = idx[:n_torch].contiguous()

    def torch_step():
        for t in leaves.values():
            t.grad = None
        torch_loss(pol, leaves, rec, adv, ret, idx_t).backward()

    fns = {"gae": lambda: ppo.gae(rec["reward"], rec["value"], next_value, 0.99, 0.95, adv_out=adv, ret_out=ret),
           "ppo_grad": lambda: pol.ppo_grad(rec, adv, ret, idx, grads_out=grads, stats_out=stats, **COEF),
           "torch_gae": torch_gae, "torch_loss_backward": torch_step}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize(device)
    samples = {n: [] for n in fns}
    for _ in range(args.passes):
        for n, fn in fns.items():
            samples[n].append(time_once(fn, args.reps))
    # the check in the run: ppo_grad on the yardstick's rows against torch's gradients and loss, and gae against the loop
    g2, s2 = pol.ppo_grad(rec, adv, ret, idx_t, **COEF)
    torch_step()
    loss_t = float(torch_loss(pol, leaves, rec, adv, ret, idx_t))
    err = {n: float((g2[n] - leaves[n].grad).abs().max() / leaves[n].grad.abs().max()) for n in WEIGHTS}
    ta, tr = torch_gae()
    gae_err = float((ta - adv).abs().max())
    us = {n: statistics.median(v) for n, v in samples.items()}
    st = [float(x) for x in stats.cpu()]
    res = {"bench": "helicopter_policy_grad", "device": torch.cuda.get_device_name(0), **CONFIG, "E": E, "K": K, "N": N,
           "N_torch": n_torch, "reps": args.reps, "passes": args.passes, "warmup": args.warmup,
           "timing": "HIP events around `reps` calls; median over interleaved passes; us per call",
           "workspace_bytes": int(pol._ppo_ws.numel()), "stats": dict(zip(ppo.STATS, st)),
           "grad_max_err_over_max_vs_torch": err, "loss_torch": loss_t, "loss_ppo_grad": float(s2[0]),
           "gae_max_abs_diff_vs_torch_loop": gae_err}
    for n, v in us.items():
        res[f"{n}_us"] = v
        res[f"{n}_spread"] = [min(samples[n]), max(samples[n])]
    res["ppo_grad_ns_per_sample"] = us["ppo_grad"] * 1e3 / N
    res["torch_ns_per_sample"] = us["torch_loss_backward"] * 1e3 / n_torch
    res["torch_over_ppo_grad_per_sample"] = res["torch_ns_per_sample"] / res["ppo_grad_ns_per_sample"]
    res["torch_gae_over_gae"] = us["torch_gae"] / us["gae"]
    res["checked"] = bool(max(err.values()) < 1e-3 and abs(loss_t - float(s2[0])) < 1e-4 * max(1.0, abs(loss_t))
                          and gae_err < 1e-4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not res["checked"]:
        sys.exit("bench_helicopter_policy_grad.py: ppo_grad / gae disagree with the torch yardstick")


if __name__ == "__main__":
    main()
