#!/usr/bin/env python
"""What the reference's clipped value loss costs the learner: <Agent>Policy.ppo_grad plain (four launches) and with
clip_vloss=True (eight: gca_*_policy_grad_vclip) in the same process, at the two README shapes,
  helicopter  4096 envs x 42 x 42, K = 128, N = 131072 samples, 64 hidden units
  bulldozer   1024 envs x 256 x 256, K = 128, N = 32768 samples (one of four minibatches), C = 2048 coarse values
and the whole HelicopterPolicy.ppo_update (4 epochs x 4 minibatches, eager) both ways at the helicopter shape. The
clipped call is checked in the run against the same loss through forward_torch and backward() on 8192 rows.
Timed with HIP events. Prints one JSON line; --out also writes it.

    python scripts/bench_ppo_vclip.py --out profiles/ppo_vclip.json

Protocol (scripts/bench_helicopter_policy_grad.py's): every variant is warmed up, then `passes` rounds visit the
variants in turn (interleaved), each timing `reps` repetitions between two events; the figure of a variant is the median
over its rounds, in microseconds per call, and the rounds' (min, max) is recorded. Needs a HIP device; there is no CPU
fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-cellular-automata_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HELI = {"E": 4096, "H": 42, "W": 42, "K": 128, "radius": 5, "block": 8, "hidden": 64, "N": 131072}
BDZ = {"E": 1024, "H": 256, "W": 256, "K": 128, "radius": 5, "block": 8, "hidden": 64, "N": 32768}
COEF = dict(clip_coef=0.2, ent_coef=0.01, vf_coef=0.5)
EPOCHS, MINIBATCHES = 4, 4
N_CHECK = 8192


def time_once(fn, reps):
    import torch

    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def torch_clipped_loss(pol, leaves, rec, adv, ret, idx):
    """include/gca.h's loss with the clipped value term, in torch ops on rows idx (one or two heads)."""
    import torch

    flat = lambda t: t.reshape((-1,) + tuple(t.shape[2:]))
    i = idx.long()
    *heads, value = pol.forward_torch(flat(rec["local"])[i], flat(rec["coarse"])[i], weights=leaves)
    act = flat(rec["action"])[i].long().reshape(len(i), -1)
    old = flat(rec["logits"])[i]
    logratio, ent, off = [], [], 0
    for h, new in enumerate(heads):
        n = new.shape[1]
        lp, lo = torch.log_softmax(new, 1), torch.log_softmax(old[:, off:off + n], 1)
        a = act[:, h:h + 1]
        logratio.append((lp.gather(1, a) - lo.gather(1, a))[:, 0])
        ent.append(-(lp.exp() * lp).sum(1))
        off += n
    ratio, ent = torch.stack(logratio, 1).exp(), torch.stack(ent, 1)
    A = adv.reshape(-1)[i]
    A = ((A - A.mean()) / (A.std(unbiased=False) + 1e-8))[:, None]
    c = COEF["clip_coef"]
    pg = torch.maximum(-A * ratio, -A * ratio.clamp(1 - c, 1 + c)).mean()
    R, vo = ret.reshape(-1)[i], rec["value"].reshape(-1)[i]
    unclipped = 0.5 * ((value - R) ** 2).mean()  # the mean BEFORE the maximum
    clipped = (vo + (value - vo).clamp(-c, c) - R) ** 2
    v_loss = 0.5 * torch.maximum(unclipped, clipped).mean()
    return pg - COEF["ent_coef"] * ent.mean() + COEF["vf_coef"] * v_loss


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if min(args.reps, args.passes, args.warmup) < 1:
        sys.exit("bench_ppo_vclip.py: every count must be >= 1")
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_ppo_vclip.py needs a HIP device (no CPU fallback, no figure without a GPU run)")
    from gymca_amd.forest_fire import ppo
    from gymca_amd.forest_fire._policy import WEIGHTS
    from gymca_amd.forest_fire.bulldozer import BatchedForestFireBulldozerEnv, BulldozerPolicy
    from gymca_amd.forest_fire.helicopter import BatchedForestFireHelicopterEnv, HelicopterPolicy

    device = torch.device("cuda", 0)
    fns, keep, checks = {}, {}, {}

    def setup(name, cfg, env, pol_cls, next_value_of, terminal_of):
        E, K, N = cfg["E"], cfg["K"], cfg["N"]
        T = E * K
        env.reset()
        make = lambda: pol_cls(env, cfg["radius"], cfg["block"], cfg["hidden"], seed=3)
        pol = make()
        rec = env.rollout_policy(pol, K, seed=5)
        adv, ret = ppo.gae(rec["reward"], rec["value"], next_value_of(pol), 0.99, 0.95, terminal=terminal_of(rec))
        # the learner is a little ahead of the collector: the ratios are off 1, the values off their records
        gen = torch.Generator(device=device).manual_seed(7)
        for n in WEIGHTS:
            w = getattr(pol, n)
            w.add_(torch.randn(w.shape, generator=gen, device=device) * w.abs().mean() * 0.05)
        idx = torch.randperm(T, generator=gen, device=device)[:N].to(torch.int32).contiguous()
        grads = {n: torch.empty_like(getattr(pol, n)) for n in WEIGHTS}
        stats, vstats = torch.empty(8, device=device), torch.empty(3, device=device)
        ws = torch.empty_like(pol._ppo_workspace(N, None))
        fns[name + "_ppo_grad"] = lambda: pol.ppo_grad(rec, adv, ret, idx, grads_out=grads, stats_out=stats,
                                                       workspace=ws, **COEF)
        fns[name + "_ppo_grad_vclip"] = lambda: pol.ppo_grad(rec, adv, ret, idx, grads_out=grads, stats_out=stats,
                                                             workspace=ws, clip_vloss=True, vstats_out=vstats, **COEF)
        keep[name] = (pol, rec, adv, ret, make, vstats)
        # the check: the clipped call against autograd on N_CHECK rows
        rows = idx[:N_CHECK].contiguous()
        g, s, vs = pol.ppo_grad(rec, adv, ret, rows, clip_vloss=True, **COEF)
        leaves = {n: getattr(pol, n).clone().requires_grad_(True) for n in WEIGHTS}
        loss = torch_clipped_loss(pol, leaves, rec, adv, ret, rows)
        loss.backward()
        err = {n: float((g[n] - leaves[n].grad).abs().max() / leaves[n].grad.abs().max()) for n in WEIGHTS}
        checks[name] = {"grad_max_err_over_max_vs_torch": err, "loss_torch": float(loss.detach()),
                        "loss_ppo_grad": float(s[0]), "vstats": dict(zip(ppo.VSTATS, [float(x) for x in vs.cpu()]))}
        del leaves, loss

    henv = BatchedForestFireHelicopterEnv(HELI["E"], HELI["H"], HELI["W"], device=device, seed=1, materialize_obs=False)
    setup("helicopter", HELI, henv, HelicopterPolicy, lambda pol: henv.act(pol, seed=5)[2], lambda rec: None)
    benv = BatchedForestFireBulldozerEnv(BDZ["E"], BDZ["H"], BDZ["W"], device=device, seed=1, materialize_obs=False,
                                         autoreset=True, max_episode_steps=200)
    setup("bulldozer", BDZ, benv, BulldozerPolicy, lambda pol: benv.act(pol, seed=5)[2],
          lambda rec: rec["terminated"] | rec["truncated"])

    # the whole update at the helicopter shape, eager, both ways
    pol, rec, adv, ret, make, _ = keep["helicopter"]
    T = HELI["E"] * HELI["K"]
    steps = EPOCHS * MINIBATCHES

    def update_setup(clip):
        p = make()
        o = ppo.Adam({n: getattr(p, n) for n in WEIGHTS}, lr=2.5e-4)
        bufs = dict(stats_out=torch.empty((steps, 8), device=device), info_out=torch.empty((steps, 2), device=device),
                    perm_out=torch.empty((EPOCHS, T), dtype=torch.int32, device=device),
                    grads_out={n: torch.empty_like(getattr(p, n)) for n in WEIGHTS},
                    workspace=torch.empty_like(p._ppo_workspace(T // MINIBATCHES, None)))
        if clip:
            bufs.update(clip_vloss=True, vstats_out=torch.empty((steps, 3), device=device))
        return lambda: p.ppo_update(o, rec, adv, ret, epochs=EPOCHS, minibatches=MINIBATCHES, seed=1, **COEF, **bufs)

    fns["helicopter_ppo_update"] = update_setup(False)
    fns["helicopter_ppo_update_vclip"] = update_setup(True)

    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize(device)
    samples = {n: [] for n in fns}
    for _ in range(args.passes):
        for n, fn in fns.items():
            samples[n].append(time_once(fn, args.reps))
    us = {n: statistics.median(v) for n, v in samples.items()}
    res = {"bench": "ppo_vclip", "device": torch.cuda.get_device_name(0), "helicopter": HELI, "bulldozer": BDZ,
           "epochs": EPOCHS, "minibatches": MINIBATCHES, "reps": args.reps, "passes": args.passes, "warmup": args.warmup,
           "timing": "HIP events around `reps` calls; median over interleaved rounds; us per call",
           "check_rows": N_CHECK, "check": checks}
    for n, v in us.items():
        res[f"{n}_us"] = v
        res[f"{n}_spread"] = [min(samples[n]), max(samples[n])]
    for name in ("helicopter_ppo_grad", "bulldozer_ppo_grad", "helicopter_ppo_update"):
        res[f"{name}_vclip_over_plain"] = us[name + "_vclip"] / us[name]
    res["checked"] = bool(all(max(c["grad_max_err_over_max_vs_torch"].values()) < 1e-3 and
                              abs(c["loss_torch"] - c["loss_ppo_grad"]) < 1e-4 * max(1.0, abs(c["loss_torch"]))
                              for c in checks.values()))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if not res["checked"]:
        sys.exit("bench_ppo_vclip.py: the clipped call disagrees with the torch yardstick")


if __name__ == "__main__":
    main()
