#!/usr/bin/env python3
"""Cost of the SGD and Adam tails (SOLVER.OPTIMIZING_METHOD sgd / adam: csrc/solver.hip) beside the AdamW tail on the
bench workload, in ONE process on one GPU (bench.py itself measures the adamw step and stays as it is):

    python tools/bench_solvers.py --steps 30 --warmup 5 --rounds 2

(i) the guarded tail alone, from HIP events around back-to-back launches on the gradients of the last step:

    guard       svit_step_guard alone (every arm below starts with it)
    adamw       svit_step_guard + svit_adamw_step_guarded                  32 B per parameter with the guard's read
    adam        svit_step_guard + svit_adam_step_guarded                   32 B
    sgd         svit_step_guard + svit_sgd_step_guarded, momentum 0.9      24 B
    sgd_m0      the same with momentum 0, no buffer                        16 B

(ii) the whole captured step (B = 8 clips of 16x224^2, bf16, forward + CE + backward + guarded clip + solver,
GraphedTrainStep(optimizer=...)) for adamw and for sgd: each arm its own model, optimizer and capture, the same weights
and batch.

The arms of each part are timed in turn, `--rounds` times over: drift of the box shows as spread between the rounds of
one arm.  Every timed tail launch must have been an APPLIED step (a dropped one returns before its first load and would
time nothing): the counters are checked.  Prints one JSON line.  GPU box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="tail launches per timing")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_solvers.py measures on the GPU; none found")

    import bench
    from svit_amd import config, losses, ops, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    kinds = {"adamw": optim.GuardedClipAdamW, "sgd": optim.GuardedClipSGD}
    rigs, w0, x, y = {}, None, None, None
    for arm in kinds:
        cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
        cfg.SVIT.GUARDED_STEP = True
        cfg.SOLVER.OPTIMIZING_METHOD = arm          # (sgd: the default tree's MOMENTUM 0.9, NESTEROV, the recipe's rates)
        if x is None:
            x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)
        torch.manual_seed(cfg.RNG_SEED)
        model = build_model(cfg, gpu_id=0)
        model.train()
        if w0 is None:
            w0 = model.flat.data.clone()
        model.flat.data.copy_(w0)
        opt = optim.construct_optimizer(model, cfg)
        assert type(opt) is kinds[arm]
        step = GraphedTrainStep(model, ce, [x], y, optimizer=opt, warmup=2)
        torch.cuda.synchronize()
        state = [getattr(opt, k) for k in opt.STATE]
        rigs[arm] = dict(cfg=cfg, model=model, opt=opt, step=step, start=[(t, t.clone()) for t in [model.flat.data] + state])

    def timed(arm):
        r = rigs[arm]
        g, opt, cfg = r["step"], r["opt"], r["cfg"]
        for t, saved in r["start"]:
            t.copy_(saved)
        opt.step_count = 0
        xs, ys = g.static_inputs[0], g.static_labels
        xs.copy_(x)
        for it in range(args.warmup):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, it / 1000.0))
            g([xs], ys)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.steps):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (args.warmup + it) / 1000.0))
            loss, _ = g([xs], ys)
        torch.cuda.synchronize()
        assert opt.stats()["applied"] == args.warmup + args.steps
        return (time.perf_counter() - t0) / args.steps * 1e3, float(loss)

    step_ms, loss = {a: [] for a in rigs}, {}
    for _ in range(args.rounds):
        for arm in rigs:
            t, loss[arm] = timed(arm)
            step_ms[arm].append(round(t, 3))

    # ---- the tails alone, each optimizer over the sgd arm's model (gradients of its last replay) ----
    model = rigs["sgd"]["model"]
    lr, wd = rigs["sgd"]["cfg"].SOLVER.BASE_LR, rigs["sgd"]["cfg"].SOLVER.WEIGHT_DECAY
    common = dict(lr=lr, weight_decay=wd, clip_grad_l2norm=1.0)
    tails = {"adamw": optim.GuardedClipAdamW(model, **common), "adam": optim.GuardedClipAdam(model, **common),
             "sgd": rigs["sgd"]["opt"], "sgd_m0": optim.GuardedClipSGD(model, momentum=0.0, **common)}
    guard_opt = tails["adamw"]
    f = model.flat

    def guard_alone():
        ops.step_guard(f.grad, guard_opt.host_rec, guard_opt.dev_rec, guard_opt.bias_table, guard_opt._ws)

    def tail_alone(opt, enqueue):
        opt.upload()
        before = opt.stats()["applied"]
        for _ in range(3):
            enqueue()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            enqueue()
        e1.record()
        torch.cuda.synchronize()
        assert opt.stats()["applied"] == before + 3 + args.reps, "a timed step was dropped"
        return round(e0.elapsed_time(e1) / args.reps * 1e3, 2)

    tail_us = {k: [] for k in ["guard"] + list(tails)}
    for _ in range(args.rounds):
        tail_us["guard"].append(tail_alone(guard_opt, guard_alone))
        for k, opt in tails.items():
            tail_us[k].append(tail_alone(opt, opt.enqueue))

    best = {k: min(v) for k, v in tail_us.items()}
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+guarded clip+solver in one captured step"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "reps": args.reps,
           "parameters": int(f.total), "tail_alone_us": tail_us, "tail_alone_us_best": best,
           "tail_vs_adamw": {k: round(best[k] / best["adamw"], 3) for k in tails},
           "update_alone_vs_adamw": {k: round((best[k] - best["guard"]) / (best["adamw"] - best["guard"]), 3) for k in tails},
           "step_ms": step_ms, "step_ms_best": {a: min(v) for a, v in step_ms.items()},
           "step_spread_ms": {a: round(max(v) - min(v), 3) for a, v in step_ms.items()}, "loss": loss}
    base = min(step_ms["adamw"])
    out["sgd_vs_adamw"] = {"ms": round(min(step_ms["sgd"]) - base, 3),
                           "pct": round((min(step_ms["sgd"]) / base - 1) * 100, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
