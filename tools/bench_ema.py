#!/usr/bin/env python3
"""Cost of the weight EMA (SVIT.EMA_DECAY: svit_ema_step_guarded, csrc/solver.hip) on the bench workload, in ONE process
on one GPU (bench.py itself measures the step without the key and stays as it is):

    python tools/bench_ema.py --steps 30 --warmup 5 --rounds 2

(i) the guarded AdamW tail alone, from HIP events around back-to-back launches on the gradients of the last step:

    tail        svit_step_guard + svit_adamw_step_guarded                          32 B per parameter
    tail_ema    the same + svit_ema_step_guarded                                   44 B
    ema         svit_ema_step_guarded alone (p read, ema read and written)         12 B

(ii) the whole captured step (B = 8 clips of 16x224^2, bf16, forward + CE + backward + guarded clip + AdamW,
GraphedTrainStep(optimizer=...)) without and with the average attached: each arm its own model, optimizer and capture,
the same weights and batch.

The arms of each part are timed in turn, `--rounds` times over: drift of the box shows as spread between the rounds of
one arm.  Every timed launch must have been an APPLIED step (a dropped one returns before its first load and would time
nothing): the counters are checked.  Prints one JSON line.  GPU box."""
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
    ap.add_argument("--decay", type=float, default=0.9999)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema.py measures on the GPU; none found")

    import bench
    from svit_amd import config, ema, losses, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    rigs, w0, x, y = {}, None, None, None
    for arm in ("adamw", "adamw_ema"):
        cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
        cfg.SVIT.GUARDED_STEP = True
        if arm == "adamw_ema":
            cfg.SVIT.EMA_DECAY = args.decay
            cfg.SVIT.EMA_WARMUP = True
        if x is None:
            x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)
        torch.manual_seed(cfg.RNG_SEED)
        model = build_model(cfg, gpu_id=0)
        model.train()
        if w0 is None:
            w0 = model.flat.data.clone()
        model.flat.data.copy_(w0)
        opt = optim.construct_optimizer(model, cfg)
        assert type(opt) is optim.GuardedClipAdamW
        av = ema.build_ema(cfg, model, opt)
        assert (av is not None) == (arm == "adamw_ema") and opt.ema is av
        step = GraphedTrainStep(model, ce, [x], y, optimizer=opt, warmup=2)
        torch.cuda.synchronize()
        state = [getattr(opt, k) for k in opt.STATE]
        rigs[arm] = dict(cfg=cfg, model=model, opt=opt, ema=av, step=step,
                         start=[(t, t.clone()) for t in [model.flat.data] + state])

    def timed(arm):
        r = rigs[arm]
        g, opt, cfg = r["step"], r["opt"], r["cfg"]
        for t, saved in r["start"]:
            t.copy_(saved)
        opt.step_count = 0
        if r["ema"] is not None:
            r["ema"].reset()
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
        if r["ema"] is not None:
            assert r["ema"].stats()["num_updates"] == args.warmup + args.steps
        return (time.perf_counter() - t0) / args.steps * 1e3, float(loss)

    step_ms, loss = {a: [] for a in rigs}, {}
    for _ in range(args.rounds):
        for arm in rigs:
            t, loss[arm] = timed(arm)
            step_ms[arm].append(round(t, 3))

    # ---- the tails alone, over the EMA arm's model (gradients of its last replay) ----
    r = rigs["adamw_ema"]
    opt, av = r["opt"], r["ema"]

    def plain_tail():
        opt._solve()

    def tail_alone(enqueue, steps_per_call):
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
        assert opt.stats()["applied"] == before + (3 + args.reps) * steps_per_call, "a timed step was dropped"
        assert opt.dev_rec[5].item() == 1, "the record says the last step was dropped: the EMA launch would time nothing"
        return round(e0.elapsed_time(e1) / args.reps * 1e3, 2)

    arms = {"tail": (plain_tail, 1), "tail_ema": (opt.enqueue, 1), "ema": (av.enqueue, 0)}
    tail_us = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, (fn, n) in arms.items():
            tail_us[k].append(tail_alone(fn, n))

    best = {k: min(v) for k, v in tail_us.items()}
    n = int(r["model"].flat.total)
    base = min(step_ms["adamw"])
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+guarded clip+AdamW in one captured step"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "reps": args.reps, "decay": args.decay,
           "parameters": n, "tail_alone_us": tail_us, "tail_alone_us_best": best,
           "ema_bytes": 12 * n, "ema_tb_per_s": round(12 * n / (best["ema"] * 1e-6) / 1e12, 2),
           "step_ms": step_ms, "step_ms_best": {a: min(v) for a, v in step_ms.items()},
           "step_spread_ms": {a: round(max(v) - min(v), 3) for a, v in step_ms.items()}, "loss": loss,
           "ema_vs_adamw": {"ms": round(min(step_ms["adamw_ema"]) - base, 3),
                            "pct": round((min(step_ms["adamw_ema"]) / base - 1) * 100, 2)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
