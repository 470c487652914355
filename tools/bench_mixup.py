#!/usr/bin/env python3
"""Step time with and without cfg.MIXUP on the bench workload, in ONE process on one GPU (bench.py itself measures the
unmixed step only and stays as it is):

    none      GraphedTrainStep(..., mixup=None): the step bench.py times
    mixup     every step a mixup record   (lam 0.3: the clip kernel blends all B clips)
    cutmix    every step a CutMix record  (a centred box of a quarter of the frame, area-corrected lam 0.75)

    python tools/bench_mixup.py --steps 30 --warmup 5 --rounds 2
    python tools/bench_mixup.py --arms mixup,cutmix --rounds 1 --steps 5           # under rocprofv3 --kernel-trace --stats

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward + clip + AdamW, hip-graph replay.  One
model and one optimizer serve all arms; every arm owns a captured step.  The arms are timed in turn, `--rounds` times over,
so that drift of the box shows up as spread between the rounds of one arm; the cost of the feature is the same-process
difference between an arm and `none`.  The mixed arms pass their record to every call (the 32-byte upload is part of
what is timed) and mix the static input where it lies, step after step -- fine for a timing, not a training run.
Prints one JSON line, with the bytes the clip kernel has to move per step (for a GB/s figure over a profiler's kernel
time).  GPU box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

ARMS = ("none", "mixup", "cutmix")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--arms", default=",".join(ARMS))
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]
    if any(a not in ARMS for a in arms):
        raise SystemExit("--arms: any of %s" % ", ".join(ARMS))
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixup.py measures on the GPU; none found")

    import bench
    from svit_amd import config, losses, mixup, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0)
    model.train()
    opt = optim.construct_optimizer(model, cfg)
    x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)
    fn = mixup.MixUp(0.8, 1.0, label_smoothing=0.1, num_classes=cfg.MODEL.NUM_CLASSES)
    S = args.crop
    q = S // 4
    records = {"none": None, "mixup": mixup.MixRecord(mixup.MODE_MIXUP, 0.3, 0, 0, 0, 0),
               "cutmix": mixup.MixRecord(mixup.MODE_CUTMIX, 1.0 - (S - 2 * q) ** 2 / float(S * S), q, S - q, q, S - q)}

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    graphed = {arm: GraphedTrainStep(model, ce, [x], y, mixup=None if arm == "none" else fn) for arm in arms}
    start = [(t, t.clone()) for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)]

    def timed(arm):
        """-> ms per step of `arm`: every leg starts from the same weights, optimizer state and batch"""
        g, rec = graphed[arm], records[arm]
        for t, saved in start:
            t.copy_(saved)
        opt.step_count = 0
        xs, ys = g.static_inputs[0], g.static_labels
        xs.copy_(x)
        kw = {} if rec is None else {"mix": rec}
        for it in range(args.warmup):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, it / 1000.0))
            g([xs], ys, **kw)
            opt.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.steps):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (args.warmup + it) / 1000.0))
            loss, _ = g([xs], ys, **kw)
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, float(loss)

    ms = {a: [] for a in arms}
    loss = {}
    for r in range(args.rounds):
        for arm in arms:
            t, loss[arm] = timed(arm)
            ms[arm].append(round(t, 3))
    clip_bytes = args.batch * 3 * args.frames * S * S * 4
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+clip+AdamW, hip-graph replay"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "ms_per_step": ms,
           "ms_per_step_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()}, "loss": loss,
           "n_graphs": {a: graphed[a].n_graphs for a in arms},
           # what svit_mixup_clips has to read + write per step (mixup: every element; CutMix: the box of every plane)
           "clip_kernel_bytes": {"mixup": 2 * clip_bytes, "cutmix": 2 * clip_bytes * (S - 2 * q) ** 2 // (S * S)}}
    if "none" in ms:
        base = min(ms["none"])
        out["cost_vs_none"] = {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                               for a, v in ms.items() if a != "none"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
