#!/usr/bin/env python3
"""Step time of per-video extents on the uint8 input route (augment.AugClips(..., extents=)), in ONE process on one GPU
(bench.py itself measures the fp32-input step and stays as it is):

    A  none    AugClips with the yaml's RandAugment tables, extents=None: the plain entry points, the baseline
    B  full    + extents equal to the buffer: the `_ext` entry points on the same pixels
    C  mixed   + videos of 240 x {320, 300, 284, 256} in the same 240 x 320 buffer, tables and records drawn per size

    python tools/bench_ragged.py --steps 30 --warmup 5 --rounds 2

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward + clip + AdamW, hip-graph replay; the
sources are 8 uint8 videos in a 16x240x320 buffer.  One model and one optimizer serve all arms; every arm owns a captured
step.  Every arm draws from the same seed, so the same operations are drawn for every clip (only the affine matrices and
the crop rectangles follow the sizes).  The arms are timed in turn, `--rounds` times over, so that drift of the box shows
up as spread between the rounds of one arm; the cost of the feature is the same-process difference between an arm and A.
Also timed, stand-alone over `--kernel-reps` launches between two events: the RandAugment chain and the im2col of each
arm.  Prints one JSON line.  GPU box."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

ARMS = ("none", "full", "mixed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--source", default="240x320")
    ap.add_argument("--widths", default="320,300,284,256")
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--aa-type", default="rand-m7-n4-mstd0.5-inc1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged.py measures on the GPU; none found")

    from svit_amd import config, losses, ops, optim, randaug
    from svit_amd.augment import AugClips, SpatialSampler, pack_videos
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0)
    model.train()
    opt = optim.construct_optimizer(model, cfg)
    B, T, S = args.batch, args.frames, args.crop
    Hs, Ws = (int(v) for v in args.source.split("x"))
    widths = [int(w) for w in args.widths.split(",")]
    g = torch.Generator().manual_seed(cfg.RNG_SEED)
    frames = torch.randint(0, 256, (B, T, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    y = torch.randint(0, cfg.MODEL.NUM_CLASSES, (B,), generator=g).to(dev)
    mean, std = cfg.DATA.MEAN, cfg.DATA.STD

    def draw(sizes):
        """per clip RandAugment first, then the spatial pipeline (the loader's order), each for the clip's own size"""
        random.seed(cfg.RNG_SEED)
        np.random.seed(cfg.RNG_SEED)
        ra = randaug.RandAugSampler(args.aa_type, "bicubic")
        sp = SpatialSampler(S, scale=cfg.DATA.TRAIN_JITTER_SCALES_RELATIVE, aspect=cfg.DATA.TRAIN_JITTER_ASPECT_RELATIVE,
                            random_flip=cfg.DATA.RANDOM_FLIP)
        drawn, records = [], []
        for v, (h, w) in enumerate(sizes):
            drawn.append(ra.draw(T, h, w, video=v))
            records.append(sp.draw(h, w, video=v))
        return drawn, records

    full = [(Hs, Ws)] * B
    mixed = [(Hs, widths[v % len(widths)]) for v in range(B)]
    drawn, records = draw(full)
    drawn_m, records_m = draw(mixed)
    # the mixed batch as a loader assembles it: the same videos cut to their widths, zero-padded into the buffer
    frames_m, extents_m = pack_videos([frames[v, :, :h, :w].contiguous() for v, (h, w) in enumerate(mixed)], Hs=Hs, Ws=Ws)
    inputs = {"none": AugClips(frames.to(dev), S, records, mean=mean, std=std, randaug=drawn),
              "full": AugClips(frames.to(dev), S, records, mean=mean, std=std, randaug=drawn, extents=full),
              "mixed": AugClips(frames_m.to(dev), S, records_m, mean=mean, std=std, randaug=drawn_m, extents=extents_m)}

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    ms = {a: [] for a in ARMS}
    loss = {}
    graphed = {arm: GraphedTrainStep(model, ce, [inputs[arm]], y) for arm in ARMS}
    start = [(t, t.clone()) for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)]

    def timed(arm):
        """-> ms per step of `arm`: every leg starts from the same weights, optimizer state and batch"""
        step = graphed[arm]
        for t, saved in start:
            t.copy_(saved)
        opt.step_count = 0
        xs, ys = step.static_inputs[0], step.static_labels
        for it in range(args.warmup):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, it / 1000.0))
            step([xs], ys)
            opt.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.steps):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (args.warmup + it) / 1000.0))
            out, _ = step([xs], ys)
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, float(out)

    for r in range(args.rounds):
        for arm in ARMS:
            t, loss[arm] = timed(arm)
            ms[arm].append(round(t, 3))

    def kernel_us(fn_):
        for _ in range(5):
            fn_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.kernel_reps):
            fn_()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.kernel_reps * 1e3, 1)

    kernels = {}
    for r in range(args.rounds):
        for arm in ARMS:
            clips = inputs[arm]
            kernels.setdefault("chain (%s)" % arm, []).append(kernel_us(clips.run_randaug))
            kernels.setdefault("im2col (%s)" % arm, []).append(kernel_us(lambda: ops._im2col_u8(
                "svit_im2col_patch_u8_aug", clips.frames, clips.lut_f32, clips.records, S, (None,), extents=clips.extents)))

    base = min(ms["none"])
    out = {"workload": "SViT %dx%d^2 bf16, %d clips from a uint8 %dx%d buffer, fwd+CE+bwd+clip+AdamW, hip-graph replay"
                       % (T, S, B, Hs, Ws),
           "aa_type": args.aa_type, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "extents": {"full": full, "mixed": mixed}, "ms_per_step": ms,
           "ms_per_step_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()}, "loss": loss,
           "n_graphs": {a: graphed[a].n_graphs for a in ARMS}, "kernel_us": kernels,
           "ops_drawn": {"full": [[o.op for o in layers] for layers in drawn],
                         "mixed": [[o.op for o in layers] for layers in drawn_m]},
           "cost_vs_none": {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                            for a, v in ms.items() if a != "none"}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
