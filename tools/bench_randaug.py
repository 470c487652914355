#!/usr/bin/env python3
"""Step time of device-side RandAugment (svit_amd/randaug.py) on the bench workload, in ONE process on one GPU (bench.py
itself measures the fp32-input step and stays as it is):

    A  none      augment.AugClips with randaug=None: the step before this feature, the baseline
    B  yaml      + tables drawn from the shipped yaml's `rand-m7-n4-mstd0.5-inc1`, bicubic (about half the layers skip)
    C  affine4   + four bicubic AFFINE layers on every clip: the worst case

    python tools/bench_randaug.py --steps 30 --warmup 5 --rounds 2

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward + clip + AdamW, hip-graph replay; the
sources are 8 uint8 videos of 16x240x320.  One model and one optimizer serve all arms; every arm owns a captured step.
The arms are timed in turn, `--rounds` times over, so that drift of the box shows up as spread between the rounds of one
arm; the cost of the feature is the same-process difference between an arm and A.  Also timed, stand-alone over
`--kernel-reps` launches between two events: the whole chain of arms B and C, and one stats / one apply launch per
operation on all 128 frames.  Prints one JSON line.  GPU box."""
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

ARMS = ("none", "yaml", "affine4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--source", default="240x320")
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--aa-type", default="rand-m7-n4-mstd0.5-inc1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_randaug.py measures on the GPU; none found")

    from svit_amd import config, hip, losses, optim, randaug
    from svit_amd.augment import AugClips, SpatialSampler
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
    g = torch.Generator().manual_seed(cfg.RNG_SEED)
    frames = torch.randint(0, 256, (B, T, Hs, Ws, 3), generator=g, dtype=torch.uint8).to(dev)
    y = torch.randint(0, cfg.MODEL.NUM_CLASSES, (B,), generator=g).to(dev)
    mean, std = cfg.DATA.MEAN, cfg.DATA.STD

    random.seed(cfg.RNG_SEED)
    np.random.seed(cfg.RNG_SEED)
    ra = randaug.RandAugSampler(args.aa_type, "bicubic")
    sp = SpatialSampler(S, scale=cfg.DATA.TRAIN_JITTER_SCALES_RELATIVE, aspect=cfg.DATA.TRAIN_JITTER_ASPECT_RELATIVE,
                        random_flip=cfg.DATA.RANDOM_FLIP)
    drawn, records = [], []
    for v in range(B):                      # per clip RandAugment first, then the spatial pipeline: the loader's order
        drawn.append(ra.draw(T, Hs, Ws, video=v))
        records.append(sp.draw(Hs, Ws, video=v))
    worst = [[randaug.make_op(name, (arg,), (1,) * T, Hs, Ws)
              for name, arg in (("Rotate", 21.0 - v), ("ShearX", 0.21), ("TranslateYRel", -0.3), ("ShearY", -0.2))]
             for v in range(B)]
    inputs = {"none": AugClips(frames, S, records, mean=mean, std=std),
              "yaml": AugClips(frames, S, records, mean=mean, std=std, randaug=drawn),
              "affine4": AugClips(frames, S, records, mean=mean, std=std, randaug=worst)}

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

    kernels = {"chain (yaml)": kernel_us(inputs["yaml"].run_randaug),
               "chain (affine4)": kernel_us(inputs["affine4"].run_randaug)}
    one = {"none": randaug.RandAugOp(), "autocontrast": randaug.RandAugOp(randaug.OP_AUTOCONTRAST),
           "equalize": randaug.RandAugOp(randaug.OP_EQUALIZE), "contrast": randaug.RandAugOp(randaug.OP_CONTRAST, arg_f=1.63),
           "posterize": randaug.RandAugOp(randaug.OP_POSTERIZE, arg_i=2),
           "color": randaug.RandAugOp(randaug.OP_COLOR, arg_f=1.63),
           "sharpness": randaug.RandAugOp(randaug.OP_SHARPNESS, arg_f=1.63),
           "affine bilinear": randaug.make_op("Rotate", (21.0,), (0,) * T, Hs, Ws),
           "affine bicubic": randaug.make_op("Rotate", (21.0,), (1,) * T, Hs, Ws)}
    dst = torch.empty_like(frames)
    ws = torch.empty(randaug.workspace_bytes(B, T), dtype=torch.uint8, device=dev)
    for name, op in one.items():
        table = torch.from_numpy(randaug.pack_table([[op]] * B)).to(dev)
        kernels["stats (%s)" % name] = kernel_us(lambda: hip.call(
            "svit_randaug_stats", hip.ptr(frames), hip.ptr(table), 0, hip.ptr(ws), B, T, Hs, Ws, 1))
        kernels["apply (%s)" % name] = kernel_us(lambda: hip.call(
            "svit_randaug_apply", hip.ptr(frames), hip.ptr(dst), hip.ptr(table), 0, hip.ptr(ws), B, T, Hs, Ws, 1))

    base = min(ms["none"])
    out = {"workload": "SViT %dx%d^2 bf16, %d clips from uint8 %dx%d sources, fwd+CE+bwd+clip+AdamW, hip-graph replay"
                       % (T, S, B, Hs, Ws),
           "aa_type": args.aa_type, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "ms_per_step": ms,
           "ms_per_step_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()}, "loss": loss,
           "n_graphs": {a: graphed[a].n_graphs for a in ARMS}, "kernel_us": kernels,
           "ops_drawn": [[o.op for o in layers] for layers in drawn],
           "cost_vs_none": {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                            for a, v in ms.items() if a != "none"}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
