#!/usr/bin/env python3
"""Step time of the device-side augmentation (svit_amd/augment.py) on the bench workload, in ONE process on one GPU
(bench.py itself measures the fp32-input step and stays as it is):

    plain          input.U8Clips: integer crops of uint8 frames (svit_im2col_patch_u8) -- the step before this feature
    aug            augment.AugClips with random-resized-crop records (svit_im2col_patch_u8_aug)
    aug_erase      the same + pixel-mode erasing on EVERY clip (RE_PROB 1: the worst case; the yaml's 0.25 erases a quarter)
    aug_erase_mix  the same + a mixup record (lam 0.3: every clip is sampled twice)

    python tools/bench_augment.py --steps 30 --warmup 5 --rounds 2

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward + clip + AdamW, hip-graph replay; the
sources are 8 uint8 videos of 16x240x320.  One model and one optimizer serve all arms; every arm owns a captured step.
The arms are timed in turn, `--rounds` times over, so that drift of the box shows up as spread between the rounds of one
arm; the cost of the feature is the same-process difference between an arm and `plain`.  Also timed, stand-alone over
`--kernel-reps` launches between two events: the im2col kernel of every arm, and the UNFUSED alternative (svit_u8_clips_render
to an fp32 clip + svit_im2col_patch).  `--kernels-only --arms plain,aug` launches just those, for a profiler's kernel
times (the three aug arms share one kernel name: profile them one at a time).  Prints one JSON line.  GPU box."""
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

ARMS = ("plain", "aug", "aug_erase", "aug_erase_mix")


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
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--kernels-only", action="store_true",
                    help="launch only the stand-alone kernels of --arms (for a rocprofv3 --kernel-trace --stats run)")
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]
    if any(a not in ARMS for a in arms):
        raise SystemExit("--arms: any of %s" % ", ".join(ARMS))
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py measures on the GPU; none found")

    from svit_amd import config, losses, mixup, ops, optim
    from svit_amd.augment import AugClips, SpatialSampler
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.input import U8Clips
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
    fn = mixup.MixUp(0.8, 1.0, label_smoothing=0.1, num_classes=cfg.MODEL.NUM_CLASSES)
    mean, std = cfg.DATA.MEAN, cfg.DATA.STD

    def records(re_prob):
        random.seed(cfg.RNG_SEED)
        np.random.seed(cfg.RNG_SEED)
        sp = SpatialSampler(S, scale=cfg.DATA.TRAIN_JITTER_SCALES_RELATIVE, aspect=cfg.DATA.TRAIN_JITTER_ASPECT_RELATIVE,
                            random_flip=cfg.DATA.RANDOM_FLIP, re_prob=re_prob, re_mode="pixel")
        return [sp.draw(Hs, Ws, video=v) for v in range(B)]

    crops = torch.tensor([[v, (7 * v) % (Hs - S + 1), (13 * v) % (Ws - S + 1)] for v in range(B)], dtype=torch.int32)
    inputs = {"plain": U8Clips(frames, S, crops, mean=mean, std=std),
              "aug": AugClips(frames, S, records(0.0), mean=mean, std=std),
              "aug_erase": AugClips(frames, S, records(1.0), mean=mean, std=std),
              "aug_erase_mix": AugClips(frames, S, records(1.0), mean=mean, std=std)}
    mix = {"aug_erase_mix": mixup.MixRecord(mixup.MODE_MIXUP, 0.3, 0, 0, 0, 0)}

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    ms = {a: [] for a in arms}
    loss, graphed = {}, {}
    if not args.kernels_only:
        graphed = {arm: GraphedTrainStep(model, ce, [inputs[arm]], y, mixup=fn if arm in mix else None) for arm in arms}
        start = [(t, t.clone()) for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)]

    def timed(arm):
        """-> ms per step of `arm`: every leg starts from the same weights, optimizer state and batch"""
        step = graphed[arm]
        for t, saved in start:
            t.copy_(saved)
        opt.step_count = 0
        xs, ys = step.static_inputs[0], step.static_labels
        kw = {"mix": mix[arm]} if arm in mix else {}
        for it in range(args.warmup):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, it / 1000.0))
            step([xs], ys, **kw)
            opt.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.steps):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (args.warmup + it) / 1000.0))
            loss, _ = step([xs], ys, **kw)
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, float(loss)

    for r in range(0 if args.kernels_only else args.rounds):
        for arm in arms:
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

    inputs["aug_erase_mix"].mix = torch.from_numpy(mix["aug_erase_mix"].pack()).to(dev)
    kernels = {}
    if "plain" in arms:
        kernels["im2col_patch_u8 (plain)"] = kernel_us(lambda: ops.im2col_patch_u8(inputs["plain"]))
    for arm in arms:
        if arm != "plain":
            kernels["im2col_patch_u8_aug (%s)" % arm] = kernel_us(lambda: ops.im2col_patch_u8_aug(inputs[arm]))
    if "aug" in arms:
        kernels["u8_clips_render (aug)"] = kernel_us(lambda: ops.u8_clips_render(inputs["aug"]))
        clip = ops.u8_clips_render(inputs["aug"])
        kernels["im2col_patch on the rendered fp32 clip"] = kernel_us(lambda: ops.im2col_patch(clip))
        kernels["unfused: render + im2col_patch (aug)"] = kernel_us(
            lambda: ops.im2col_patch(ops.u8_clips_render(inputs["aug"])))

    out = {"workload": "SViT %dx%d^2 bf16, %d clips from uint8 %dx%d sources, fwd+CE+bwd+clip+AdamW, hip-graph replay"
                       % (T, S, B, Hs, Ws),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "ms_per_step": ms,
           "ms_per_step_best": {a: min(v) for a, v in ms.items() if v},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items() if v}, "loss": loss,
           "n_graphs": {a: graphed[a].n_graphs for a in graphed}, "kernel_us": kernels,
           "records": {"aug": [list(r) for r in records(0.0)]}}
    if ms.get("plain"):
        base = min(ms["plain"])
        out["cost_vs_plain"] = {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                                for a, v in ms.items() if a != "plain"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
