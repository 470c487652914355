#!/usr/bin/env python3
"""Step time of the frames pass from uint8 clips (GraphedTrainStep(frames_pass="u8"), svit_amd/input.py FramesView) on
the bench workload, in ONE process on one GPU (bench.py itself measures the fp32-input step and stays as it is):

    render_fp32    the only way to run the recipe (AugClips input + the reference's frames pass) before the feature:
                   clips.render() eagerly every step (the 77 MB fp32 clip), then the replayed fp32 step with
                   frames_pass=True, which copies the clip into its static input and permutes it into B*T frames
    u8             the replayed AugClips step with frames_pass="u8": clip and frames operands both assembled from the
                   uint8 frames and the records, no fp32 clip

    python tools/bench_frames_u8.py --steps 30 --warmup 5 --rounds 2

The workload is bench.py's with --frames-pass: B = 8 clips of 16x224^2, bf16, forward + no-grad frames pass + CE +
backward + clip + AdamW, hip-graph replay; the sources are 8 uint8 videos of 16x240x320 with random-resized-crop records.
One model and one optimizer serve both arms; each arm owns a captured step.  The arms are timed in turn, `--rounds`
times over, so that drift of the box shows up as spread between the rounds of one arm.  Also timed, stand-alone over
`--kernel-reps` launches between two events: svit_im2col_patch_u8_aug_frames beside svit_im2col_patch_u8_aug, and the
pieces of the fp32 route (render, the permute copy of the clip into frames, svit_im2col_patch of the frames).
Prints one JSON line.  GPU box."""
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

ARMS = ("render_fp32", "u8")


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
    ap.add_argument("--kernels-only", action="store_true", help="launch only the stand-alone kernels")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames_u8.py measures on the GPU; none found")

    from svit_amd import config, losses, ops, optim
    from svit_amd.augment import AugClips, SpatialSampler
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.input import FramesView
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
    random.seed(cfg.RNG_SEED)
    np.random.seed(cfg.RNG_SEED)
    sp = SpatialSampler(S, scale=cfg.DATA.TRAIN_JITTER_SCALES_RELATIVE, aspect=cfg.DATA.TRAIN_JITTER_ASPECT_RELATIVE,
                        random_flip=cfg.DATA.RANDOM_FLIP, re_prob=0.0)
    records = [sp.draw(Hs, Ws, video=v) for v in range(B)]
    clips = AugClips(frames, S, records, mean=cfg.DATA.MEAN, std=cfg.DATA.STD)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    ms = {a: [] for a in ARMS}
    loss, graphed = {}, {}
    if not args.kernels_only:
        graphed = {"render_fp32": GraphedTrainStep(model, ce, [clips.render()], y, frames_pass=True),
                   "u8": GraphedTrainStep(model, ce, [clips], y, frames_pass="u8")}
        start = [(t, t.clone()) for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)]

    def timed(arm):
        """-> ms per step of `arm`: every leg starts from the same weights, optimizer state and batch"""
        step = graphed[arm]
        for t, saved in start:
            t.copy_(saved)
        opt.step_count = 0
        ys = step.static_labels
        static = step.static_inputs[0]          # u8: the frames and records already lie in the step's own buffers

        def one(it):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, it / 1000.0))
            out, _ = step([clips.render() if arm == "render_fp32" else static], ys)
            opt.step()
            return out

        for it in range(args.warmup):
            one(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.steps):
            out = one(args.warmup + it)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, float(out)

    for r in range(0 if args.kernels_only else args.rounds):
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

    view = FramesView(clips)
    clip32 = clips.render()
    frames32 = clip32.transpose(1, 2).flatten(0, 1).unsqueeze(2).contiguous()
    kernels = {
        "im2col_patch_u8_aug_frames": kernel_us(lambda: ops.im2col_patch_u8_aug_frames(view)),
        "im2col_patch_u8_aug": kernel_us(lambda: ops.im2col_patch_u8_aug(clips)),
        "u8_clips_render": kernel_us(lambda: ops.u8_clips_render(clips)),
        "fp32 clip -> frames permute copy": kernel_us(lambda: clip32.transpose(1, 2).flatten(0, 1).unsqueeze(2).contiguous()),
        "im2col_patch on the fp32 frames": kernel_us(lambda: ops.im2col_patch(frames32)),
    }
    same = torch.equal(ops.im2col_patch_u8_aug_frames(view)[0].view(torch.int16), ops.im2col_patch(frames32)[0].view(torch.int16))

    out = {"workload": "SViT %dx%d^2 bf16, %d clips from uint8 %dx%d sources, fwd + frames pass + CE + bwd + clip + AdamW, "
                       "hip-graph replay" % (T, S, B, Hs, Ws),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "ms_per_step": ms,
           "ms_per_step_best": {a: min(v) for a, v in ms.items() if v},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items() if v}, "loss": loss,
           "n_graphs": {a: graphed[a].n_graphs for a in graphed}, "kernel_us": kernels,
           "frames_operand_equals_fp32_route": bool(same), "records": [list(r) for r in records]}
    if ms["u8"] and ms["render_fp32"]:
        a, b = min(ms["render_fp32"]), min(ms["u8"])
        out["u8_vs_render_fp32"] = {"ms": round(b - a, 3), "pct": round((b / a - 1) * 100, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
