#!/usr/bin/env python3
"""Step time of an image rank on uint8 stills (augment.AugClips with T = 1; boxes and targets from augment.draw_still),
in ONE process on one GPU (bench.py itself measures the video rank's fp32 step and stays as it is):

    A  fp32    the image-rank step as it was: fp32 stills [B,3,1,S,S] (normalised, cropped and augmented on the host)
    B  u8      AugClips over uint8 stills with per-still extents: resized crop, flip, erasing in the im2col
    C  u8+ra   + the yaml's RandAugment tables (AUG.AA_TYPE / AUG.INTERPOLATION): the 2N chain kernels ahead of it

    python tools/bench_image_rank_u8.py --steps 30 --warmup 5 --rounds 2 [--out profiles/r14_image_rank_u8_step.txt]

The workload is the recipe's image rank: B = 63 stills, S = 224, the 16-frame model's T' = 1 path, HAOG box / contact
losses, forward + backward + clip + AdamW, hip-graph replay; the sources are 63 uint8 stills of 240 x 320.  One model and
one optimizer serve all arms; every arm owns a captured step whose inputs and targets live in the step's static buffers
(no copy inside the timed region, as in bench.py).  The u8 arms' records, tables and targets come from
`augment.draw_still` with the yaml's values; the fp32 arm is fed arm B's rendered stills and targets (the same step up
to the DropPath / dropout draws of each replay).  The arms are timed in turn, `--rounds` times over, so that drift of the box shows up as spread between
the rounds of one arm.  Also timed: the host's share (`draw_still` for the 63 stills, boxes included) and, stand-alone
between two events, the RandAugment chain and the im2col of each arm.  Prints one JSON line.  GPU box."""
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

ARMS = ("fp32", "u8", "u8+ra")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=63)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--source", default="240x320")
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_image_rank_u8.py measures on the GPU; none found")

    from svit_amd import config, losses, ops, optim, randaug
    from svit_amd.augment import AugClips, build_sampler, draw_still, pack_videos
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    cfg.merge_from_file(os.path.join(ROOT, "tests", "golden", "ssv2.yaml"))      # AUG.* and the relative jitter
    cfg.NUM_GPUS, cfg.DATA.NUM_FRAMES, cfg.DATA.TRAIN_CROP_SIZE = 1, args.frames, args.crop
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0)
    model.train()
    opt = optim.construct_optimizer(model, cfg)
    B, S = args.batch, args.crop
    Hs, Ws = (int(v) for v in args.source.split("x"))
    g = torch.Generator().manual_seed(cfg.RNG_SEED)
    stills = [torch.randint(0, 256, (1, Hs, Ws, 3), generator=g, dtype=torch.uint8) for _ in range(B)]
    frames, extents = pack_videos(stills, Hs=Hs, Ws=Ws)
    # four hand / object boxes per still: centres U[.25,.75], sizes U[.1,.4] of the still, ~10 % absent rows
    c = torch.rand(B, 1, 4, 2, generator=g) * 0.5 + 0.25
    wh = torch.rand(B, 1, 4, 2, generator=g) * 0.3 + 0.1
    boxes = (torch.cat((c - wh / 2, c + wh / 2), -1) * torch.tensor([Ws, Hs, Ws, Hs])).numpy().astype(np.float32)
    boxes[(torch.rand(B, 1, 4, generator=g) < 0.1).numpy()] = 0
    contact = torch.tensor([-1, 0, 3])[torch.randint(0, 3, (B, 2), generator=g)]
    mean, std = cfg.DATA.MEAN, cfg.DATA.STD

    def draw(with_ra):
        random.seed(cfg.RNG_SEED)
        np.random.seed(cfg.RNG_SEED)
        ra, sp = (randaug.build_randaug(cfg) if with_ra else None), build_sampler(cfg, "train")
        t0 = time.perf_counter()
        drawn = [draw_still(ra, sp, Hs, Ws, boxes[v], video=v) for v in range(B)]
        host_ms = (time.perf_counter() - t0) * 1e3
        meta = {"haog_bboxes": torch.stack([t for _, _, t in drawn]).to(dev), "contact_state": contact.to(dev)}
        return [o for o, _, _ in drawn], [r for _, r, _ in drawn], meta, host_ms

    _, rec_b, meta_b, host_b = draw(False)
    tab_c, rec_c, meta_c, host_c = draw(True)
    u8 = AugClips(frames.to(dev), S, rec_b, mean=mean, std=std, extents=extents)
    inputs = {"fp32": u8.render(), "u8": u8,
              "u8+ra": AugClips(frames.to(dev), S, rec_c, mean=mean, std=std, randaug=tab_c, extents=extents)}
    metas = {"fp32": meta_b, "u8": meta_b, "u8+ra": meta_c}
    haog = losses.VideoImageLoss(cfg, is_video_rank=False)

    def loss_fun(preds, extra, labels):
        return haog.total(haog(preds, extra, None, labels))

    ms = {a: [] for a in ARMS}
    loss = {}
    graphed = {arm: GraphedTrainStep(model, loss_fun, [inputs[arm]], metas[arm]) for arm in ARMS}
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
        kernels.setdefault("im2col (fp32)", []).append(kernel_us(lambda: ops.im2col_patch(inputs["fp32"])))
        for arm in ARMS[1:]:
            clips = inputs[arm]
            kernels.setdefault("chain (%s)" % arm, []).append(kernel_us(clips.run_randaug))
            kernels.setdefault("im2col (%s)" % arm, []).append(kernel_us(lambda: ops._im2col_u8(
                "svit_im2col_patch_u8_aug", clips.frames, clips.lut_f32, clips.records, S, (None,), extents=clips.extents)))

    base = min(ms["fp32"])
    out = {"workload": "SViT image rank, %d stills -> %d^2 bf16 (T' = 1 of the %d-frame model), uint8 sources %dx%d, "
                       "fwd+HAOG+bwd+clip+AdamW, hip-graph replay" % (B, S, args.frames, Hs, Ws),
           "aa_type": cfg.AUG.AA_TYPE, "interpolation": cfg.AUG.INTERPOLATION, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds, "ms_per_step": ms, "ms_per_step_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()}, "loss": loss,
           "n_graphs": {a: graphed[a].n_graphs for a in ARMS}, "kernel_us": kernels,
           "host_draw_ms_per_batch": {"u8": round(host_b, 3), "u8+ra": round(host_c, 3)},
           "input_bytes_per_step": {"fp32": inputs["fp32"].numel() * 4, "u8": frames.numel()},
           "ops_drawn": [[o.op for o in layers] for layers in tab_c],
           "vs_fp32": {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                       for a, v in ms.items() if a != "fp32"}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
