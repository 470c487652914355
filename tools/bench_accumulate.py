#!/usr/bin/env python3
"""Step time of k accumulated micro-steps (graph.AccumulatedTrainStep: k replays, ONE optimizer step) against the path a
one-GPU user had before -- k replays of GraphedTrainStep(optimizer=guarded), i.e. k optimizer steps -- on the bench
workload, in ONE process on one GPU (bench.py itself measures the single step and stays as it is):

    replays      k x GraphedTrainStep(optimizer=guarded): weight refresh, memset and guarded tail in every replay
    accumulated  AccumulatedTrainStep over one captured micro-step used k times: eager prologue (weight refresh, memset),
                 k replays without either, the eager guarded tail once with grad_scale = 1/k

    python tools/bench_accumulate.py --steps 20 --warmup 3 --rounds 2
    python tools/bench_accumulate.py --recipe            # + one W = 1, k = 8 step of the recipe's shapes

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward, hip-graph replay, k = 4 video
micro-steps per "step".  One model serves both arms; every leg starts from the same weights and optimizer state.  The
arms are timed in turn, `--rounds` times over: drift of the box shows as spread between the rounds of one arm.
`--recipe`: the yaml's eight ranks as virtual ranks of one GPU -- 7 x 9 clips with cross entropy and 63 stills with the
HAOG losses, two captures -- timed over `--recipe-steps` steps, with torch.cuda.max_memory_allocated.  Prints one JSON
line.  GPU box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

ARMS = ("replays", "accumulated")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--recipe", action="store_true")
    ap.add_argument("--recipe-steps", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_accumulate.py measures on the GPU; none found")

    import bench
    from svit_amd import config, losses, optim
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    cfg.SVIT.GUARDED_STEP = True
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0)
    model.train()
    guarded = optim.construct_optimizer(model, cfg)
    assert type(guarded) is optim.GuardedClipAdamW
    x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)
    k = args.k

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    whole = GraphedTrainStep(model, ce, [x], y, optimizer=guarded)
    micro = GraphedTrainStep(model, ce, [x], y, accumulate=True)
    acc = AccumulatedTrainStep(model, [micro] * k, guarded)
    start = [(t, t.clone()) for t in (model.flat.data, guarded.exp_avg, guarded.exp_avg_sq)]

    def reset():
        for t, saved in start:
            t.copy_(saved)
        guarded.step_count = 0

    def one(arm, it):
        optim.set_lr(guarded, optim.get_lr_at_epoch(cfg, it / 1000.0))
        if arm == "replays":
            xs, ys = whole.static_inputs, whole.static_labels
            for _ in range(k):
                loss, _ = whole(xs, ys)
            return loss
        return acc([(micro.static_inputs, micro.static_labels)] * k)[-1]

    def timed(arm):
        reset()
        (whole if arm == "replays" else micro).static_inputs[0].copy_(x)
        for it in range(args.warmup):
            one(arm, it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.steps):
            loss = one(arm, args.warmup + it)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, float(loss)

    ms = {a: [] for a in ARMS}
    loss = {}
    for _ in range(args.rounds):
        for arm in ARMS:
            t, loss[arm] = timed(arm)
            ms[arm].append(round(t, 3))
    stats = guarded.stats()
    best = {a: min(v) for a, v in ms.items()}
    out = {"workload": "SViT %dx%d^2 bf16, %d clips per micro-step, k = %d micro-steps per step, fwd+CE+bwd, hip-graph "
                       "replay, guarded clip+AdamW" % (args.frames, args.crop, args.batch, k),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "k": k,
           "ms_per_step": ms, "ms_per_step_best": best,
           "ms_per_micro_step_best": {a: round(v / k, 3) for a, v in best.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()},
           "accumulated_minus_replays": {"ms": round(best["accumulated"] - best["replays"], 3),
                                         "pct": round((best["accumulated"] / best["replays"] - 1) * 100, 2)},
           "optimizer_steps_per_step": {"replays": k, "accumulated": 1}, "loss": loss,
           "n_graphs": {"whole": whole.n_graphs, "micro": micro.n_graphs}, "parameters": model.flat.total,
           "applied_in_last_leg": stats["applied"],
           "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1024 ** 3, 2)}

    if args.recipe:
        del whole, micro, acc
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        from svit_amd.dp import virtual_roles
        rcfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=8)
        rcfg.IMAGE_TRAIN.GPU_IDS, rcfg.IMAGE_TRAIN.BATCH_SIZE, rcfg.TRAIN.BATCH_SIZE = [7], 63, 63
        roles = virtual_roles(rcfg, 1, 0)
        assert [r.batch_size for r in roles] == [9] * 7 + [63] and [r.is_image for r in roles] == [False] * 7 + [True]
        vloss = losses.VideoImageLoss(rcfg, is_video_rank=True)
        iloss = losses.VideoImageLoss(rcfg, is_video_rank=False)
        vx, vy = bench.synth_batch(rcfg, 9, dev, seed=1)
        ix, imeta = bench.synth_image_batch(rcfg, 63, dev, seed=2)
        video = GraphedTrainStep(model, lambda p, e, l: vloss.total(vloss(p, e, l, l)), [vx], vy, accumulate=True)
        image = GraphedTrainStep(model, lambda p, e, l: iloss.total(iloss(p, e, l, l)), [ix], imeta, accumulate=True)
        step = AccumulatedTrainStep(model, [video] * 7 + [image], guarded)
        batches = [(video.static_inputs, video.static_labels)] * 7 + [(image.static_inputs, image.static_labels)]
        reset()
        step(batches)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.recipe_steps):
            got = step(batches)
        torch.cuda.synchronize()
        out["recipe_w1_k8"] = {
            "shapes": "7 x 9 clips of %dx%d^2 (CE) + 63 stills of %d^2 (HAOG), two captures" % (args.frames, args.crop,
                                                                                                args.crop),
            "ms_per_step": round((time.perf_counter() - t0) / args.recipe_steps * 1e3, 2), "steps": args.recipe_steps,
            "losses": [round(float(l), 4) for l in got], "guarded": guarded.stats(),
            "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1024 ** 3, 2),
            "memory_reserved_gb": round(torch.cuda.memory_reserved(dev) / 1024 ** 3, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
