#!/usr/bin/env python3
"""Cost of per-range learning-rate scales (SOLVER.LAYER_DECAY / SVIT.LR_MULT) on the bench workload, in ONE process on
one GPU (bench.py itself measures the classic step without scales and stays as it is):

    python tools/bench_layer_decay.py --steps 30 --warmup 5 --rounds 2

(i) the guarded tail alone, from HIP events around back-to-back launches on the gradients of the last step:

    plain       svit_step_guard + svit_adamw_step_guarded
    seg2        the `_seg` pair over a two-entry table that covers the buffer
    lr_ones     svit_step_guard + svit_adamw_step_guarded_lr over the 38-range table, every scale 1.0
    lr_decay    the same launch with the scales of LAYER_DECAY = 0.75

(ii) the whole captured step (B = 8 clips of 16x224^2, bf16, forward + CE + backward + guarded clip + AdamW,
GraphedTrainStep(optimizer=GuardedClipAdamW)), without the keys and at LAYER_DECAY = 0.75: each arm its own model,
optimizer and capture, the same weights and batch.

The arms of each part are timed in turn, `--rounds` times over: drift of the box shows as spread between the rounds of
one arm.  Prints one JSON line.  GPU box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

DECAY = 0.75


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
        raise SystemExit("bench_layer_decay.py measures on the GPU; none found")

    import bench
    from svit_amd import config, losses, ops, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    rigs, w0, x, y = {}, None, None, None
    for arm in ("plain", "decay"):
        cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
        cfg.SVIT.GUARDED_STEP = True
        if arm == "decay":
            cfg.SOLVER.LAYER_DECAY = DECAY
        if x is None:
            x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)
        torch.manual_seed(cfg.RNG_SEED)
        model = build_model(cfg, gpu_id=0)
        model.train()
        if w0 is None:
            w0 = model.flat.data.clone()
        model.flat.data.copy_(w0)
        opt = optim.construct_optimizer(model, cfg)
        assert type(opt) is optim.GuardedClipAdamW and (opt.lr_segments is not None) == (arm == "decay")
        step = GraphedTrainStep(model, ce, [x], y, optimizer=opt, warmup=2)
        torch.cuda.synchronize()
        rigs[arm] = dict(cfg=cfg, model=model, opt=opt, step=step,
                         start=[(t, t.clone()) for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)])

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
        return (time.perf_counter() - t0) / args.steps * 1e3, float(loss)

    step_ms, loss = {a: [] for a in rigs}, {}
    for _ in range(args.rounds):
        for arm in rigs:
            t, loss[arm] = timed(arm)
            step_ms[arm].append(round(t, 3))

    # ---- the tail alone, on the decayed arm's buffers (gradients of its last replay) ----
    opt = rigs["decay"]["opt"]
    f = opt.flat
    whole = np.array([[0, f.n_decay], [f.n_decay, f.total]], dtype=np.int64)
    ones = np.ones(len(opt.lr_scales), dtype=np.float32)
    rec = (opt.host_rec, opt.dev_rec)
    b = (opt.betas[0], opt.betas[1], opt.eps)

    def guard():
        ops.step_guard(f.grad, *rec, opt.bias_table, opt._ws)

    def lr_tail(scales):
        guard()
        ops.adamw_step_guarded_lr(f.data, f.grad, opt.exp_avg, opt.exp_avg_sq, f.n_decay, opt.lr_segments, scales, *rec, *b)

    def seg2():
        ops.step_guard_seg(f.grad, whole, *rec, opt.bias_table, opt._ws)
        ops.adamw_step_guarded_seg(f.data, f.grad, opt.exp_avg, opt.exp_avg_sq, f.n_decay, whole, *rec, *b)

    def plain():
        guard()
        ops.adamw_step_guarded(f.data, f.grad, opt.exp_avg, opt.exp_avg_sq, f.n_decay, *rec, *b)

    tails = {"plain": plain, "seg2": seg2, "lr_ones": lambda: lr_tail(ones), "lr_decay": lambda: lr_tail(opt.lr_scales)}

    def tail_alone(enqueue):
        opt.upload()
        for _ in range(3):
            enqueue()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            enqueue()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.reps * 1e3, 2)

    tail_us = {k: [] for k in tails}
    for _ in range(args.rounds):
        for k, fn in tails.items():
            tail_us[k].append(tail_alone(fn))

    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+guarded clip+AdamW in one captured step"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "reps": args.reps,
           "layer_decay": DECAY, "ranges": int(len(opt.lr_segments)), "parameters": int(f.total),
           "tail_alone_us": tail_us, "tail_alone_us_best": {k: min(v) for k, v in tail_us.items()},
           "step_ms": step_ms, "step_ms_best": {a: min(v) for a, v in step_ms.items()},
           "step_spread_ms": {a: round(max(v) - min(v), 3) for a, v in step_ms.items()}, "loss": loss}
    base = min(step_ms["plain"])
    out["decay_vs_plain"] = {"ms": round(min(step_ms["decay"]) - base, 3),
                             "pct": round((min(step_ms["decay"]) / base - 1) * 100, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
