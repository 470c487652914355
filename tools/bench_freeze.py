#!/usr/bin/env python3
"""Step time and memory of the training step with frozen parameters on the bench workload, in ONE process on one GPU
(bench.py itself measures the all-trainable classic step and stays as it is):

    full        nothing frozen                                   -- the step every other arm is compared with
    cut3        SViT.freeze_below(4): stem and blocks 0-2 frozen (the cut above the big-M stages)
    cut14       SViT.freeze_below(15): stem and blocks 0-13 frozen (blocks 14, 15, the final norm and the head train)
    head        SViT.freeze_below(depth + 2): the head alone trains

    python tools/bench_freeze.py --steps 30 --warmup 5 --rounds 2

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward + clip + AdamW, as ONE captured step
with the guarded tail inside (GraphedTrainStep(optimizer=GuardedClipAdamW)).  Every arm has its own model, optimizer and
capture (the flags are read when those are built); all start from the same weights and see the same batch.  The arms are
timed in turn, `--rounds` times over: drift of the box shows as spread between the rounds of one arm.  Reported per arm:
ms per step (every round, best, spread), the peak of allocated memory while the arm was built and captured (above what
was allocated before: the activations its capture keeps), the trainable floats and the kernel-launch count of one body.
The tail alone, from HIP events around back-to-back launches on the gradients of the last step: the plain pair, the
`_seg` pair over a table that covers the whole buffer (the cost of the lookup itself) and the `_seg` pair over each
arm's segments.  Prints one JSON line.  GPU box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

ARMS = ("full", "cut3", "cut14", "head")


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
        raise SystemExit("bench_freeze.py measures on the GPU; none found")

    import bench
    from svit_amd import config, hip, losses, ops, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    cfg.SVIT.GUARDED_STEP = True
    x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    launches = [0]
    real_call = hip.call

    def counting(name, *a, **k):
        launches[0] += 1
        return real_call(name, *a, **k)

    rigs, w0 = {}, None
    for arm in arms:
        torch.manual_seed(cfg.RNG_SEED)
        model = build_model(cfg, gpu_id=0)
        model.train()
        depth = len(model.plan.blocks)
        if w0 is None:
            w0 = model.flat.data.clone()
        model.flat.data.copy_(w0)
        model.freeze_below({"full": 0, "cut3": 4, "cut14": 15, "head": depth + 2}[arm])
        opt = optim.construct_optimizer(model, cfg)
        assert type(opt) is optim.GuardedClipAdamW
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        hip.call, launches[0] = counting, 0
        try:
            step = GraphedTrainStep(model, ce, [x], y, optimizer=opt, warmup=2)
        finally:
            hip.call = real_call
        torch.cuda.synchronize()
        segs = opt.segments
        rigs[arm] = dict(model=model, opt=opt, step=step, cut=opt.cut,
                         peak_mb=round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1),
                         held_mb=round((torch.cuda.memory_allocated(dev) - base) / 2 ** 20, 1),
                         launches_per_body=launches[0] // 3,         # two warm-up bodies + the captured one
                         trainable=int(model.flat.total if segs is None else sum(b - a for a, b in segs)),
                         start=[(t, t.clone()) for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)])

    def timed(arm):
        r = rigs[arm]
        g, opt = r["step"], r["opt"]
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

    def tail_alone(opt, segs, reps=20):
        """ms of the guarded tail's launches alone, back to back, on the gradients the last replay left; segs: None =
        the plain pair, else the `_seg` pair over that table"""
        f = opt.flat

        def enqueue():
            if segs is None:
                ops.step_guard(f.grad, opt.host_rec, opt.dev_rec, opt.bias_table, opt._ws)
                ops.adamw_step_guarded(f.data, f.grad, opt.exp_avg, opt.exp_avg_sq, f.n_decay, opt.host_rec, opt.dev_rec,
                                       opt.betas[0], opt.betas[1], opt.eps)
            else:
                ops.step_guard_seg(f.grad, segs, opt.host_rec, opt.dev_rec, opt.bias_table, opt._ws)
                ops.adamw_step_guarded_seg(f.data, f.grad, opt.exp_avg, opt.exp_avg_sq, f.n_decay, segs, opt.host_rec,
                                           opt.dev_rec, opt.betas[0], opt.betas[1], opt.eps)
        opt.upload()
        for _ in range(3):
            enqueue()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            enqueue()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / reps, 4)

    ms = {a: [] for a in arms}
    loss = {}
    for _ in range(args.rounds):
        for arm in arms:
            t, loss[arm] = timed(arm)
            ms[arm].append(round(t, 3))
    tail = {}
    first = rigs[arms[0]]
    f = first["model"].flat
    whole = np.array([[0, f.n_decay], [f.n_decay, f.total]], dtype=np.int64)
    tail["plain_pair_whole_buffer"] = tail_alone(first["opt"], None)
    tail["seg_pair_whole_buffer"] = tail_alone(first["opt"], whole)
    for arm in arms:
        if rigs[arm]["opt"].segments is not None:
            tail["seg_pair_" + arm] = tail_alone(rigs[arm]["opt"], rigs[arm]["opt"].segments)
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+guarded clip+AdamW in one captured step"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "ms_per_step": ms,
           "ms_per_step_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()}, "loss": loss,
           "cut": {a: rigs[a]["cut"] for a in arms},
           "capture_peak_mb": {a: rigs[a]["peak_mb"] for a in arms},
           "capture_held_mb": {a: rigs[a]["held_mb"] for a in arms},
           "launches_per_body": {a: rigs[a]["launches_per_body"] for a in arms},
           "trainable_floats": {a: rigs[a]["trainable"] for a in arms}, "parameters": int(f.total),
           "tail_alone_ms": tail}
    if "full" in ms:
        base = min(ms["full"])
        out["vs_full"] = {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                          for a, v in ms.items() if a != "full"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
