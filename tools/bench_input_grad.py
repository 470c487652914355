#!/usr/bin/env python3
"""Cost of the input gradient (svit_patch_embed_dgrad, csrc/dgrad.hip) on the bench workload, in ONE process on one GPU
(bench.py itself makes no request and stays as it is):

    python tools/bench_input_grad.py --steps 30 --warmup 5 --rounds 2

(i) the kernel alone on operands of the bench step's shape (B = 8 clips of 16x224^2: dtok bf16 [200704, 96], w16 bf16
[96, 448] -> f32 [8,3,16,224,224]): `--reps` launches captured back to back into one graph, HIP events around a replay,
so that the host side of a call is not in the figure;
(ii) the whole captured step (bf16, forward + CE + backward + guarded clip + AdamW, GraphedTrainStep(optimizer=...))
without and with `input_grad=True`: each arm its own model, optimizer and capture, the same weights and batch.

The arms are timed in turn, `--rounds` times over: drift of the box shows as spread between the rounds of one arm.  The
asking arm's `step.input_grad` must be finite and non-zero after the timed replays (the default weight-gradient mode meets
in fp32 atomics, so the two arms' losses agree only to rounding).  Prints one JSON line.  GPU box."""
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
    ap.add_argument("--reps", type=int, default=20, help="launches per timing of the kernel alone")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_input_grad.py measures on the GPU; none found")

    import bench
    from svit_amd import config, losses, ops, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    rigs, w0, x, y = {}, None, None, None
    for arm in ("plain", "input_grad"):
        cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
        cfg.SVIT.GUARDED_STEP = True
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
        step = GraphedTrainStep(model, ce, [x], y, optimizer=opt, warmup=2, input_grad=arm == "input_grad")
        torch.cuda.synchronize()
        state = [getattr(opt, k) for k in opt.STATE]
        rigs[arm] = dict(cfg=cfg, opt=opt, step=step, start=[(t, t.clone()) for t in [model.flat.data] + state])

    def timed(arm):
        r = rigs[arm]
        g, opt, cfg = r["step"], r["opt"], r["cfg"]
        for t, saved in r["start"]:
            t.copy_(saved)
        opt.step_count = 0
        opt.dev_rec.zero_()
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
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        assert opt.stats()["applied"] == args.warmup + args.steps
        if g.input_grad is not None:
            assert bool(torch.isfinite(g.input_grad).all()) and float(g.input_grad.abs().max()) > 0.0
            assert tuple(g.input_grad.shape) == (args.batch, 3, args.frames, args.crop, args.crop)
        return ms, float(loss)

    step_ms, loss = {a: [] for a in rigs}, {}
    for _ in range(args.rounds):
        for arm in rigs:
            t, loss[arm] = timed(arm)
            step_ms[arm].append(round(t, 3))

    # ---- the kernel alone ----
    B, T, S = args.batch, args.frames, args.crop
    To, Ho = (T - 1) // 2 + 1, (S - 1) // 4 + 1
    g = torch.Generator(device=dev).manual_seed(1)
    dtok = torch.randn((B * To * Ho * Ho, 96), device=dev, generator=g).to(torch.bfloat16)
    w16 = (0.1 * torch.randn((96, 448), device=dev, generator=g)).to(torch.bfloat16)
    out = torch.empty((B, 3, T, S, S), device=dev)
    ops.patch_embed_dgrad(dtok, w16, B, T, S, S, out=out)
    torch.cuda.synchronize()
    first = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.reps):
            ops.patch_embed_dgrad(dtok, w16, B, T, S, S, out=out)
    kernel_us = []
    for _ in range(args.rounds):
        graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        kernel_us.append(round(e0.elapsed_time(e1) / args.reps * 1e3, 2))
    assert torch.equal(out.view(torch.int32), first.view(torch.int32))      # every launch the same bits
    # products the formula sums: per axis the (output position, tap) pairs whose pixel lies inside the clip
    pairs = [sum(1 for o in range(n_o) for k in range(taps) if 0 <= stride * o - pad + k < n)
             for n, n_o, taps, stride, pad in ((T, To, 3, 2, 1), (S, Ho, 7, 4, 3), (S, Ho, 7, 4, 3))]
    macs = B * 3 * 96 * pairs[0] * pairs[1] * pairs[2]
    written = out.numel() * 4
    base = min(step_ms["plain"])
    best = min(kernel_us) * 1e-6
    res = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+guarded clip+AdamW in one captured step"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "reps": args.reps,
           "gmacs": round(macs / 1e9, 3), "mb_written": round(written / 1e6, 1),
           "kernel_alone_us": kernel_us, "kernel_alone_us_best": min(kernel_us),
           "kernel_tmacs_per_s": round(macs / best / 1e12, 2), "kernel_write_gb_per_s": round(written / best / 1e9, 1),
           "step_ms": step_ms, "step_ms_best": {a: min(v) for a, v in step_ms.items()},
           "step_spread_ms": {a: round(max(v) - min(v), 3) for a, v in step_ms.items()}, "loss": loss,
           "vs_plain": {"ms": round(min(step_ms["input_grad"]) - base, 3),
                        "pct": round((min(step_ms["input_grad"]) / base - 1) * 100, 2)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
