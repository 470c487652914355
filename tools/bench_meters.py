#!/usr/bin/env python3
"""What logging the losses costs per step on the bench workload, in ONE process on one GPU (bench.py itself times the
step without any logging and stays as it is):

    step    GraphedTrainStep(optimizer=guarded) replay alone: nothing is read back
    item    the same replay, then `.item()` on every entry of the loss dict in every iteration -- what a caller has to do
            today for the reference's log lines (tools/train_net.py:153-167)
    meter   GraphedTrainStep(optimizer=guarded, meter=TrainMeter) at cfg.LOG_PERIOD = 10: one more launch inside the
            replay, one read per 10 iterations (meter.log_iter_stats in every iteration)

    python tools/bench_meters.py --steps 30 --warmup 5 --rounds 2

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward + clip + AdamW, hip-graph replay; the
loss function returns a three-entry dict in every arm.  One model serves all arms; the arms are timed in turn, `--rounds`
times over: drift of the box shows as spread between the rounds of one arm.  Prints one JSON line.  GPU box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

ARMS = ("step", "item", "meter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--period", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meters.py measures on the GPU; none found")

    import bench
    from svit_amd import config, losses, meters, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    cfg.LOG_PERIOD = args.period
    cfg.SVIT.GUARDED_STEP = True
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0)
    model.train()
    opt = optim.construct_optimizer(model, cfg)
    x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)
    half = torch.tensor(0.5, device=dev)

    def loss_fun(preds, extra, labels):
        ce = losses.cross_entropy(preds, labels)
        return {"loss_ce": ce, "half": ce * half, "loss": ce}

    meter = meters.TrainMeter(args.warmup + args.steps, cfg)
    plain = GraphedTrainStep(model, loss_fun, [x], y, optimizer=opt)
    metered = GraphedTrainStep(model, loss_fun, [x], y, optimizer=opt, meter=meter)
    start = [(t, t.clone()) for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)]

    def timed(arm):
        """-> (ms per step, last loss): every leg starts from the same weights, optimizer state and batch"""
        g = metered if arm == "meter" else plain
        for t, saved in start:
            t.copy_(saved)
        opt.step_count = 0
        meter.reset()
        xs, ys = g.static_inputs[0], g.static_labels
        xs.copy_(x)
        last = None

        def one(it):
            nonlocal last
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, it / 1000.0))
            g([xs], ys)
            if arm == "item":
                last = {k: v.item() for k, v in g.loss_dict.items()}
            elif arm == "meter":
                last = meter.log_iter_stats(0, it) or last
        for it in range(args.warmup):
            one(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.warmup, args.warmup + args.steps):
            one(it)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        return ms, (float(g.loss) if last is None else last["loss"])

    ms = {a: [] for a in ARMS}
    loss = {}
    for r in range(args.rounds):
        for arm in ARMS:
            t, loss[arm] = timed(arm)
            ms[arm].append(round(t, 3))
    base = min(ms["step"])
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+clip+AdamW in one hip-graph replay, 3-entry loss dict"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "log_period": args.period,
           "ms_per_step": ms, "ms_per_step_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()},
           "cost_vs_step": {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                            for a, v in ms.items() if a != "step"},
           "loss": loss, "n_graphs": {"step": plain.n_graphs, "meter": metered.n_graphs}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
