#!/usr/bin/env python3
"""Step time of the guarded optimizer tail against the classic one on the bench workload, in ONE process on one GPU
(bench.py itself measures the classic step only and stays as it is):

    classic        GraphedTrainStep replay, then the eager FusedClipAdamW.step()          -- the step bench.py times
    guarded_eager  the same replay, then the eager GuardedClipAdamW.step()
    guarded_graph  GraphedTrainStep(optimizer=guarded): the tail inside the captured step
    guarded_skip   the same, every step poisoned (loss * NaN): the tail drops every step

    python tools/bench_guarded_step.py --steps 30 --warmup 5 --rounds 2

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward + clip + AdamW, hip-graph replay.  One
model serves all arms; the loss of every arm is CE times a one-element device tensor (1, or NaN in the skip arm), so all
arms replay the same launches up to the tail.  The arms are timed in turn, `--rounds` times over: drift of the box shows
as spread between the rounds of one arm, and the yardstick of every arm is `classic` of the same run.  Besides ms per
step the tool reports the tail alone, from HIP events: around the eager optimizer call of every timed step (eager arms),
and around back-to-back launches of the guarded tail on the gradients of the last step (`tail_alone_ms`: applied and
dropped; what the in-graph arms hold at their end).  Prints one JSON line.  GPU box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

ARMS = ("classic", "guarded_eager", "guarded_graph", "guarded_skip")


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
        raise SystemExit("bench_guarded_step.py measures on the GPU; none found")

    import bench
    from svit_amd import config, losses, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0)
    model.train()
    classic = optim.construct_optimizer(model, cfg)
    cfg.SVIT.GUARDED_STEP = True
    guarded = optim.construct_optimizer(model, cfg)
    assert type(classic) is optim.FusedClipAdamW and type(guarded) is optim.GuardedClipAdamW
    x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)
    poison = torch.ones(1, device=dev)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels) * poison

    plain = GraphedTrainStep(model, ce, [x], y)
    tail = GraphedTrainStep(model, ce, [x], y, optimizer=guarded)
    start = [(t, t.clone()) for t in (model.flat.data, classic.exp_avg, classic.exp_avg_sq, guarded.exp_avg,
                                      guarded.exp_avg_sq)]

    def timed(arm):
        """-> (ms per step, ms of the eager tail per step or None, loss): every leg starts from the same weights,
        optimizer state and batch"""
        g = plain if arm in ("classic", "guarded_eager") else tail
        opt = classic if arm == "classic" else guarded
        eager = arm in ("classic", "guarded_eager")
        for t, saved in start:
            t.copy_(saved)
        opt.step_count = 0
        poison.fill_(float("nan") if arm == "guarded_skip" else 1.0)
        xs, ys = g.static_inputs[0], g.static_labels
        xs.copy_(x)
        for it in range(args.warmup):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, it / 1000.0))
            g([xs], ys)
            if eager:
                opt.step()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.steps):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (args.warmup + it) / 1000.0))
            loss, _ = g([xs], ys)
            if eager:
                ev[it][0].record()
                opt.step()
                ev[it][1].record()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        tail_ms = sum(a.elapsed_time(b) for a, b in ev) / args.steps if eager else None
        return ms, tail_ms, float(loss)

    def tail_alone(poisoned, reps=20):
        """ms of the guarded tail's three launches alone, back to back on the gradients the last replay left"""
        for t, saved in start:
            t.copy_(saved)
        guarded.step_count = 0
        poison.fill_(float("nan") if poisoned else 1.0)
        plain(plain.static_inputs, plain.static_labels)
        guarded.upload()
        for _ in range(3):
            guarded.enqueue()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            guarded.enqueue()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    ms = {a: [] for a in arms}
    tails = {a: [] for a in arms}
    loss = {}
    for r in range(args.rounds):
        for arm in arms:
            t, tl, loss[arm] = timed(arm)
            ms[arm].append(round(t, 3))
            if tl is not None:
                tails[arm].append(round(tl, 3))
    alone = {"applied": round(tail_alone(False), 3), "dropped": round(tail_alone(True), 3)}
    stats = guarded.stats()
    n = model.flat.total
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+clip+AdamW, hip-graph replay"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "ms_per_step": ms,
           "ms_per_step_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()},
           "eager_tail_ms": {a: v for a, v in tails.items() if v}, "tail_alone_ms": alone, "loss": loss,
           "n_graphs": {"plain": plain.n_graphs, "tail": tail.n_graphs}, "parameters": n,
           # 28 B per parameter in the AdamW launch (p, m, v read + written, g read) + 4 B in the sum of squares
           "tail_bytes": {"applied": 32 * n, "dropped": 4 * n}, "guarded_stats_after_dropped_leg": stats}
    if "classic" in ms:
        base = min(ms["classic"])
        out["cost_vs_classic"] = {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                                  for a, v in ms.items() if a != "classic"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
