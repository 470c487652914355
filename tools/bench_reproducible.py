#!/usr/bin/env python3
"""Step time of the three weight-gradient modes on the bench workload, in ONE process on one GPU (bench.py itself
measures the default mode only and stays as it is):

    default        row splits meet in fp32 atomics                         (Engine defaults)
    reproducible   row splits flush into slabs, summed in split order      (engine.reproducible = True)
    deterministic  no row split at all                                     (engine.deterministic = True)

    python tools/bench_reproducible.py --steps 30 --warmup 5 --rounds 2
    python tools/bench_reproducible.py --arms reproducible --rounds 1 --steps 5 --no-trace      # under a profiler

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward + clip + AdamW, hip-graph replay.
One model and one optimizer serve all arms; every arm owns a captured step (the mode is fixed at capture).  The arms
are timed in turn, `--rounds` times over, so that drift of the box shows up as spread between the rounds of one arm.
Per arm it also reports the HIP-event time of the weight-gradient GEMM calls of one eager step (for `reproducible` that
includes the reduce launches: one event pair brackets both launches of a call), the number of those calls and the
slab workspace.  Prints one JSON line.  GPU box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

ARMS = ("default", "reproducible", "deterministic")
TN_CALLS = ("svit_gemm_tn", "svit_gemm_tn_grouped", "svit_gemm_tn_grouped_ex", "svit_gemm_tn_grouped_slab")


def set_arm(eng, arm):
    eng.reproducible = arm == "reproducible"
    eng.deterministic = arm == "deterministic"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--no-trace", action="store_true", help="skip the event-timed eager step of every arm")
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]
    if any(a not in ARMS for a in arms):
        raise SystemExit("--arms: any of %s" % ", ".join(ARMS))

    import bench
    from svit_amd import config, hip, losses, ops, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0)
    model.train()
    opt = optim.construct_optimizer(model, cfg)
    x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)
    eng = model.engine

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    graphed = {}
    for arm in arms:
        set_arm(eng, arm)
        graphed[arm] = GraphedTrainStep(model, ce, [x], y)
    start = [(t, t.clone()) for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)]

    def timed(arm, it0):
        """-> ms per step of `arm`: every leg starts from the same weights and optimizer state"""
        g = graphed[arm]
        for t, saved in start:
            t.copy_(saved)
        opt.step_count = 0
        xs, ys = g.static_inputs[0], g.static_labels
        for it in range(args.warmup):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (it0 + it) / 1000.0))
            g([xs], ys)
            opt.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in range(args.steps):
            optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (it0 + args.warmup + it) / 1000.0))
            loss, _ = g([xs], ys)
            opt.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, float(loss)

    ms = {a: [] for a in arms}
    loss = {}
    for r in range(args.rounds):
        for arm in arms:
            t, loss[arm] = timed(arm, 0)
            ms[arm].append(round(t, 3))
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+clip+AdamW, hip-graph replay"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "ms_per_step": ms,
           "ms_per_step_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()}, "loss": loss}
    if "default" in ms:
        base = min(ms["default"])
        out["overhead_vs_default"] = {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                                      for a, v in ms.items() if a != "default"}
    if not args.no_trace:
        tn = {}
        for arm in arms:
            set_arm(eng, arm)
            for traced in (False, True):        # (one untraced eager step first: lazy state of the eager path)
                if traced:
                    hip.start_trace()
                model.flat.grad.zero_()
                logits, extra = model([x], {})
                ce(logits, extra, y).backward()
                torch.cuda.synchronize()
            trace = hip.stop_trace()
            calls = [(n, e0.elapsed_time(e1)) for n, e0, e1, _ in trace if n in TN_CALLS]
            tn[arm] = {"ms": round(sum(t for _, t in calls), 3), "calls": len(calls),
                       "by_entry_point": {n: sum(1 for m, _ in calls if m == n) for n in sorted({m for m, _ in calls})}}
        out["tn_eager_step"] = tn
        if "reproducible" in tn and "default" in tn:
            # every slab call of this step holds <= SVIT_TN_GROUP_MAX problems: one GEMM launch + one reduce launch
            out["added_dispatches"] = tn["reproducible"]["calls"]
    set_arm(eng, "default")
    out["slab_workspace_mb"] = {tag: round(b.numel() * 4 / 1e6, 2) for (_, tag), b in ops._tn_slab_ws.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
