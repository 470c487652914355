#!/usr/bin/env python3
"""Cost of the update monitor (SVIT.UPDATE_MONITOR: svit_update_snapshot + svit_update_stats, csrc/update.hip) on the bench
workload, in ONE process on one GPU (bench.py itself measures the step without the key and stays as it is):

    python tools/bench_updmon.py --steps 30 --warmup 5 --rounds 2

(i) the launches alone, from HIP events around back-to-back launches on the buffers of the last step:

    snapshot        svit_update_snapshot on a due step (p read, shadow written)          8 B per parameter
    stats           svit_update_stats' two launches on a due step (p, shadow, g, m, v)   20 B
    pair            both                                                                 28 B
    pair_not_due    both on a step that is not due: no workgroup loads anything
    tail            svit_step_guard + svit_adamw_step_guarded                            32 B
    tail_update     the same with the snapshot in front of the solver and the statistics behind it   60 B

(ii) the whole captured step (B = 8 clips of 16x224^2, bf16, forward + CE + backward + guarded clip + AdamW,
GraphedTrainStep(optimizer=...)) without the key, with a monitor that records every step and with one that records every
tenth: each arm its own model, optimizer and capture, the same weights and batch.

The arms of each part are timed in turn, `--rounds` times over: drift of the box shows as spread between the rounds of one
arm.  Every timed launch of a "due" arm must have been an APPLIED, due step (a launch that is not due returns before its
first load and would time nothing): the counters and the ring are checked.  Prints one JSON line.  GPU box."""
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
    ap.add_argument("--reps", type=int, default=20, help="launches per timing")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_updmon.py measures on the GPU; none found")

    import bench
    from svit_amd import config, losses, optim, updmon
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    rigs, w0, x, y = {}, None, None, None
    for arm, every in (("adamw", None), ("update_every_1", 1), ("update_every_10", 10)):
        cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
        cfg.SVIT.GUARDED_STEP = True
        cfg.LOG_PERIOD = 10
        if every is not None:
            cfg.SVIT.UPDATE_MONITOR = True
            cfg.SVIT.UPDATE_MONITOR_EVERY = every
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
        mon = updmon.build_update_monitor(cfg, opt)
        assert (mon is not None) == (every is not None) and opt.update_monitor is mon
        step = GraphedTrainStep(model, ce, [x], y, optimizer=opt, warmup=2)
        torch.cuda.synchronize()
        state = [getattr(opt, k) for k in opt.STATE]
        rigs[arm] = dict(cfg=cfg, model=model, opt=opt, mon=mon, step=step,
                         start=[(t, t.clone()) for t in [model.flat.data] + state])

    def timed(arm):
        r = rigs[arm]
        g, opt, cfg, mon = r["step"], r["opt"], r["cfg"], r["mon"]
        for t, saved in r["start"]:
            t.copy_(saved)
        opt.step_count = 0
        opt.dev_rec.zero_()
        if mon is not None:
            mon.reset()
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
        total = args.warmup + args.steps
        assert opt.stats()["applied"] == total
        if mon is not None:         # the newest due step is in the ring
            rows = mon.read()
            assert len(rows["steps"]) and int(rows["steps"][-1]) == (total - 1) // mon.every * mon.every, rows["steps"]
        return ms, float(loss)

    step_ms, loss = {a: [] for a in rigs}, {}
    for _ in range(args.rounds):
        for arm in rigs:
            t, loss[arm] = timed(arm)
            step_ms[arm].append(round(t, 3))

    # ---- the launches alone, over the every-step arm's model (buffers of its last replay) ----
    r = rigs["update_every_1"]
    opt, mon = r["opt"], r["mon"]

    def plain_tail():
        opt.update_monitor = None
        try:
            opt._solve()
        finally:
            opt.update_monitor = mon

    def alone(o, enqueue, steps_per_call):
        o.upload()
        before = o.stats()["applied"]
        for _ in range(3):
            enqueue()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            enqueue()
        e1.record()
        torch.cuda.synchronize()
        assert o.stats()["applied"] == before + (3 + args.reps) * steps_per_call, "a timed step was dropped"
        assert o.dev_rec[5].item() == 1, "the record says the last step was dropped"
        return round(e0.elapsed_time(e1) / args.reps * 1e3, 2)

    def pair(m):
        def both():
            m.snapshot()
            m.enqueue()
        return both

    arms = {"tail": (plain_tail, 1), "tail_update": (opt._solve, 1), "snapshot": (mon.snapshot, 0),
            "stats": (mon.enqueue, 0), "pair": (pair(mon), 0)}
    alone_us = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, (fn, n) in arms.items():
            alone_us[k].append(alone(opt, fn, n))
            if n == 0:              # the launches ran on a due step: the ring's newest row is the record's step
                s = opt.stats()
                assert int(mon._rows(-1)["head"]["step"][-1]) == s["applied"] + s["skipped"] - 1

    # the three launches on a step that is not due: all return before their first load (the every-tenth arm's monitor,
    # whose optimizer stands behind step warmup + steps - 1)
    r10 = rigs["update_every_10"]
    s10 = r10["opt"].stats()
    assert (s10["applied"] + s10["skipped"] - 1) % 10 != 0 and r10["opt"].dev_rec[5].item() == 1
    ring10, shadow10 = r10["mon"].ring.clone(), r10["mon"].shadow.clone()
    alone_us["pair_not_due"] = [alone(r10["opt"], pair(r10["mon"]), 0) for _ in range(args.rounds)]
    assert torch.equal(ring10, r10["mon"].ring), "a launch that was not due wrote the ring"
    assert torch.equal(shadow10.view(torch.int32), r10["mon"].shadow.view(torch.int32)), "... or the shadow"
    best = {k: min(v) for k, v in alone_us.items()}
    n = int(r["model"].flat.total)
    base = min(step_ms["adamw"])
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+guarded clip+AdamW in one captured step"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "reps": args.reps,
           "parameters": n, "tensors": len(mon.names), "alone_us": alone_us, "alone_us_best": best,
           "bytes": {"snapshot": 8 * n, "stats": 20 * n, "pair": 28 * n},
           "tb_per_s": {k: round(b * n / (best[k] * 1e-6) / 1e12, 2) for k, b in (("snapshot", 8), ("stats", 20), ("pair", 28))},
           "step_ms": step_ms, "step_ms_best": {a: min(v) for a, v in step_ms.items()},
           "step_spread_ms": {a: round(max(v) - min(v), 3) for a, v in step_ms.items()}, "loss": loss,
           "vs_adamw": {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                        for a, v in step_ms.items() if a != "adamw"}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
