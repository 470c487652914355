#!/usr/bin/env python3
"""Cost of the attention statistics (SVIT.ATTN_MONITOR: svit_attn_stats, csrc/attnmon.hip) on the bench workload, in ONE
process on one GPU (bench.py itself measures the step without the key and stays as it is):

    python tools/bench_attnmon.py --steps 30 --warmup 5 --rounds 2

(i) the pair of launches alone over the operands of one saved forward of the bench step (16 sites, 65 (block, head)
pairs, 1 + 64 + 32 probe rows each per sample): `--reps` pairs captured back to back into one graph, HIP events around a
replay, so that the host side of a call is not in the figure -- once due, once not due (a step record whose step is no
multiple of `every`);
(ii) the whole captured step (B = 8 clips of 16x224^2, bf16, forward + CE + backward + guarded clip + AdamW,
GraphedTrainStep(optimizer=...)) without the key, with it at every = 1 and at every = 10: each arm its own model,
optimizer and capture, the same weights and batch.

The arms are timed in turn, `--rounds` times over: drift of the box shows as spread between the rounds of one arm.  Every
timed replay that was due must have left its row: the ring is checked.  Prints one JSON line.  GPU box."""
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
    ap.add_argument("--reps", type=int, default=20, help="pairs of launches per timing")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attnmon.py measures on the GPU; none found")

    import bench
    from svit_amd import attnmon, config, losses, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    every = {"adamw": None, "attn_monitor": 1, "attn_monitor_every_10": 10}
    rigs, w0, x, y = {}, None, None, None
    for arm in every:
        cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
        cfg.SVIT.GUARDED_STEP = True
        cfg.LOG_PERIOD = args.warmup + args.steps
        if every[arm]:
            cfg.SVIT.ATTN_MONITOR, cfg.SVIT.ATTN_MONITOR_EVERY = True, every[arm]
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
        mon = attnmon.build_attnmon(cfg, model, opt)
        assert (mon is not None) == bool(every[arm]) and model.engine.attn_monitor is mon
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
        if mon is not None:         # every due replay left its row, none with a bad row
            rows = mon.read()
            due = list(range(0, total, mon.every))
            assert rows["steps"].tolist() == due and rows["passes"].tolist() == due and rows["lost"] == 0, rows["steps"]
            assert int(rows["n_bad"].sum()) == 0 and float(rows["sum_dev"].max()) < 2.0 ** -8
        return ms, float(loss)

    step_ms, loss = {a: [] for a in rigs}, {}
    for _ in range(args.rounds):
        for arm in rigs:
            t, loss[arm] = timed(arm)
            step_ms[arm].append(round(t, 3))

    # ---- the pair of launches alone, over the operands of one saved forward of the step ----
    r = rigs["attn_monitor"]
    model, opt = r["model"], r["opt"]
    model.attach_attention_monitor(None)
    with torch.no_grad():
        _, st = model.engine.forward(x, save=True)
    torch.cuda.synchronize()
    assert int(opt.dev_rec.view(torch.int64)[0]) % 1000 != 0          # (the step record of the timed run: not due at 1000)
    pair_us = {}
    probes = {"due": attnmon.AttentionMonitor(model, 4, optimizer=opt, every=1),
              "not_due": attnmon.AttentionMonitor(model, 4, optimizer=opt, every=1000)}
    sites = probes["due"].sites_of(st)[0]
    macs = sum(s["B"] * s["heads"] * probes["due"].n_probe(s["Lq"], s["n_obj"]) * s["Nk"] * (96 + s["bias_cols"]) for s in sites)
    for name, mon in probes.items():
        mon.enqueue(st)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.reps):
                mon.enqueue(st)
        pair_us[name] = []
        for _ in range(args.rounds):
            before = mon.state.tolist()
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            after = mon.state.tolist()
            assert after[0] == before[0] + 2 * args.reps and after[1] == before[1] + (2 * args.reps if name == "due" else 0)
            pair_us[name].append(round(e0.elapsed_time(e1) / args.reps * 1e3, 2))
    rows = probes["due"].read()
    assert int(rows["n_bad"].sum()) == 0 and len(rows["passes"]) == 4
    base = min(step_ms["adamw"])
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+guarded clip+AdamW in one captured step"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "reps": args.reps,
           "sites": len(sites), "entries": probes["due"].ent_slots,
           "workgroups": sum(s["B"] * s["heads"] * 3 for s in sites), "gmacs": round(macs / 1e9, 3),
           "pair_alone_us": pair_us, "pair_alone_us_best": {k: min(v) for k, v in pair_us.items()},
           "pair_tmacs_per_s": round(macs / (min(pair_us["due"]) * 1e-6) / 1e12, 2),
           "entropy_norm_mean": float("%.4g" % rows["entropy_norm"][-1].mean()),
           "sum_dev_max": float("%.4g" % rows["sum_dev"][-1].max()),
           "step_ms": step_ms, "step_ms_best": {a: min(v) for a, v in step_ms.items()},
           "step_spread_ms": {a: round(max(v) - min(v), 3) for a, v in step_ms.items()}, "loss": loss,
           "vs_adamw": {a: {"ms": round(min(step_ms[a]) - base, 3), "pct": round((min(step_ms[a]) / base - 1) * 100, 2)}
                        for a in step_ms if a != "adamw"}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
