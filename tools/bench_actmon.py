#!/usr/bin/env python3
"""Cost of the forward statistics (SVIT.ACT_MONITOR: svit_act_stats, csrc/actmon.hip) on the bench workload, in ONE
process on one GPU (bench.py itself measures the step without the key and stays as it is):

    python tools/bench_actmon.py --steps 30 --warmup 5 --rounds 2

(i) the pair of launches alone over arrays of the bench step's sizes (49 sites: about 1.1 M LayerNorm rows and 1.0 M
log-sum-exps, 13 MB): `--reps` pairs captured back to back into one graph, HIP events around a replay, so that the host
side of a call is not in the figure (the same pairs issued from Python are timed beside it, for comparison);
(ii) the whole captured step (B = 8 clips of 16x224^2, bf16, forward + CE + backward + guarded clip + AdamW,
GraphedTrainStep(optimizer=...)) without the key and with it: each arm its own model, optimizer and capture, the same
weights and batch.

The arms are timed in turn, `--rounds` times over: drift of the box shows as spread between the rounds of one arm.  Every
timed replay must have left its row: the pass counter and the ring are checked.  Prints one JSON line.  GPU box."""
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
    ap.add_argument("--reps", type=int, default=50, help="pairs of launches per timing")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_actmon.py measures on the GPU; none found")

    import bench
    from svit_amd import actmon, config, losses, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    rigs, w0, x, y = {}, None, None, None
    for arm in ("adamw", "act_monitor"):
        cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
        cfg.SVIT.GUARDED_STEP = True
        cfg.LOG_PERIOD = args.warmup + args.steps
        if arm == "act_monitor":
            cfg.SVIT.ACT_MONITOR = True
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
        mon = actmon.build_actmon(cfg, model, opt)
        assert (mon is not None) == (arm == "act_monitor") and model.engine.act_monitor is mon
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
        if mon is not None:         # every replay left its row, none with a bad row
            rows = mon.read()
            assert rows["passes"].tolist() == list(range(total)) and rows["lost"] == 0, rows["passes"]
            assert rows["steps"].tolist() == list(range(total)) and int(rows["n_bad"].sum()) == 0
        return ms, float(loss)

    step_ms, loss = {a: [] for a in rigs}, {}
    for _ in range(args.rounds):
        for arm in rigs:
            t, loss[arm] = timed(arm)
            step_ms[arm].append(round(t, 3))

    # ---- the pair of launches alone, over arrays of the step's sizes ----
    r = rigs["act_monitor"]
    mon, plan = r["mon"], r["model"].plan
    T0 = args.frames // plan.patch_stride[0]
    H0 = args.crop // plan.patch_stride[1]
    geo = actmon.slot_geometry(plan, args.frames, T0, H0, H0)
    gen = torch.Generator(device=dev).manual_seed(1)

    def rows_of(i):
        heads, (t, h, w), n_obj = geo[i]
        return args.batch * (heads or 1) * (1 + t * h * w + n_obj)

    def mean(n):
        return torch.randn(n, device=dev, generator=gen) * 0.3

    def rstd(n):
        return torch.exp(torch.randn(n, device=dev, generator=gen) * 0.5)
    st = {"B": args.batch, "Tx": args.frames, "thw0": (T0, H0, H0), "blocks": []}
    for i in range(len(plan.blocks)):
        st["blocks"].append({"mean1": mean(rows_of(3 * i)), "rstd1": rstd(rows_of(3 * i)),
                             "lse2": mean(rows_of(3 * i + 1)) + 5.0,
                             "mean2": mean(rows_of(3 * i + 2)), "rstd2": rstd(rows_of(3 * i + 2))})
    st["mean"], st["rstd"] = mean(rows_of(len(geo) - 1)), rstd(rows_of(len(geo) - 1))
    sites = mon.sites_of(st)[0]
    ln_rows = sum(n for _, b, n in sites if b is not None)
    lse_rows = sum(n for _, b, n in sites if b is None)
    nbytes = 8 * ln_rows + 4 * lse_rows

    # `reps` pairs captured back to back into ONE graph and replayed: the host side of enqueue() (a 49-entry table built
    # in Python) is paid at capture, the events see the kernels' own time
    mon.enqueue(st)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(args.reps):
            mon.enqueue(st)

    def pair_alone():
        before = int(mon.state[0])
        graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        assert int(mon.state[0]) == before + 2 * args.reps
        return round(e0.elapsed_time(e1) / args.reps * 1e3, 2)

    def pair_eager():       # the same pairs issued from Python: the host's issue rate, for comparison only
        for _ in range(3):
            mon.enqueue(st)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            mon.enqueue(st)
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / args.reps * 1e3, 2)

    pair_us, eager_us = [], []
    for _ in range(args.rounds):
        pair_us.append(pair_alone())
        eager_us.append(pair_eager())
    want, mass = actmon.acts_host([(a.cpu().numpy(), None if b is None else b.cpu().numpy())
                                   for a, b in mon.sites_of(st)[2]])
    got = mon.read()
    err = abs(got["sum"].data[-1] - want["sum"])
    assert (err <= 2.0 ** -27 * mass).all() and (got["arg"].data[-1] == want["arg"]).all()
    base = min(step_ms["adamw"])
    out = {"workload": "SViT %dx%d^2 bf16, %d clips, fwd+CE+bwd+guarded clip+AdamW in one captured step"
                       % (args.frames, args.crop, args.batch),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "reps": args.reps,
           "sites": len(sites), "ln_rows": ln_rows, "lse_rows": lse_rows, "bytes": nbytes,
           "windows": sum((n + mon.window - 1) // mon.window for _, _, n in sites),
           "pair_alone_us": pair_us, "pair_alone_us_best": min(pair_us), "pair_issued_from_python_us": eager_us,
           "pair_gb_per_s": round(nbytes / (min(pair_us) * 1e-6) / 1e9, 1),
           "step_ms": step_ms, "step_ms_best": {a: min(v) for a, v in step_ms.items()},
           "step_spread_ms": {a: round(max(v) - min(v), 3) for a, v in step_ms.items()}, "loss": loss,
           "vs_adamw": {"ms": round(min(step_ms["act_monitor"]) - base, 3),
                        "pct": round((min(step_ms["act_monitor"]) / base - 1) * 100, 2)}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
