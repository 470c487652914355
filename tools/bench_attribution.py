#!/usr/bin/env python3
"""Cost of one attribution pass (svit_amd/attribution.py) on the bench workload, in ONE process on one GPU (bench.py
itself makes no request and stays as it is):

    python tools/bench_attribution.py --passes 16 --warmup 1 --rounds 2

Arms, per SmoothGrad pass at B = 8, 16x224^2, one model and one batch for all of them:
(a) the route without the input-gradient-only pass: the replay of GraphedTrainStep(input_grad=True) -- a full training
    backward with its gradient memset and weight refresh -- plus torch ops for the perturbation (randn, mul, add into
    the static clip) and the accumulation (add_ with alpha);
(b) `Attribution.smoothgrad`: 32 bytes uploaded, svit_attr_perturb, the replay of GraphedTrainStep(input_grad="only"),
    svit_attr_accumulate;
(c) the two kernels alone: `--reps` pairs captured back to back into one graph, HIP events around a replay.
The bare replays of the two captures (no perturbation, no accumulation) are timed as well.  The arms are timed in
turn, `--rounds` times over: drift of the box shows as spread between the rounds of one arm.  Prints one JSON line.
GPU box."""
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
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls of each arm before its timed one")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20, help="kernel pairs per timing of the kernels alone")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attribution.py measures on the GPU; none found")

    import bench
    from svit_amd import config, ops
    from svit_amd.attribution import Attribution, pack_record
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    x, y = bench.synth_batch(cfg, args.batch, dev, seed=cfg.RNG_SEED)
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0)
    model.train()
    n = args.passes
    sigma = 0.15 * (x.flatten(1).amax(dim=1) - x.flatten(1).amin(dim=1))

    def scalar(preds, extra, labels):
        return preds.gather(1, labels[:, None]).sum()

    full = GraphedTrainStep(model, scalar, [x], y, warmup=2, input_grad=True)
    attr = Attribution(model, x, target=y)
    acc = torch.empty_like(x)
    noise = torch.empty_like(x)

    def arm_a():
        xs = full.static_inputs[0]
        for k in range(n):
            noise.normal_()
            torch.addcmul(x, noise, sigma.view(-1, 1, 1, 1, 1), out=xs)
            full([xs], full.static_labels)
            if k == 0:
                torch.mul(full.input_grad, 1.0 / n, out=acc)
            else:
                acc.add_(full.input_grad, alpha=1.0 / n)

    def arm_b():
        attr.smoothgrad(n=n, sigma=sigma)

    def bare(step):
        def run():
            for _ in range(n):
                step([step.static_inputs[0]], step.static_labels)
        return run

    arms = {"a_full_step_torch_ops": arm_a, "b_attribution_smoothgrad": arm_b,
            "replay_input_grad_true": bare(full), "replay_input_grad_only": bare(attr.step)}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    per_pass = {a: [] for a in arms}
    for _ in range(args.rounds):
        for a, fn in arms.items():
            per_pass[a].append(round(timed(fn), 3))
    assert bool(torch.isfinite(attr.acc).all()) and float(attr.acc.abs().max()) > 0.0
    assert bool(torch.isfinite(acc).all()) and float(acc.abs().max()) > 0.0

    # ---- the two kernels alone ----
    rec = torch.frombuffer(bytearray(pack_record(1.0, 1.0 / n, 7, 1, False)), dtype=torch.int32).to(dev)
    out, g = torch.empty_like(x), torch.randn_like(x)
    graphs = {}
    for name, fn in (("perturb", lambda: ops.attr_perturb(x, rec, sigma=sigma, out=out)),
                     ("perturb_no_noise", lambda: ops.attr_perturb(x, rec, base=g, out=out)),
                     ("accumulate", lambda: ops.attr_accumulate(g, acc, rec))):
        fn()
        torch.cuda.synchronize()
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(args.reps):
                fn()
    kernel_us = {k: [] for k in graphs}
    for _ in range(args.rounds):
        for name, graph in graphs.items():
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            kernel_us[name].append(round(e0.elapsed_time(e1) / args.reps * 1e3, 2))
    mb = x.numel() * 4 / 1e6
    best = {a: min(v) for a, v in per_pass.items()}
    res = {"workload": "SViT %dx%d^2 bf16, %d clips, one SmoothGrad pass of %d" % (args.frames, args.crop, args.batch, n),
           "passes": n, "warmup": args.warmup, "rounds": args.rounds, "reps": args.reps, "clip_mb": round(mb, 1),
           "ms_per_pass": per_pass, "ms_per_pass_best": best,
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in per_pass.items()},
           "b_vs_a": {"ms": round(best["b_attribution_smoothgrad"] - best["a_full_step_torch_ops"], 3),
                      "pct": round((best["b_attribution_smoothgrad"] / best["a_full_step_torch_ops"] - 1) * 100, 2)},
           "only_vs_true_replay_ms": round(best["replay_input_grad_only"] - best["replay_input_grad_true"], 3),
           "kernels_alone_us": kernel_us, "kernels_alone_us_best": {k: min(v) for k, v in kernel_us.items()},
           "kernels_gb_per_s": {"perturb": round(2 * mb / min(kernel_us["perturb"]) * 1e3, 1),
                                "perturb_no_noise": round(3 * mb / min(kernel_us["perturb_no_noise"]) * 1e3, 1),
                                "accumulate": round(3 * mb / min(kernel_us["accumulate"]) * 1e3, 1)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
