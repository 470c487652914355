#!/usr/bin/env python3
"""What the 3-crop test loop costs per batch when its input comes from HOST memory, in ONE process on one GPU
(tools/bench_eval.py draws its input from a tensor already in HBM; bench.py measures training and stays as it is):

    a  fp32     today's route with host batches: per video an fp32, host-normalised, host-rescaled [3,T,S,w] tensor in
                pinned memory, `.to(dev)` on the main stream, evaluate.spatial_crops, the eager model, TestMeter.update_stats
    b  eager    uint8 route, eager: augment.pack_videos into a pinned buffer, uploaded on the main stream into a staging
                AugClips (frames, records, extents), the eager model (ATen head), update_stats
    c  static   graph.GraphedEvalStep (fused head, the fold inside the graph) replayed over its static input: no upload
    d  feeder   c + feeder.ClipFeeder with its producer thread: wait_ready, next(), replay, pump()

    python tools/bench_eval_u8.py --steps 30 --warmup 5 --rounds 2

Workload: the ssv2 test setting, 4 videos per batch of 16 uint8 frames 240 x {320, 300, 284, 256}, three 224^2 views each
(12 clips), bf16 eval forward.  A ring of four pre-built host batches is cycled, so neither decoding nor the host rescale
of arm a is timed.  The arms are timed in turn, `--rounds` times over; every arm is reported against a of the same run.
Also: svit_head_eval against the ATen eval head (cat + SViTHead.forward) on the tokens of a 12-clip batch, `--kernel-reps`
launches between two events, alternated.  Prints one JSON line.  GPU box."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

ARMS = ("fp32", "eager", "static", "feeder")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--source", default="240x320")
    ap.add_argument("--widths", default="320,300,284,256")
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_u8.py measures on the GPU; none found")

    from svit_amd import config, evaluate, feeder as fd
    from svit_amd.augment import AugClips, build_sampler, pack_records, pack_videos
    from svit_amd.graph import GraphedEvalStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0).eval()
    V, T, S = args.videos, args.frames, args.crop
    crops, repeat = evaluate.unique_views(cfg)
    Hs, Ws = (int(v) for v in args.source.split("x"))
    widths = [int(w) for w in args.widths.split(",")]
    sizes = [(Hs, widths[v % len(widths)]) for v in range(V)]
    mean, std = cfg.DATA.MEAN, cfg.DATA.STD
    sampler = build_sampler(cfg, "test")
    n_videos = V * args.ring

    def host_batch(k):
        """what a loader hands over after decoding: uint8 videos + test-view records + label tree; and for arm a the
        same videos as the reference's loader ships them (normalised, short side rescaled to S, fp32, pinned)"""
        g = torch.Generator().manual_seed(cfg.RNG_SEED + k)
        videos = [torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]
        records, ids = evaluate.test_views(sampler, sizes, k * V, crops)
        labels = (ids // crops * 7) % cfg.MODEL.NUM_CLASSES          # (one label per video, as the meter asserts)
        fp32 = []
        for x, rec in zip(videos, records[::crops]):
            t = (x.float() / 255.0 - torch.tensor(mean)) / torch.tensor(std)
            t = torch.nn.functional.interpolate(t.permute(3, 0, 1, 2), size=(rec.out_h, rec.out_w), mode="bilinear",
                                                align_corners=False)
            fp32.append(t[None].contiguous().pin_memory())
        return videos, records, {"labels": labels, "clip_ids": ids}, fp32

    ring = [host_batch(k) for k in range(args.ring)]
    frames0, extents0 = pack_videos(ring[0][0], Hs=Hs, Ws=Ws)
    clips = AugClips(frames0.to(dev), S, ring[0][1], mean=mean, std=std, extents=extents0)
    tree0 = {k: v.to(dev) for k, v in ring[0][2].items()}
    meters = {a: evaluate.TestMeter(n_videos, crops, cfg.MODEL.NUM_CLASSES, args.steps) for a in ARMS}
    step = GraphedEvalStep(model, [clips], tree0, test_meter=meters["static"], repeat=repeat)
    fed = GraphedEvalStep(model, [clips], tree0, test_meter=meters["feeder"], repeat=repeat)
    target, static_labels = step.static_inputs[0], step.static_labels
    stage = clips.clone()
    pinned_ring = [(torch.empty(tuple(frames0.shape), dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(2)]
    tables = [pack_records(r) for _, r, _, _ in ring]
    ring_feeder = fd.ClipFeeder.for_step(fed, depth=args.depth)
    host = {"wait_ready": 0.0, "next": 0.0}
    torch.cuda.synchronize()

    def clocked(name, fn, *a, **kw):
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        host[name] += time.perf_counter() - t0
        return out

    @torch.no_grad()
    def run(arm, n, first):
        meter = meters[arm]
        if arm == "fp32":
            for it in range(n):
                _, _, tree, fp32 = ring[(first + it) % len(ring)]
                x = torch.cat([evaluate.spatial_crops(t.to(dev, non_blocking=True), S, crops) for t in fp32])
                probs, _ = model([x], {})
                meter.update_stats(probs, tree["labels"].to(dev, non_blocking=True),
                                   tree["clip_ids"].to(dev, non_blocking=True), repeat=repeat)
        elif arm == "eager":
            for it in range(n):
                videos, _, tree, _ = ring[(first + it) % len(ring)]
                buf, ev = pinned_ring[it % 2]           # (two pinned buffers: the upload of step n - 2 has read this one)
                ev.synchronize()
                _, ext = pack_videos(videos, Hs=Hs, Ws=Ws, out=buf)
                stage.frames.copy_(buf, non_blocking=True)
                ev.record()
                stage.extents.copy_(ext, non_blocking=True)
                stage.records.copy_(tables[(first + it) % len(ring)], non_blocking=True)
                probs, _ = model([stage], {})
                meter.update_stats(probs, tree["labels"].to(dev, non_blocking=True),
                                   tree["clip_ids"].to(dev, non_blocking=True), repeat=repeat)
        elif arm == "static":
            for it in range(n):
                probs, _ = step([target], static_labels)
        else:
            f = ring_feeder
            producer = fd.Producer(f, (ring[(first + it) % len(ring)][:3] for it in range(n)))
            producer.start()
            for it in range(n):
                clocked("wait_ready", producer.wait_ready)
                inputs, labels = clocked("next", f.next)
                probs, _ = fed(inputs, labels)
                f.pump()
            producer.stop()
        return probs

    ms = {a: [] for a in ARMS}
    host_ms = {a: [] for a in ARMS}

    def timed(arm):
        meters[arm].reset()
        step.refresh()
        run(arm, args.warmup, 0)
        torch.cuda.synchronize()
        for k in host:
            host[k] = 0.0
        t0 = time.perf_counter()
        run(arm, args.steps, args.warmup)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps * 1e3
        return dt, {k: round(v / args.steps * 1e3, 3) for k, v in host.items() if v}

    for r in range(args.rounds):
        for arm in ARMS:
            t, h = timed(arm)
            ms[arm].append(round(t, 3))
            host_ms[arm].append(h)

    # the routes agree: the ring once through a, b and d (c replays one static batch and is left out).  b and d differ by
    # the two heads' rounding only; a also by its host-side bilinear rescale (torch's taps, not the kernel's)
    for arm in ("fp32", "eager", "feeder"):
        meters[arm].reset()
        run(arm, len(ring), 0)
    torch.cuda.synchronize()
    agree = {"eager_vs_fp32_maxabs": float((meters["eager"].video_preds - meters["fp32"].video_preds).abs().max()),
             "feeder_vs_eager_maxabs": float((meters["feeder"].video_preds - meters["eager"].video_preds).abs().max()),
             "clips_folded_per_video": int(meters["feeder"].clip_count.min())}

    # ---- the head, stand-alone -----------------------------------------------------------------------------------------
    def events_us(fn_, reps):
        for _ in range(3):
            fn_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn_()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / reps * 1e3, 1)

    with torch.no_grad():
        tokens = model.engine.forward(target, None, save=False)[0]
    n_obj = T * model.O

    @torch.no_grad()
    def aten_head():
        return model.head(torch.cat((tokens[:, :1], tokens[:, -n_obj:]), dim=1), T=T)

    head_us = {"svit_head_eval": [], "ATen eval head (cat + SViTHead.forward)": []}
    for r in range(args.rounds):
        head_us["svit_head_eval"].append(events_us(lambda: model.head_eval(tokens, T), args.kernel_reps))
        head_us["ATen eval head (cat + SViTHead.forward)"].append(events_us(aten_head, args.kernel_reps))

    ring_feeder.close()
    base = min(ms["fp32"])
    out = {"workload": "SViT %dx%d^2 bf16 eval, %d videos per batch of %d uint8 frames %s, %d views each (%d clips), "
                       "ensemble fold x%d, ring of %d host batches" % (T, S, V, T, sorted(set(sizes)), crops, V * crops,
                                                                     repeat, len(ring)),
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "depth": args.depth,
           "ms_per_batch": ms, "ms_per_batch_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()},
           "videos_per_s_best": {a: round(V / min(v) * 1e3, 1) for a, v in ms.items()},
           "host_ms_per_batch": host_ms,
           "vs_fp32": {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                       for a, v in ms.items() if a != "fp32"},
           "bytes_per_batch": {"fp32 (host-rescaled videos)": int(sum(t.numel() * 4 for t in ring[0][3])),
                               "uint8 padded": int(frames0.numel()),
                               "uint8 tight": int(fd.tight_bytes(sizes, T))},
           "agreement": agree, "head_us": head_us, "head_tokens": list(tokens.shape)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
