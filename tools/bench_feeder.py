#!/usr/bin/env python3
"""What it costs to bring a batch from host memory to the captured step (svit_amd/feeder.py), in ONE process on one GPU
(bench.py itself measures the fp32-input step over static inputs and stays as it is):

    a  static   the captured step replayed over its static inputs: what every other tools/bench_*.py times
    e  unpack   (diagnostic) a plus one svit_feed_unpack launch per step from a slot already on the device: no upload
    b  direct   today's route, all on the main thread and stream: augment.pack_videos into a pinned buffer, upload,
                AugClips.copy_ into the static input (inside the step's call), replay
    c  feeder   feeder.ClipFeeder with its producer thread: put runs beside the loop; next(), replay, pump()
    d  inline   the feeder with put on the main thread: next(), replay, put(next batch), pump()

    python tools/bench_feeder.py --steps 30 --warmup 5 --rounds 2

The workload is bench.py's: B = 8 clips of 16x224^2, bf16, forward + CE + backward + clip + AdamW, hip-graph replay; the
sources are 8 uint8 videos of 240 x {320, 300, 284, 256} in a 16x240x320 buffer with the yaml's RandAugment tables.  A ring
of four pre-built host batches is cycled, so no decoding is timed.  The arms are timed in turn, `--rounds` times over, so
that drift of the box shows up as spread between the rounds of one arm.  For c and d the host time per step inside
`wait_ready` (the producer is behind), `next` (the upload is behind) and `put` is reported next to the step time.
Also measured: the host-to-device rate of a pinned copy of the padded batch; bytes per batch, tight against padded; the
host time of pack_tight against pack_videos (both into pinned memory); the unpack kernel against a torch device-to-device
copy_ of the padded buffer (the launch it replaces), `--kernel-reps` launches between two events, alternated.
Prints one JSON line.  GPU box."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

ARMS = ("static", "direct", "feeder", "inline", "unpack")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--crop", type=int, default=224)
    ap.add_argument("--source", default="240x320")
    ap.add_argument("--widths", default="320,300,284,256")
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--aa-type", default="rand-m7-n4-mstd0.5-inc1")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feeder.py measures on the GPU; none found")

    from svit_amd import config, feeder as fd, losses, ops, optim, randaug
    from svit_amd.augment import AugClips, SpatialSampler, pack_records, pack_videos
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.model import build_model
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = config.ssv2_cfg(num_frames=args.frames, crop=args.crop, num_gpus=1)
    torch.manual_seed(cfg.RNG_SEED)
    model = build_model(cfg, gpu_id=0)
    model.train()
    opt = optim.construct_optimizer(model, cfg)
    B, T, S = args.batch, args.frames, args.crop
    Hs, Ws = (int(v) for v in args.source.split("x"))
    widths = [int(w) for w in args.widths.split(",")]
    sizes = [(Hs, widths[v % len(widths)]) for v in range(B)]
    mean, std = cfg.DATA.MEAN, cfg.DATA.STD

    def host_batch(seed):
        """(videos, records, labels, RandAugment table): what a loader hands over after decoding.  Pixels and labels
        differ from batch to batch; the DRAWS are one seed's for every batch, so that every arm replays the same
        operations (an AFFINE layer costs fourteen times a point operation: other draws are other step times)"""
        g = torch.Generator().manual_seed(cfg.RNG_SEED + seed)
        videos = [torch.randint(0, 256, (T, h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]
        labels = torch.randint(0, cfg.MODEL.NUM_CLASSES, (B,), generator=g)
        random.seed(cfg.RNG_SEED)
        np.random.seed(cfg.RNG_SEED)
        ra = randaug.RandAugSampler(args.aa_type, "bicubic")
        sp = SpatialSampler(S, scale=cfg.DATA.TRAIN_JITTER_SCALES_RELATIVE, aspect=cfg.DATA.TRAIN_JITTER_ASPECT_RELATIVE,
                            random_flip=cfg.DATA.RANDOM_FLIP)
        table, records = [], []
        for v, (h, w) in enumerate(sizes):
            table.append(ra.draw(T, h, w, video=v))
            records.append(sp.draw(h, w, video=v))
        return videos, records, labels, table

    ring = [host_batch(k) for k in range(args.ring)]
    frames0, extents0 = pack_videos(ring[0][0], Hs=Hs, Ws=Ws)
    clips = AugClips(frames0.to(dev), S, ring[0][1], mean=mean, std=std, randaug=ring[0][3], extents=extents0)

    def ce(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    step = GraphedTrainStep(model, ce, [clips], ring[0][2].to(dev))
    target, static_labels = step.static_inputs[0], step.static_labels
    start = [(t, t.clone()) for t in (model.flat.data, opt.exp_avg, opt.exp_avg_sq)]
    # today's route: a staging AugClips on the device (its `raw` is the upload target) and one pinned padded buffer
    stage = clips.clone()
    pinned_ring = [(torch.empty(tuple(frames0.shape), dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(2)]
    pinned = pinned_ring[0][0]
    direct_tables = [(pack_records(r), torch.from_numpy(randaug.pack_table(t))) for _, r, _, t in ring]
    host = {"wait_ready": 0.0, "next": 0.0, "put": 0.0}
    # the feeders are built once, outside every timed leg (page-locking two slots takes longer than a step)
    ring_feeder = fd.ClipFeeder.for_step(step, depth=args.depth)
    resident_feeder = fd.ClipFeeder.for_step(step, depth=1)
    resident_feeder.put(*ring[0])
    resident_feeder.next()
    resident = resident_feeder._slots[0].args       # the launch arguments of a slot that stays on the device
    torch.cuda.synchronize()

    def clocked(name, fn, *a, **kw):
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        host[name] += time.perf_counter() - t0
        return out

    def run(arm, n, first):
        """n steps of `arm`, batch `first + i` of the ring at step i"""
        if arm == "static":
            for it in range(n):
                optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (first + it) / 1000.0))
                out, _ = step([target], static_labels)
                opt.step()
        elif arm == "direct":
            for it in range(n):
                videos, _, labels, _ = ring[(first + it) % len(ring)]
                rec, tab = direct_tables[(first + it) % len(ring)]
                buf, ev = pinned_ring[it % 2]           # (two pinned buffers: the upload of step n - 2 has read this one)
                ev.synchronize()
                _, ext = pack_videos(videos, Hs=Hs, Ws=Ws, out=buf)
                stage.raw.copy_(buf, non_blocking=True)
                ev.record()
                stage.extents.copy_(ext, non_blocking=True)
                stage.ra_table.copy_(tab, non_blocking=True)
                stage.records.copy_(rec, non_blocking=True)
                optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (first + it) / 1000.0))
                out, _ = step([stage], labels.to(dev, non_blocking=True))
                opt.step()
        elif arm == "feeder":
            f = ring_feeder
            producer = fd.Producer(f, (ring[(first + it) % len(ring)] for it in range(n)))
            producer.start()
            for it in range(n):
                clocked("wait_ready", producer.wait_ready)
                inputs, labels = clocked("next", f.next)
                optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (first + it) / 1000.0))
                out, _ = step(inputs, labels)
                opt.step()
                f.pump()
            producer.stop()
        elif arm == "unpack":
            for it in range(n):
                ops.feed_unpack(resident)
                optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (first + it) / 1000.0))
                out, _ = step([target], static_labels)
                opt.step()
        else:
            f = ring_feeder
            clocked("put", f.put, *ring[first % len(ring)])
            for it in range(n):
                inputs, labels = clocked("next", f.next)
                optim.set_lr(opt, optim.get_lr_at_epoch(cfg, (first + it) / 1000.0))
                out, _ = step(inputs, labels)
                opt.step()
                if it + 1 < n:
                    clocked("put", f.put, *ring[(first + it + 1) % len(ring)])
                f.pump()
        return out

    ms = {a: [] for a in ARMS}
    host_ms = {a: [] for a in ARMS}
    loss = {}

    def timed(arm):
        for t, saved in start:
            t.copy_(saved)
        opt.step_count = 0
        run(arm, args.warmup, 0)
        torch.cuda.synchronize()
        for k in host:
            host[k] = 0.0
        t0 = time.perf_counter()
        out = run(arm, args.steps, args.warmup)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps * 1e3
        return dt, float(out), {k: round(v / args.steps * 1e3, 3) for k, v in host.items() if v}

    for r in range(args.rounds):
        for arm in ARMS:
            t, loss[arm], h = timed(arm)
            ms[arm].append(round(t, 3))
            host_ms[arm].append(h)

    # ---- the parts, stand-alone --------------------------------------------------------------------------------------
    def events_ms(fn_, reps, stream=None):
        for _ in range(3):
            fn_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn_()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    padded_bytes = frames0.numel()
    dev_buf = torch.empty_like(target.raw)
    h2d = [round(padded_bytes / (events_ms(lambda: dev_buf.copy_(pinned, non_blocking=True), 10) * 1e-3) / 1e9, 2)
           for _ in range(args.rounds)]
    tight_slot = torch.empty(fd.tight_bytes(sizes, T), dtype=torch.uint8).pin_memory()
    tight_dev = torch.empty(tight_slot.numel(), dtype=torch.uint8, device=dev)
    h2d_tight_ms = [round(events_ms(lambda: tight_dev.copy_(tight_slot, non_blocking=True), 10), 3) for _ in range(args.rounds)]
    h2d_padded_ms = [round(events_ms(lambda: dev_buf.copy_(pinned, non_blocking=True), 10), 3) for _ in range(args.rounds)]

    def host_ms_of(fn_, reps=5):
        fn_()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn_()
        return round((time.perf_counter() - t0) / reps * 1e3, 3)

    pack = {"pack_tight": [], "pack_videos": []}
    for r in range(args.rounds):
        pack["pack_tight"].append(host_ms_of(lambda: fd.pack_tight(ring[1][0], out=tight_slot)))
        pack["pack_videos"].append(host_ms_of(lambda: pack_videos(ring[1][0], Hs=Hs, Ws=Ws, out=pinned)))

    _, offsets, extents = fd.pack_tight(ring[1][0], out=tight_slot)
    tight_dev.copy_(tight_slot)
    off_dev, ext_dev = torch.from_numpy(offsets).to(dev), torch.from_numpy(extents).to(dev)
    uargs = ops.feed_args(tight_dev, dev_buf, off_dev, ext_dev)
    src_pad = pack_videos(ring[1][0], Hs=Hs, Ws=Ws)[0].to(dev)
    kernels = {"svit_feed_unpack": [], "torch copy_ (padded, D2D)": []}
    for r in range(args.rounds):
        kernels["svit_feed_unpack"].append(round(events_ms(lambda: ops.feed_unpack(uargs), args.kernel_reps) * 1e3, 1))
        kernels["torch copy_ (padded, D2D)"].append(round(events_ms(lambda: dev_buf.copy_(src_pad), args.kernel_reps) * 1e3, 1))
    ops.feed_unpack(uargs)
    torch.cuda.synchronize()
    assert torch.equal(dev_buf, src_pad), "the unpacked buffer is not pack_videos'"

    ring_feeder.close()
    resident_feeder.close()
    base = min(ms["static"])
    out = {"workload": "SViT %dx%d^2 bf16, %d clips from uint8 videos of %s in a %dx%d buffer, fwd+CE+bwd+clip+AdamW, "
                       "hip-graph replay, ring of %d host batches" % (T, S, B, sorted(set(sizes)), Hs, Ws, len(ring)),
           "aa_type": args.aa_type, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "depth": args.depth,
           "ms_per_step": ms, "ms_per_step_best": {a: min(v) for a, v in ms.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in ms.items()},
           "clips_per_s_best": {a: round(B / min(v) * 1e3, 1) for a, v in ms.items()},
           "host_ms_per_step": host_ms, "loss": loss,
           "vs_static": {a: {"ms": round(min(v) - base, 3), "pct": round((min(v) / base - 1) * 100, 2)}
                         for a, v in ms.items() if a != "static"},
           "bytes_per_batch": {"tight": int(tight_slot.numel()), "padded": int(padded_bytes)},
           "h2d_GBps_pinned_padded": h2d, "h2d_ms": {"tight": h2d_tight_ms, "padded": h2d_padded_ms},
           "host_pack_ms": pack, "kernel_us": kernels}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
