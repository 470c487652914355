"""The batch feeder on the device: svit_feed_unpack (csrc/feed.hip) against `feeder.unpack_host`, and feeder.ClipFeeder
against the direct route (`pack_videos` + `AugClips` + copy into the captured step), bit for bit.

Kernel shapes: tests/feeder_cases.py -- row pitches of 9, 15, 21, 48 and 72 bytes, so one 16-byte chunk of the destination
spans three rows, two rows, a row and its padding, a third of a row, and rows astride; videos with 33- and 57-byte rows;
every output buffer between 64-byte canaries.  Steps: the tiny configuration (4 frames, S = 64, drop rates 0,
`engine.reproducible`) over a 20 x 24 buffer, so equal operands give equal bits."""
import random
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import feeder_cases as FC
from tests import smoke_impl as SM
from tests.test_augment_gpu import R
from tests.test_ragged_gpu import tight_videos

CANARY = 64
HS, WS, S = 20, 24, 64
AA, INTERP = "rand-m7-n4-mstd0.5-inc1", "random"


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import ops
    return ops


@pytest.fixture(scope="module")
def F(ops):
    from svit_amd import feeder
    return feeder


def guarded(nbytes, poison=0xEE):
    """`nbytes` device bytes between two 64-byte canaries -> (uint8 tensor, check())"""
    raw = torch.full((nbytes + 2 * CANARY,), 0x5C, dtype=torch.uint8, device="cuda")
    t = raw[CANARY:CANARY + nbytes]
    t.fill_(poison)

    def check():
        assert bool((raw[:CANARY] == 0x5C).all()) and bool((raw[CANARY + nbytes:] == 0x5C).all()), "canary overwritten"
    return t, check


def device_unpack(ops, slot, offsets, extents, V, T, Hs, Ws, fill=0, swap_rb=False, segments=(), sentinel=0x33):
    """one launch on a NumPy slot -> (frames as NumPy, [segment targets as NumPy]).  The slot is the head of a larger
    allocation whose tail holds `sentinel`; frames and every segment target lie between canaries.
    segments: [(src_off, bytes)]"""
    n = slot.size
    big = torch.full((n + 4096,), sentinel, dtype=torch.uint8, device="cuda")
    big[:n] = torch.from_numpy(np.ascontiguousarray(slot)).cuda()
    frames, check = guarded(V * T * Hs * Ws * 3)
    checks, targets, segs = [check], [], []
    for src_off, nbytes in segments:
        t, c = guarded(max(nbytes, 4))
        checks.append(c)
        targets.append((t, nbytes))
        segs.append((src_off, t, nbytes))
    off = None if offsets is None else torch.tensor([int(o) for o in offsets], dtype=torch.int64, device="cuda")
    ext = None if extents is None else torch.tensor([[int(h), int(w)] for h, w in extents], dtype=torch.int32, device="cuda")
    args = ops.feed_args(big, frames.view(V, T, Hs, Ws, 3), off, ext, fill, swap_rb, segs, slot_bytes=n)
    ops.feed_unpack(args)
    torch.cuda.synchronize()
    for c in checks:
        c()
    outs = []
    for t, nbytes in targets:
        assert bool((t[nbytes:] == 0xEE).all()), "a segment wrote past its length"
        outs.append(t[:nbytes].cpu().numpy())
    return frames.view(V, T, Hs, Ws, 3).cpu().numpy(), outs


# ------------------------------------------------------------------------------------ 1. the kernel against unpack_host ----
@pytest.mark.parametrize("case", FC.shape_cases(), ids=lambda c: "%dx%d_T%d_%s" % (c[0], c[1], c[2], "_".join("%dx%d" % s for s in c[3])))
def test_kernel_is_unpack_host(ops, F, case):
    Hs, Ws, T, sizes = case
    vids = FC.random_videos(sizes, T, seed=Hs * 100 + Ws + T)
    slot, offsets, extents = F.pack_tight(vids, out=np.random.default_rng(1).integers(0, 256, 1 << 16, dtype=np.uint8))
    for fill in (0, 255):
        for swap_rb in (False, True):
            want = F.unpack_host(slot, offsets, extents, T, Hs, Ws, fill=fill, swap_rb=swap_rb)
            got, _ = device_unpack(ops, slot, offsets, extents, 4, T, Hs, Ws, fill, swap_rb)
            assert int((got != want).sum()) == 0, (case, fill, swap_rb, int((got != want).sum()))
    # null tables: every video fills the buffer at v*T*Hs*Ws*3
    full = np.random.default_rng(2).integers(0, 256, (4 * T * Hs * Ws * 3 + 15) // 16 * 16, dtype=np.uint8)
    want = F.unpack_host(full, None, None, T, Hs, Ws, fill=7, swap_rb=True, V=4)
    assert np.array_equal(want[..., ::-1].reshape(-1), full[:want.size])
    got, _ = device_unpack(ops, full, None, None, 4, T, Hs, Ws, 7, True)
    assert int((got != want).sum()) == 0


def test_buffer_past_4_gib_is_addressed_in_int64(ops):
    """three videos of a 1 x 26000 x 27500 buffer: 2.145 GB each, just under the 2^31 rule, 6.4 GB in all -- chunk
    addresses pass 2^32 and the kernel takes its 64-bit division.  Every video is a 3 x 3 corner at an odd offset, the
    rest is fill; compared on the device (a host yardstick of 6.4 GB would take minutes)."""
    V, T, Hs, Ws = 3, 1, 26000, 27500
    assert T * Hs * Ws * 3 < 2 ** 31 and V * T * Hs * Ws * 3 > 2 ** 32
    slot = (np.arange(128) + 100).astype(np.uint8)                           # (no byte equals the fill)
    offsets, extents = [0, 33, 67], [(3, 3)] * V
    frames, check = guarded(V * T * Hs * Ws * 3)
    dev_slot = torch.from_numpy(slot).cuda()
    off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    ext = torch.tensor(extents, dtype=torch.int32, device="cuda")
    buf = frames.view(V, T, Hs, Ws, 3)
    ops.feed_unpack(ops.feed_args(dev_slot, buf, off, ext, fill=7))
    torch.cuda.synchronize()
    check()
    for v in range(V):
        assert np.array_equal(buf[v, 0, :3, :3].cpu().numpy().reshape(-1), slot[offsets[v]:offsets[v] + 27]), v
        assert int((buf[v] != 7).sum()) == 27, v
    del buf, frames
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------ 2. wild tables ----
@pytest.mark.parametrize("swap_rb", [False, True])
def test_wild_tables_never_read_outside_the_slot(ops, F, swap_rb):
    Hs, Ws, T = 12, 16, 2
    sizes = [(12, 16), (3, 3), (12, 11), (11, 16)]
    slot, offsets, extents = F.pack_tight(FC.random_videos(sizes, T, seed=5))
    absent = 0
    for offs, exts in FC.wild_tables(slot.size, T, Hs, Ws, offsets, extents):
        want = F.unpack_host(slot, offs, exts, T, Hs, Ws, fill=77, swap_rb=swap_rb)
        a, _ = device_unpack(ops, slot, offs, exts, 4, T, Hs, Ws, 77, swap_rb, sentinel=0x00)
        b, _ = device_unpack(ops, slot, offs, exts, 4, T, Hs, Ws, 77, swap_rb, sentinel=0xFF)
        assert np.array_equal(a, b), (offs, exts)              # nothing behind slot_bytes reaches the result
        assert int((a != want).sum()) == 0, (offs, exts, int((a != want).sum()))
        absent += sum(bool((a[v] == 77).all()) for v in range(4))
    assert absent >= 16


# --------------------------------------------------------------------------------------------------------- 3. segments ----
def test_segments_copy_exact_byte_counts(ops, F):
    rng = np.random.default_rng(3)
    slot = rng.integers(0, 256, 16 * 300, dtype=np.uint8)
    vids = FC.random_videos([(3, 3)], 1, seed=1)
    slot[:27] = vids[0].reshape(-1)
    for segments in ([(64, 0)], [(48, 1)], [(4784, 4)], [(4736, 64)], [(1024, 1027)],
                     [(32, 0), (48, 1), (64, 4), (128, 64), (192, 1027), (1232, 3), (1248, 1027), (4736, 64)]):
        got, outs = device_unpack(ops, slot, [0], [(3, 3)], 1, 1, 5, 7, 9, False, segments)
        assert np.array_equal(got, F.unpack_host(slot, [0], [(3, 3)], 1, 5, 7, fill=9))
        for (src_off, nbytes), out in zip(segments, outs):
            assert np.array_equal(out, slot[src_off:src_off + nbytes]), (src_off, nbytes)
    with pytest.raises(Exception, match="bad argument"):
        device_unpack(ops, slot, [0], [(3, 3)], 1, 1, 5, 7, 0, False, [(4784, 17)])       # one byte past the slot


# ----------------------------------------------------------------------------------------- 4. feeder == direct route ----
def video_batch(sizes, seed):
    """host videos of `sizes` + RandAugment table and records drawn for each video's own size + labels"""
    from svit_amd import randaug
    from svit_amd.augment import SpatialSampler
    vids = [torch.from_numpy(x) for x in tight_videos(sizes, T=4, lo=17, span=196)]
    vids = [torch.roll(x, seed, 0) for x in vids]
    random.seed(seed)
    np.random.seed(seed)
    aug = randaug.RandAugSampler(AA, INTERP)
    spatial = SpatialSampler(S, scale=(0.5, 1.0), aspect=(0.75, 1.3333), re_prob=1.0, re_mode="pixel")
    table = [aug.draw(4, h, w, video=v) for v, (h, w) in enumerate(sizes)]
    recs = [spatial.draw(h, w, video=v) for v, (h, w) in enumerate(sizes)]
    return vids, recs, torch.roll(P.labels(len(sizes)), seed, 0), table


def direct_clips(batch):
    from svit_amd.augment import AugClips, pack_videos
    vids, recs, _, table = batch
    frames, ext = pack_videos(vids, Hs=HS, Ws=WS)
    return AugClips(frames.cuda(), S, recs, randaug=table, extents=ext)


def assert_target_is(target, static_labels, direct, labels):
    torch.cuda.synchronize()
    assert torch.equal(target.raw if direct.raw is not None else target.frames,
                       direct.raw if direct.raw is not None else direct.frames)
    assert torch.equal(target.records, direct.records)
    assert (target.extents is None) == (direct.extents is None)
    if direct.extents is not None:
        assert torch.equal(target.extents, direct.extents)
    if direct.ra_table is not None:
        assert torch.equal(target.ra_table, direct.ra_table)
    if isinstance(static_labels, dict):
        for k in static_labels:
            assert torch.equal(static_labels[k], labels[k].to(static_labels[k].device)), k
    else:
        assert torch.equal(static_labels, labels.to(static_labels.device))


@pytest.fixture(scope="module")
def net(ops):
    from svit_amd import losses
    cfg, model, _, _ = SM.build_hip_model(4, 64)
    model.engine.reproducible = True
    fn = losses.VideoImageLoss(cfg)

    def loss_fun(preds, extra, labels):
        return fn.total(fn(preds, extra, labels, {}))
    return cfg, model, loss_fun


MIXES = [[(20, 23), (19, 24)], [(12, 11), (20, 19)], [(3, 3), (20, 24)], [(17, 19), (7, 9)], [(20, 24), (12, 16)]]


@pytest.mark.parametrize("mixed", [False, True])
def test_feeder_is_the_direct_route(F, net, mixed):
    from svit_amd import mixup
    from svit_amd.graph import GraphedTrainStep
    cfg, model, loss_fun = net
    first = video_batch([(20, 24), (20, 24)], 1)
    fn = mixup.MixUp(0.8, 1.0, label_smoothing=0.1, num_classes=174) if mixed else None
    step = GraphedTrainStep(model, loss_fun, [direct_clips(first)], first[2].cuda(), mixup=fn)
    mixes = [mixup.MixRecord(1, 0.3, 0, 0, 0, 0), mixup.MixRecord(2, 0.75, 10, 40, 5, 50), mixup.NO_MIX] if mixed else [None]
    seen = []
    with F.ClipFeeder.for_step(step, depth=2) as feeder:
        assert feeder.slot_bytes % 16 == 0 and feeder.target is step.static_inputs[0]
        for i, sizes in enumerate(MIXES[:3] if mixed else MIXES):           # depth 2: each slot is reused
            batch = video_batch(sizes, 2 + i)
            vids, recs, labels, table = batch
            direct = direct_clips(batch)
            feeder.put(vids, recs, labels, randaug=table)
            inputs, static_labels = feeder.next()
            assert inputs[0] is step.static_inputs[0] and static_labels is step.static_labels
            assert_target_is(inputs[0], static_labels, direct, labels)
            mix = mixes[i % len(mixes)]
            loss, _ = step(inputs, static_labels, mix=mix)
            feeder.pump()
            torch.cuda.synchronize()
            got = (loss.clone(), model.flat.grad.clone())
            loss, _ = step([direct], labels.cuda(), mix=mix)
            torch.cuda.synchronize()
            assert torch.isfinite(got[0]) and float(got[1].abs().max()) > 0
            assert torch.equal(got[0], loss), (sizes, float(got[0]), float(loss))
            assert torch.equal(got[1], model.flat.grad), (sizes, int((got[1] != model.flat.grad).sum()))
            seen.append(float(loss))
    assert len(set(seen)) == len(seen)


def test_feeder_refuses_what_the_direct_route_refuses(F):
    from svit_amd.augment import AugClips
    frames = torch.zeros((2, 1, 12, 16, 3), dtype=torch.uint8, device="cuda")
    recs = [R(0, 0, 0, 12, 16, 8, 8), R(1, 0, 0, 12, 16, 8, 8)]
    y = torch.zeros(2, dtype=torch.int64, device="cuda")
    vids = FC.random_videos([(12, 16), (9, 11)], 1, seed=1)
    with F.ClipFeeder(AugClips(frames, 8, recs, extents=[(12, 16)] * 2), y) as feeder:
        with pytest.raises(ValueError, match="augmentation record 1: source rectangle outside the extent"):
            feeder.put(vids, recs, torch.zeros(2, dtype=torch.int64))
        with pytest.raises(ValueError, match="larger than the 12x16 buffer"):
            feeder.put(FC.random_videos([(12, 16), (13, 16)], 1, seed=1), recs, torch.zeros(2, dtype=torch.int64))
        with pytest.raises(ValueError, match="holds 2 videos"):
            feeder.put(vids[:1], recs, torch.zeros(2, dtype=torch.int64))
        with pytest.raises(ValueError, match="without RandAugment"):
            feeder.put(vids, [recs[0], R(1, 0, 0, 9, 11, 8, 8)], torch.zeros(2, dtype=torch.int64), randaug=[[]])
        with pytest.raises(ValueError, match="the step holds"):
            feeder.put(vids, [recs[0], R(1, 0, 0, 9, 11, 8, 8)], torch.zeros(3, dtype=torch.int64))
        assert feeder.pending == 0
    with F.ClipFeeder(AugClips(frames, 8, recs), y) as feeder:                 # no extents: exactly Hs x Ws
        with pytest.raises(ValueError, match="takes exactly 12x16"):
            feeder.put(vids, recs, torch.zeros(2, dtype=torch.int64))
        full = FC.random_videos([(12, 16), (12, 16)], 1, seed=2)
        feeder.put(full, recs, torch.tensor([5, 6]))
        inputs, labels = feeder.next()
        torch.cuda.synchronize()
        assert np.array_equal(inputs[0].frames.cpu().numpy(), np.stack(full)) and labels.tolist() == [5, 6]


# ------------------------------------------------------------------------------------------------------ 5. image rank ----
def test_image_rank_stills_and_label_tree(F):
    from svit_amd import losses
    from svit_amd.augment import AugClips, pack_videos
    from svit_amd.graph import GraphedTrainStep
    from tests.test_image_rank_u8_gpu import PARTS, SIZES, draw_batch
    cfg, model, _, _ = SM.build_hip_model(4, 64)
    model.engine.reproducible = True
    fn = losses.VideoImageLoss(cfg, is_video_rank=False)

    def loss_fun(preds, extra, labels):
        d = fn(preds, extra, None, labels)
        d["loss"] = fn.total(d)
        return d

    def direct_of(batch):
        _, _, vids, recs, table, _ = batch
        frames, ext = pack_videos([torch.from_numpy(v) for v in vids], Hs=HS, Ws=WS)
        return AugClips(frames.cuda(), S, recs, randaug=table, extents=ext)

    first = draw_batch(SIZES, 1)
    step = GraphedTrainStep(model, loss_fun, [direct_of(first)], {k: v.cuda() for k, v in first[5].items()})
    with F.ClipFeeder.for_step(step) as feeder:
        for sizes, seed in (([(12, 16), (20, 24), (7, 9)], 2), ([(3, 3), (20, 19), (16, 24)], 3), (SIZES, 4)):
            batch = draw_batch(sizes, seed)
            _, _, vids, recs, table, meta = batch
            assert tuple(vids[0].shape[:1]) == (1,)
            feeder.put(vids, recs, meta, randaug=table)
            inputs, labels = feeder.next()
            direct = direct_of(batch)
            assert_target_is(inputs[0], labels, direct, meta)
            assert set(labels) == {"haog_bboxes", "contact_state"} and labels is step.static_labels
            step(inputs, labels)
            torch.cuda.synchronize()
            got = {k: step.loss_dict[k].clone() for k in PARTS + ("loss",)}
            grad = model.flat.grad.clone()
            step([direct], {k: v.cuda() for k, v in meta.items()})
            torch.cuda.synchronize()
            for k in got:
                assert torch.equal(got[k], step.loss_dict[k]), (sizes, k)
            assert float(got["boxes_l1_loss"]) > 0 and torch.equal(grad, model.flat.grad)


# -------------------------------------------------------------------------------------------------- 6. slot discipline ----
def bare_target(V=3, T=2, Hs=12, Ws=16):
    from svit_amd.augment import AugClips
    frames = torch.full((V, T, Hs, Ws, 3), 0xEE, dtype=torch.uint8, device="cuda")
    clips = AugClips(frames, 8, [R(v, 0, 0, Hs, Ws, 8, 8) for v in range(V)], extents=[(Hs, Ws)] * V)
    return clips, torch.zeros(V, dtype=torch.int64, device="cuda")


def bare_batch(k, V=3, T=2, Hs=12, Ws=16):
    sizes = [FC.candidates(Hs, Ws)[(k + v) % len(FC.candidates(Hs, Ws))] for v in range(V)]
    vids = FC.random_videos(sizes, T, seed=50 + k)
    recs = [R(v, 0, 0, h, w, 8, 8, flip=k % 2) for v, (h, w) in enumerate(sizes)]
    return vids, recs, torch.arange(V) + 10 * k


def assert_bare(target, labels, batch):
    from svit_amd.augment import pack_records, pack_videos
    vids, recs, y = batch
    torch.cuda.synchronize()
    frames, ext = pack_videos([torch.from_numpy(v) for v in vids], Hs=target.frames.shape[2], Ws=target.frames.shape[3])
    assert torch.equal(target.frames.cpu(), frames) and torch.equal(target.extents.cpu(), ext)
    assert torch.equal(target.records.cpu(), pack_records(recs)) and torch.equal(labels.cpu(), y)


def test_slot_discipline(F):
    target, y = bare_target()
    with F.ClipFeeder(target, y, depth=2) as feeder:
        with pytest.raises(F.FeederEmpty):
            feeder.next()
        feeder.put(*bare_batch(0), timeout=0)
        feeder.put(*bare_batch(1), timeout=0)
        with pytest.raises(F.FeederFull):
            feeder.put(*bare_batch(2), timeout=0)
        assert feeder.pending == 2 and feeder.pump() == 2 and feeder.pump() == 0
        inputs, labels = feeder.next()
        torch.cuda.synchronize()
        assert_bare(inputs[0], labels, bare_batch(0))              # FIFO
        feeder.put(*bare_batch(2), timeout=0)                      # the first slot is free again
        feeder.next()
        assert_bare(target, y, bare_batch(1))
        feeder.next()
        assert_bare(target, y, bare_batch(2))
        with pytest.raises(F.FeederEmpty):
            feeder.next()
    with pytest.raises(RuntimeError, match="closed"):
        feeder.put(*bare_batch(0), timeout=0)
    # depth 1: the one pinned slot and the one device slot are each rewritten behind their events
    target, y = bare_target()
    with F.ClipFeeder(target, y, depth=1) as feeder:
        feeder.put(*bare_batch(3))
        feeder.next()
        feeder.put(*bare_batch(4))
        torch.cuda.synchronize()
        assert_bare(target, y, bare_batch(3))
        feeder.next()
        torch.cuda.synchronize()
        assert_bare(target, y, bare_batch(4))


def test_producer_thread_feeds_in_order(F):
    target, y = bare_target()
    main = threading.get_ident()
    threads = []

    def batches():
        for k in range(6):
            threads.append(threading.get_ident())
            yield bare_batch(k)
    with F.ClipFeeder(target, y, depth=2) as feeder:
        producer = F.Producer(feeder, batches())
        producer.start()
        for k in range(6):
            producer.wait_ready()
            inputs, labels = feeder.next()
            assert_bare(inputs[0], labels, bare_batch(k))
            feeder.pump()
        with pytest.raises(F.FeederEmpty):
            producer.wait_ready()
        producer.stop()
    assert len(threads) == 6 and main not in threads


# ------------------------------------------------------------------------------------------- 7. train_epoch(feeder=) ----
def test_train_epoch_with_a_feeder_is_the_epoch_by_hand(F):
    from svit_amd import losses, meters, optim, train
    from svit_amd.graph import GraphedTrainStep
    from tests.test_meters_gpu import numbers
    cfg, ma, _, _ = SM.build_hip_model(4, 64)
    _, mb, _, _ = SM.build_hip_model(4, 64)
    ma.engine.reproducible = mb.engine.reproducible = True
    cfg.LOG_PERIOD = 2
    fn, wl = losses.VideoImageLoss(cfg), losses.get_lambdas_dict(cfg)

    def loss_fun(p, e, y):
        d = fn(p, e, y, {})
        d["loss"] = sum(wl[k] * d[k] for k in d)
        return d

    first = video_batch([(20, 24), (20, 24)], 1)
    loader = [video_batch(sizes, 2 + i) for i, sizes in enumerate(MIXES[:4])]
    a = optim.GuardedClipAdamW(ma, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    b = optim.GuardedClipAdamW(mb, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    meter_a, meter_b = meters.TrainMeter(len(loader), cfg), meters.TrainMeter(len(loader), cfg)
    step_a = GraphedTrainStep(ma, loss_fun, [direct_clips(first)], first[2].cuda(), optimizer=a, meter=meter_a)
    step_b = GraphedTrainStep(mb, loss_fun, [direct_clips(first)], first[2].cuda(), optimizer=b, meter=meter_b)
    torch.cuda.synchronize()
    assert torch.equal(ma.flat.data, mb.flat.data)
    lines_a, lines_b = [], []
    log_a = meter_a.log_iter_stats
    meter_a.log_iter_stats = lambda e, i: lines_a.append(numbers(log_a(e, i)))
    with F.ClipFeeder.for_step(step_a) as feeder:
        with pytest.raises(ValueError, match="another step"):
            train.train_epoch([], step_b, b, meter_b, 0, cfg, feeder=feeder)
        host_loader = [(vids, recs, labels, None, {}, table) for vids, recs, labels, table in loader]
        epoch_a = numbers(train.train_epoch(host_loader, step_a, a, meter_a, 0, cfg, feeder=feeder))
        assert feeder.pending == 0
    for i, batch in enumerate(loader):
        optim.set_lr(b, optim.get_lr_at_epoch(cfg, i / float(len(loader)))["lr"])
        step_b([direct_clips(batch)], batch[2].cuda())
        lines_b.append(numbers(meter_b.log_iter_stats(0, i)))
    epoch_b = numbers(meter_b.log_epoch_stats(0))
    torch.cuda.synchronize()
    assert epoch_a == epoch_b and lines_a == lines_b and [l is not None for l in lines_a] == [False, True, False, True]
    assert set(epoch_a) >= {"loss_ce", "loss", "lr"} and a.stats()["applied"] == 4 == b.stats()["applied"]
    for name, x, y in (("weights", ma.flat.data, mb.flat.data), ("exp_avg", a.exp_avg, b.exp_avg),
                       ("exp_avg_sq", a.exp_avg_sq, b.exp_avg_sq)):
        assert torch.equal(x, y), (name, int((x != y).sum()))


# ------------------------------------------------------------------------------------ 8. feeders as accumulated batches ----
def test_accumulated_step_takes_feeders(F):
    from svit_amd.augment import AugClips, pack_videos
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    from svit_amd.hip import SvitHipError
    from tests import test_accumulate_gpu as TA
    from tests.test_image_rank_u8_gpu import SIZES, draw_batch
    cfg, model = TA.build(mode="reproducible")
    opt = TA.optimizer_for(model)

    def stills_of(batch):
        _, _, vids, recs, table, _ = batch
        frames, ext = pack_videos([torch.from_numpy(v) for v in vids], Hs=HS, Ws=WS)
        return AugClips(frames.cuda(), S, recs, randaug=table, extents=ext)

    v0, i0 = video_batch([(20, 24), (20, 24)], 1), draw_batch(SIZES, 1)
    video = GraphedTrainStep(model, TA.loss_of(cfg, False), [direct_clips(v0)], v0[2].cuda(), accumulate=True)
    image = GraphedTrainStep(model, TA.loss_of(cfg, True), [stills_of(i0)], {k: v.cuda() for k, v in i0[5].items()},
                             accumulate=True)
    step = AccumulatedTrainStep(model, [video, image], opt)
    with F.ClipFeeder.for_step(video) as fv, F.ClipFeeder.for_step(image) as fi:
        with pytest.raises(SvitHipError, match="micro-step 0: the feeder was built over another"):
            step([fi, fv])
        for k, (sizes, still_sizes) in enumerate(((MIXES[0], [(12, 16), (20, 24), (7, 9)]), (MIXES[1], [(3, 3), (20, 19), (16, 24)]))):
            vb, ib = video_batch(sizes, 5 + k), draw_batch(still_sizes, 5 + k)
            snap = TA.snapshot(model, opt)
            fv.put(vb[0], vb[1], vb[2], randaug=vb[3])
            fi.put(ib[2], ib[3], ib[5], randaug=ib[4])
            losses = step([fv, fi])
            got = TA.state_bits(model, opt) + [torch.stack([l.detach() for l in losses]).clone().view(torch.int32)]
            assert fv.pending == 0 and fi.pending == 0
            TA.restore(model, opt, snap)
            losses = step([([direct_clips(vb)], vb[2].cuda()), ([stills_of(ib)], {k: v.cuda() for k, v in ib[5].items()})])
            want = TA.state_bits(model, opt) + [torch.stack([l.detach() for l in losses]).clone().view(torch.int32)]
            TA.assert_bits(got, want, "accumulated step %d" % k)
            assert float(model.flat.grad.abs().max()) > 0
