"""Per-video extents on the uint8 input route, on the device: videos of different sizes in one padded buffer get, byte for
byte, what each would get alone as a tight clip -- RandAugment (`svit_randaug_*_ext`), the spatial stage
(`svit_im2col_patch_u8_aug[_frames]_ext`, `svit_u8_clips_render_ext`) and a captured step that serves any mix of sizes.

Shapes: T = 2, window S = 8; a 12 x 16 buffer (under one 256-pixel block) with videos 12x16, 9x16, 12x11 (33 row bytes)
and 3x3; a 20 x 24 buffer (two blocks) with one 17x19 video (57 row bytes).  The padding holds a pattern of 0 and 255,
never zeros only: a kernel that reads or counts it gives other bytes.  (Equalize is the identity on a frame of
fewer than 255 pixels, so the statistics test uses the larger buffer: 17x19 and 20x15.)"""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import randaug_cases as RC
from tests import smoke_impl as SM
from tests.test_augment_gpu import MEAN, STD, R, _mix, bits
from tests.test_randaug_gpu import _mixed_table

T, S = 2, 8
BUFFERS = [((12, 16), [(12, 16), (9, 16), (12, 11), (3, 3)]), ((20, 24), [(17, 19)])]
MARGIN = 4096


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import ops
    return ops


@pytest.fixture(scope="module")
def ra(ops):
    from svit_amd import randaug
    return randaug


def tight_videos(sizes, T=T, lo=0, span=256):
    """NumPy u8 [T,h,w,3] per size, a different closed-form video each (values in [lo, lo + span))"""
    out = []
    for k, (h, w) in enumerate(sizes):
        x = RC.source((k + 1, T, h, w, 3))[k].astype(np.int64)
        out.append((lo + x * span // 256).astype(np.uint8))
    return out


def padded(vids, Hs, Ws):
    """the videos in the top-left corners of a u8 [V,T,Hs,Ws,3] buffer whose padding alternates 0 and 255"""
    V, T_ = len(vids), vids[0].shape[0]
    idx = np.arange(V * T_ * Hs * Ws * 3).reshape(V, T_, Hs, Ws, 3)
    buf = np.where((idx // 3 + idx // 7) % 2 == 0, 0, 255).astype(np.uint8)
    for v, x in enumerate(vids):
        buf[v, :, :x.shape[1], :x.shape[2]] = x
    return buf


def outside_mask(sizes, Hs, Ws):
    m = np.ones((len(sizes), 1, Hs, Ws, 1), dtype=bool)
    for v, (h, w) in enumerate(sizes):
        m[v, :, :h, :w] = False
    return m


def guarded(shape, dtype, fill):
    """a tensor of `shape` in the middle of an allocation with canary margins -> (tensor, check())"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((nbytes + 2 * MARGIN,), 0x5C, dtype=torch.uint8, device="cuda")
    t = raw[MARGIN:MARGIN + nbytes].view(dtype).view(shape)
    t.copy_(fill if torch.is_tensor(fill) else torch.full(shape, fill, dtype=dtype))

    def check():
        assert bool((raw[:MARGIN] == 0x5C).all()) and bool((raw[MARGIN + nbytes:] == 0x5C).all()), "canary overwritten"
    return t, check


def device_apply(ra, src_np, table, extents):
    """the 2N kernels on a NumPy batch -> NumPy; every buffer sits between canaries, dst / tmp start poisoned and src
    must come back unchanged.  extents: None, or ANY int [V,2] table (uploaded as it is)"""
    table = ra.pack_table(table)
    V, T_ = src_np.shape[:2]
    checks = []

    def buf(shape, dtype, fill):
        t, c = guarded(shape, dtype, fill)
        checks.append(c)
        return t
    src = buf(src_np.shape, torch.uint8, torch.from_numpy(np.ascontiguousarray(src_np)))
    dst, tmp = buf(src_np.shape, torch.uint8, 77), buf(src_np.shape, torch.uint8, 99)
    ws = buf((ra.workspace_bytes(V, T_),), torch.uint8, 0)
    tab = buf(table.shape, torch.int32, torch.from_numpy(table))
    ext = None if extents is None else buf((V, 2), torch.int32, torch.tensor(np.asarray(extents).tolist(), dtype=torch.int32))
    out = ra.apply(src, tab, dst, tmp if table.shape[1] > 1 else None, ws, extents=ext)
    torch.cuda.synchronize()
    assert out is dst and np.array_equal(src.cpu().numpy(), src_np)
    for c in checks:
        c()
    return dst.cpu().numpy()


def diff(a, b):
    return int((a != b).sum())


def case_table(ra, sizes):
    """every case of randaug_cases for every video, drawn for the video's own size: row c*V + v"""
    return [[ra.make_op(name, args, () if filt is None else (filt,) * T, h, w)]
            for name, args, filt in RC.single_cases() for h, w in sizes]


# ------------------------------------------------------------------------------------------------- 1. RandAugment ----
@pytest.mark.parametrize("buf", range(len(BUFFERS)))
def test_randaugment_inside_the_extent_is_the_tight_video(ra, buf):
    (Hs, Ws), sizes = BUFFERS[buf]
    cases, V = RC.single_cases(), len(sizes)
    vids = tight_videos(sizes)
    batch = np.tile(padded(vids, Hs, Ws), (len(cases), 1, 1, 1, 1))            # the cases as videos: one launch pair
    ext = np.tile(np.array(sizes), (len(cases), 1))
    table = case_table(ra, sizes)
    got = device_apply(ra, batch, table, ext)
    out = np.tile(outside_mask(sizes, Hs, Ws), (len(cases), T, 1, 1, 3))
    assert np.array_equal(got[out], batch[out])                                 # every byte outside the extents is the input's
    changed = 0
    for v, (h, w) in enumerate(sizes):
        tight = np.repeat(vids[v][None], len(cases), axis=0)
        tt = table[v::V]
        on_device = device_apply(ra, tight, tt, None)                            # the existing kernels on the tight copy
        on_host = ra.apply_host(tight, tt)                                       # the PIL-exact yardstick
        for c, case in enumerate(cases):
            corner = got[c * V + v, :, :h, :w]
            assert diff(corner, on_device[c]) == 0, (case, (h, w), diff(corner, on_device[c]))
            assert diff(corner, on_host[c]) == 0, (case, (h, w), diff(corner, on_host[c]))
            changed += diff(corner, vids[v]) > 0
            if case[0].startswith("Sharpness"):
                # PIL leaves the border ring of the image alone: the TRUE last row and column, not the buffer's
                assert np.array_equal(corner[:, h - 1], vids[v][:, h - 1]) and np.array_equal(corner[:, :, w - 1], vids[v][:, :, w - 1])
                assert np.array_equal(corner[:, 0], vids[v][:, 0]) and np.array_equal(corner[:, :, 0], vids[v][:, :, 0])
                assert h == 3 or diff(corner[:, 1:h - 1, 1:w - 1], vids[v][:, 1:h - 1, 1:w - 1]) > 0
    assert changed > len(cases) * V // 2


@pytest.mark.parametrize("buf", range(len(BUFFERS)))
def test_randaugment_chains_inside_the_extent(ra, buf):
    """two whole 4-layer chains per video (mixed filters across the frames; Equalize, AutoContrast, Contrast and
    Sharpness behind a geometric layer, so the statistics see the fill)"""
    (Hs, Ws), sizes = BUFFERS[buf]
    vids = tight_videos(sizes)
    for k in range(2):
        table = [_mixed_table(ra, h, w)[k] for h, w in sizes]
        batch = padded(vids, Hs, Ws)
        got = device_apply(ra, batch, table, sizes)
        out = np.broadcast_to(outside_mask(sizes, Hs, Ws), batch.shape)
        assert np.array_equal(got[out], batch[out])
        for v, (h, w) in enumerate(sizes):
            corner = got[v, :, :h, :w]
            on_device = device_apply(ra, vids[v][None], [table[v]], None)[0]
            on_host = ra.apply_host(vids[v][None], [table[v]])[0]
            assert diff(corner, on_device) == 0 and diff(corner, on_host) == 0, (k, (h, w))
            assert diff(corner, vids[v]) > 0


@pytest.mark.parametrize("op", ["OP_AUTOCONTRAST", "OP_EQUALIZE", "OP_CONTRAST"])
def test_statistics_do_not_count_the_padding(ra, op):
    """videos with bytes in [60, 180) inside padding of 0 and 255: counted, the padding would make AutoContrast the
    identity, flatten Equalize's table and move the Contrast mean -- the plain entry points show that it would"""
    (Hs, Ws), sizes = BUFFERS[1][0], [(17, 19), (20, 15)]    # (Equalize is the identity below 255 pixels: the larger buffer)
    vids = tight_videos(sizes, lo=60, span=120)
    batch = padded(vids, Hs, Ws)
    rec = ra.RandAugOp(getattr(ra, op), arg_f=1.7)
    table = [[rec]] * len(sizes)
    got = device_apply(ra, batch, table, sizes)
    blind = device_apply(ra, batch, table, None)
    for v, (h, w) in enumerate(sizes):
        want = ra.apply_host(vids[v][None], [[rec]])[0]
        assert diff(got[v, :, :h, :w], want) == 0
        assert diff(want, vids[v]) > 0 and diff(blind[v, :, :h, :w], want) > 0


# ----------------------------------------------------------------------------------------------- 2. spatial stage ----
def erase(rec, mode, box, seed):
    return rec._replace(erase_mode=mode, et=box[0], el=box[1], eh=box[2], ew=box[3], seed=seed)


def records_for(sizes):
    """per video: a resized crop that touches the extent's far edges (the taps there clamp, they do not read padding),
    flip, every erase mode, and the test-mode record drawn for the video's own size"""
    from svit_amd.augment import SpatialSampler
    test_mode = SpatialSampler(S, spatial_sampling="uniform", random_flip=False)
    recs = []
    for v, (h, w) in enumerate(sizes):
        ch, cw = max(h - 1, 1), max(w - 2, 1)
        crop = R(v, h - ch, w - cw, ch, cw, S, S, flip=v % 2)
        recs.append(erase(crop, 1 + v % 3, (1, 2, 4, 5), 7 + v) if v else crop)
        recs.append(R(v, 0, 0, h, w, S + 2, S + 1, oy=2, ox=1, flip=1 - v % 2))
        np.random.seed(v)
        recs.append(test_mode.draw(h, w, video=v, spatial_idx=v % 3))
    recs.append(erase(R(0, 0, 0, sizes[0][0], sizes[0][1], S, S), 3, (0, 3, 8, 4), 11))
    return recs


def spatial_outputs(ops, clips):
    from svit_amd.input import FramesView
    cols, thw = ops.im2col_patch_u8_aug(clips)
    fcols, fthw = ops.im2col_patch_u8_aug_frames(FramesView(clips))
    render = clips.render()
    torch.cuda.synchronize()
    B = clips.shape[0]
    return cols.view(B, -1, 448), fcols.view(B, -1, 448), render


def ragged_and_tight(ops, buf):
    """the ragged AugClips of one buffer and, per clip b, the outputs of a one-video AugClips over the tight copy with
    the same record at row b (video = 0; the erase noise is keyed by the clip's row)"""
    from svit_amd.augment import AugClips
    (Hs, Ws), sizes = BUFFERS[buf]
    vids = tight_videos(sizes)
    recs = records_for(sizes)
    frames, check = guarded((len(sizes), T, Hs, Ws, 3), torch.uint8, torch.from_numpy(padded(vids, Hs, Ws)))
    clips = AugClips(frames, S, recs, mean=MEAN, std=STD, extents=sizes)
    tight = []
    for b, rec in enumerate(recs):
        alone = AugClips(torch.from_numpy(vids[rec.video][None]).cuda(), S, [rec._replace(video=0)] * len(recs),
                         mean=MEAN, std=STD)
        tight.append(tuple(o[b] for o in spatial_outputs(ops, alone)))
    return clips, recs, tight, check


@pytest.mark.parametrize("buf", range(len(BUFFERS)))
def test_spatial_stage_reads_each_clip_through_its_own_extent(ops, buf):
    clips, recs, tight, check = ragged_and_tight(ops, buf)
    cols, fcols, render = spatial_outputs(ops, clips)
    assert tuple(cols.shape) == (len(recs), 4, 448) and tuple(fcols.shape) == (len(recs), T * 4, 448)
    for b, rec in enumerate(recs):
        assert torch.equal(bits(cols[b]), bits(tight[b][0])), (b, rec)
        assert torch.equal(bits(fcols[b]), bits(tight[b][1])), (b, rec)
        assert torch.equal(bits(render[b]), bits(tight[b][2])), (b, rec)
    check()


@pytest.mark.parametrize("buf", range(len(BUFFERS)))
def test_mix_partner_is_sampled_through_its_own_extent(ops, buf):
    """mixup and CutMix: clip b against clip B-1-b, a clip of another video with another extent -- the operand is the
    fp32 route's (mix of the TIGHT renders, one rounding), clip pass and frames pass"""
    from svit_amd.input import FramesView
    clips, recs, tight, check = ragged_and_tight(ops, buf)
    plain = ops.im2col_patch_u8_aug(clips)[0]
    render = torch.stack([t[2] for t in tight]).contiguous()
    for m in (_mix(1, 0.3), _mix(2, 0.75, (1, 7, 0, 5))):
        record = torch.from_numpy(m.pack()).cuda()
        clips.mix = record
        mixed = ops.mixup_clips(render.clone(), record)
        want = ops.im2col_patch(mixed)[0]
        got = ops.im2col_patch_u8_aug(clips)[0]
        assert torch.equal(bits(got), bits(want)), m
        assert not torch.equal(bits(got), bits(plain))
        fwant = ops.im2col_patch(mixed.transpose(1, 2).flatten(0, 1).unsqueeze(2).contiguous())[0]
        fgot = ops.im2col_patch_u8_aug_frames(FramesView(clips))[0]
        assert torch.equal(bits(fgot), bits(fwant)), m
    check()


def test_augclips_hands_the_extents_to_the_chain(ops, ra):
    """AugClips(randaug=, extents=): `frames` holds the chain's output per extent, and clone / copy_ / set_extents
    carry the table"""
    from svit_amd.augment import AugClips
    (Hs, Ws), sizes = BUFFERS[0]
    vids = tight_videos(sizes)
    recs = records_for(sizes)
    table = [_mixed_table(ra, h, w)[v % 2] for v, (h, w) in enumerate(sizes)]
    batch = padded(vids, Hs, Ws)
    clips = AugClips(torch.from_numpy(batch).cuda(), S, recs, mean=MEAN, std=STD, randaug=table, extents=sizes)
    want = AugClips(torch.from_numpy(ra.apply_host(batch, table, sizes)).cuda(), S, recs, mean=MEAN, std=STD, extents=sizes)
    assert torch.equal(clips.render(), want.render()) and torch.equal(clips.frames, want.frames)
    twin = clips.clone()
    assert twin.extents.data_ptr() != clips.extents.data_ptr() and torch.equal(twin.extents, clips.extents)
    assert torch.equal(twin.render(), want.render())
    # another mix of sizes through copy_ and through set_extents + set_records
    sizes2 = [(9, 12), (12, 16), (5, 16), (12, 7)]
    vids2 = tight_videos(sizes2)
    recs2 = records_for(sizes2)[:len(recs)]
    table2 = [_mixed_table(ra, h, w)[1 - v % 2] for v, (h, w) in enumerate(sizes2)]
    batch2 = padded(vids2, Hs, Ws)
    other = AugClips(torch.from_numpy(batch2).cuda(), S, recs2, mean=MEAN, std=STD, randaug=table2, extents=sizes2)
    want2 = AugClips(torch.from_numpy(ra.apply_host(batch2, table2, sizes2)).cuda(), S, recs2, mean=MEAN, std=STD,
                     extents=sizes2).render()
    twin.copy_(other)
    assert torch.equal(twin.render(), want2)
    clips.raw.copy_(other.raw)
    clips.set_randaug(table2).set_extents(sizes2).set_records(recs2)
    assert torch.equal(clips.render(), want2)
    # the refusals
    u8 = torch.from_numpy(batch).cuda()
    with pytest.raises(ValueError, match="smaller than 3x3"):
        AugClips(u8, S, recs[:1], randaug=table, extents=[(12, 16), (2, 16), (12, 11), (3, 3)])
    with pytest.raises(ValueError, match="larger than the 12x16 buffer"):
        AugClips(u8, S, recs[:1], extents=[(12, 17), (9, 16), (12, 11), (3, 3)])
    with pytest.raises(ValueError, match="augmentation record 0: source rectangle outside the extent"):
        AugClips(u8, S, [R(1, 0, 0, 10, 16, S, S)], extents=sizes)
    with pytest.raises(ValueError, match="record 0"):
        clips.set_records([R(3, 0, 0, 12, 8, S, S)] * len(recs))          # video 3 is 12x7 now: checked against the new table
    with pytest.raises(ValueError, match="without extents"):
        AugClips(u8, S, recs[:1]).set_extents(sizes)
    with pytest.raises(ValueError, match="with and without extents"):
        AugClips(u8, S, recs).copy_(AugClips(u8, S, recs, extents=sizes))


def test_u8clips_checks_its_crops_against_the_extents():
    from svit_amd.input import U8Clips
    (Hs, Ws), sizes = BUFFERS[0]
    u8 = torch.from_numpy(padded(tight_videos(sizes), Hs, Ws)).cuda()
    ok = U8Clips(u8, S, torch.tensor([[0, 4, 8], [1, 1, 8], [2, 4, 3]], dtype=torch.int32), extents=sizes)
    assert ok.clone().extents.tolist() == [list(s) for s in sizes]
    for row in ([1, 2, 0], [2, 0, 4], [3, 0, 0]):
        U8Clips(u8, S, torch.tensor([[0, 0, 0], row], dtype=torch.int32))               # inside the buffer ...
        with pytest.raises(ValueError, match="crop 1 reaches outside the extent"):
            U8Clips(u8, S, torch.tensor([[0, 0, 0], row], dtype=torch.int32), extents=sizes)


# ------------------------------------------------------------------- 3. no extents, full extents: the old bytes ----
def test_none_and_full_extents_are_the_old_entry_points(ops, ra):
    from svit_amd import hip
    from svit_amd.augment import AugClips
    from svit_amd.input import FramesView
    (Hs, Ws), sizes = BUFFERS[1][0], [BUFFERS[1][0]] * 3
    batch = padded(tight_videos([(Hs - 3, Ws - 5)] * 3), Hs, Ws)
    table = [_mixed_table(ra, Hs, Ws)[v % 2] for v in range(3)]
    old = device_apply(ra, batch, table, None)
    assert np.array_equal(old, ra.apply_host(batch, table))
    assert np.array_equal(device_apply(ra, batch, table, sizes), old)
    # the `_ext` entry points with a null table
    src, dst, tmp = torch.from_numpy(batch).cuda(), torch.empty(batch.shape, dtype=torch.uint8, device="cuda"), None
    tab = torch.from_numpy(ra.pack_table([t[:1] for t in table])).cuda()
    ws = torch.zeros(ra.workspace_bytes(3, T), dtype=torch.uint8, device="cuda")
    hip.call("svit_randaug_stats_ext", src.data_ptr(), tab.data_ptr(), None, 0, ws.data_ptr(), 3, T, Hs, Ws, 1)
    hip.call("svit_randaug_apply_ext", src.data_ptr(), dst.data_ptr(), tab.data_ptr(), None, 0, ws.data_ptr(), 3, T, Hs, Ws, 1)
    assert np.array_equal(dst.cpu().numpy(), device_apply(ra, batch, [t[:1] for t in table], None))
    recs = records_for([(Hs, Ws)] * 3)
    u8 = torch.from_numpy(batch).cuda()
    plain = AugClips(u8, S, recs, mean=MEAN, std=STD)
    full = AugClips(u8, S, recs, mean=MEAN, std=STD, extents=sizes)
    assert plain.extents is None and FramesView(plain).extents is None
    for m in (None, _mix(1, 0.3), _mix(2, 0.75, (1, 7, 0, 5))):
        plain.mix = full.mix = None if m is None else torch.from_numpy(m.pack()).cuda()
        for a, b in zip(spatial_outputs(ops, plain), spatial_outputs(ops, full)):
            assert torch.equal(bits(a), bits(b)), m
    B = len(recs)
    cols = torch.empty((B * 4, 448), dtype=torch.bfloat16, device="cuda")
    hip.call("svit_im2col_patch_u8_aug_ext", u8.data_ptr(), u8.numel(), plain.lut_f32.data_ptr(), plain.records.data_ptr(),
             None, None, cols.data_ptr(), B, T, Hs, Ws, S)
    plain.mix = None
    assert torch.equal(bits(cols), bits(ops.im2col_patch_u8_aug(plain)[0]))
    lib = hip.load()
    assert lib.svit_randaug_stats_ext(16, 16, 18, 0, 16, 1, 1, 8, 8, 1, None) == -3          # extents not 4-byte aligned
    assert lib.svit_u8_clips_render_ext(16, 192, 16, 16, 18, 16, 1, 1, 8, 8, 8, None) == -3


# -------------------------------------------------------------------------------------------- 4. the device clamps ----
def test_any_extents_table_is_clamped_into_the_buffer(ops, ra):
    """(0,0), (-5, 10^9), (Hs+1, 1): the kernels use (1,1), (1,Ws), (Hs,1) -- arithmetic on in-range memory, predicted
    by `clamp_extents` / `clamp_records`; every buffer between canaries"""
    from svit_amd import augment
    from svit_amd.augment import AugClips
    (Hs, Ws), _ = BUFFERS[0]
    wild = [(0, 0), (-5, 10 ** 9), (Hs + 1, 1)]
    clamped = augment.clamp_extents(wild, Hs, Ws)
    assert clamped.tolist() == [[1, 1], [1, Ws], [Hs, 1]]
    batch = padded(tight_videos([(Hs, Ws)] * 3), Hs, Ws)
    for k in range(2):
        table = [_mixed_table(ra, Hs, Ws)[k]] * 3
        got = device_apply(ra, batch, table, wild)
        want = batch.copy()
        for v, (h, w) in enumerate(clamped.tolist()):
            for t in range(T):
                img = batch[v, t, :h, :w]
                for rec in table[v]:
                    img = ra.apply_frame(img, rec, t)
                want[v, t, :h, :w] = img
        assert np.array_equal(got, want), (k, diff(got, want))
    # records reaching past their video's extent are pulled inside it
    sizes = [(12, 16), (9, 16), (12, 11)]
    recs = [R(0, 0, 0, 12, 16, S, S), R(1, 5, 3, 9, 20, S, S, flip=1), R(2, 2, 9, 12, 8, S + 3, S + 3, oy=1, ox=2),
            R(1, -4, 14, 30, 5, S, S), R(2, 11, 10, 3, 3, S, S), R(7, 0, 0, 99, 99, S, S)]
    for ext in (sizes, wild):
        frames, check = guarded((3, T, Hs, Ws, 3), torch.uint8, torch.from_numpy(batch))
        clips = AugClips(frames, S, [recs[0]] * len(recs), mean=MEAN, std=STD, extents=[(Hs, Ws)] * 3)
        clips.set_extents(ext, validate=False).set_records(recs, validate=False)
        pulled = augment.clamp_records(clips.records, 3, Hs, Ws, S, ext)
        e = augment.clamp_extents(ext, Hs, Ws)[pulled[:, 0].numpy()]
        assert bool((pulled[:, 1] + pulled[:, 3] <= torch.from_numpy(e[:, 0])).all())
        assert bool((pulled[:, 2] + pulled[:, 4] <= torch.from_numpy(e[:, 1])).all())
        assert not torch.equal(pulled, augment.clamp_records(clips.records, 3, Hs, Ws, S))
        want = AugClips(frames, S, pulled, mean=MEAN, std=STD)               # inside the buffer: the plain kernels
        for a, b in zip(spatial_outputs(ops, clips), spatial_outputs(ops, want)):
            assert torch.equal(bits(a), bits(b)), ext
        check()


# -------------------------------------------------------------------------------------------- 5. the captured step ----
@pytest.fixture(scope="module")
def net(ops):
    from svit_amd import losses
    cfg, model, spec, sd = SM.build_hip_model(4, 64)
    model.engine.reproducible = True
    cfg.SVIT.CONSISTENCY = "l2"
    loss_mod = losses.VideoImageLoss(cfg)

    def loss_fun(preds, extra, labels):
        return loss_mod.total(loss_mod(preds, extra, labels, {}))

    return model, loss_fun


def step_batch(ra, sizes, seed, Hs=80, Ws=96, T4=4, S64=64):
    """host videos of `sizes` packed into the 80 x 96 buffer + RandAugment table and records drawn for each video's
    own size -> the AugClips arguments"""
    from svit_amd.augment import SpatialSampler, pack_videos
    vids = [torch.from_numpy(x) for x in tight_videos(sizes, T=T4, lo=17, span=196)]
    frames, ext = pack_videos(vids, Hs=Hs, Ws=Ws)
    random.seed(seed)
    np.random.seed(seed)
    aug = ra.RandAugSampler("rand-m7-n4-mstd0.5-inc1", "random")
    spatial = SpatialSampler(S64, scale=(0.5, 1.0), aspect=(0.75, 1.3333), re_prob=1.0, re_mode="pixel")
    table = [aug.draw(T4, h, w, video=v) for v, (h, w) in enumerate(ext.tolist())]
    recs = [spatial.draw(h, w, video=v) for v, (h, w) in enumerate(ext.tolist())]
    return frames, recs, table, ext


@pytest.mark.parametrize("frames_pass", [False, "u8"])
def test_one_captured_step_serves_every_mix_of_sizes(ra, net, frames_pass):
    from svit_amd.augment import AugClips
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.hip import SvitHipError
    from svit_amd.input import FramesView
    model, loss_fun = net
    y = P.labels(2).cuda()

    def clips_of(sizes, seed, **kw):
        frames, recs, table, ext = step_batch(ra, sizes, seed, **kw)
        return AugClips(frames.cuda(), 64, recs, randaug=table, extents=ext)

    def eager(clips):
        model.flat.grad.zero_()
        logits, extra = model([clips], {})
        if frames_pass:
            with torch.no_grad():       # the frames pass as the step runs it (svit_amd/graph.py)
                view = FramesView(clips, fresh=True)
                fy, _ = model.engine.forward(view, model.sample_drop_scales(view.shape[0], y.device), save=False)
                fp, fe = model.head(torch.cat((fy[:, :1], fy[:, -model.O:]), dim=1), T=1)
            extra["frames_output"] = {"preds": fp, "extra_preds": fe}
        loss = loss_fun(logits, extra, y)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), logits.detach().clone(), model.flat.grad.clone()

    step = GraphedTrainStep(model, loss_fun, [clips_of([(80, 96), (80, 96)], 1)], y, frames_pass=frames_pass)
    seen = []
    for sizes, seed in (([(80, 75), (70, 96)], 2), ([(64, 64), (80, 91)], 3)):
        clips = clips_of(sizes, seed)
        want = eager(clips)
        loss, (logits, _) = step([clips], y)
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and float(want[2].abs().max()) > 0
        assert torch.equal(loss, want[0]) and torch.equal(logits, want[1]) and torch.equal(model.flat.grad, want[2]), sizes
        seen.append(float(loss))
    assert seen[0] != seen[1]
    with pytest.raises(SvitHipError, match="captured for a frame buffer"):
        step([clips_of([(80, 75), (70, 100)], 4, Ws=100)], y)
