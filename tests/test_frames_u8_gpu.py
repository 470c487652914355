"""The frames pass straight from uint8 clips (input.FramesView, svit_im2col_patch_u8_aug_frames,
GraphedTrainStep(frames_pass="u8")).

Every value comparison is bit equality: the frames operand and `svit_im2col_patch` of the rendered fp32 frames perform
the same fp32 operations (aug_pixel, the mix) and one bf16 rounding, and with `engine.reproducible` the step behind
equal operands is the same launches on the same bytes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import smoke_impl as SM
from tests.test_augment_gpu import MEAN, STD, R, _mix, bits

AUG_STAGE_FRAMES = 5460         # csrc/input.hip: LDS bytes for the staged rectangle of the frames variant
XO, COLS = 62, 252              # output positions / clip columns per chunk


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import ops
    return ops


def u8_video(T, V=3, side=96):
    video = P.frames(V, T, side)                                  # [V,3,T,96,96], |x| <= 1.7 -> bytes in [17, 212]
    return ((video * 0.225 + 0.45) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()


def random_u8(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


def as_frames(clip):
    """fp32 [B,3,T,S,S] -> the frames pass's input [B*T,3,1,S,S] (tools/train_net.py:105-110)"""
    return clip.transpose(1, 2).flatten(0, 1).unsqueeze(2).contiguous()


def frames_cols(ops, view):
    """ops.im2col_patch_u8_aug_frames, then the same launch into a buffer of bf16 NaNs: no element is left out"""
    from svit_amd import hip
    cols, thw = ops.im2col_patch_u8_aug_frames(view)
    fr, rec = view.frames, view.device_records()
    nan = torch.full(cols.shape, float("nan"), device=fr.device, dtype=torch.bfloat16)
    hip.call("svit_im2col_patch_u8_aug_frames", fr.data_ptr(), fr.numel(), view.lut_f32.data_ptr(), rec.data_ptr(),
             None if view.mix is None else view.mix.data_ptr(), nan.data_ptr(), rec.shape[0], fr.shape[1], fr.shape[2],
             fr.shape[3], view.size)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(nan).any()), "elements left out"
    assert torch.equal(bits(nan), bits(cols))
    return cols, thw


# ------------------------------------------------------------------- the kernel's size predicate, restated ----
def _axis32(dst, n_in, scale):
    """aug_axis of csrc/input.hip in fp32: -> (i0, i1).  The product of two fp32 numbers is exact in float64 and so is
    the sum with -0.5 at these magnitudes: one rounding, like the fma."""
    src = np.float32(np.float64(np.float32(scale)) * np.float64(np.float32(dst) + np.float32(0.5)) - 0.5)
    src = max(src, np.float32(0))
    i0 = min(int(src), n_in - 1)
    return i0, i0 + (1 if i0 < n_in - 1 else 0)


def staged_paths(rec, S):
    """{(yo, chunk): staged?} of the frames variant for one (clamped) record: one frame's rectangle -- the source rows
    of the block's 7 output rows x the source columns of the chunk's COLS output columns, rows padded to words -- is
    staged where it fits AUG_STAGE_FRAMES bytes, gathered otherwise"""
    sy = np.float32(np.float64(rec.h) / np.float64(rec.out_h))
    sx = np.float32(np.float64(rec.w) / np.float64(rec.out_w))
    Ho = Wo = (S - 1) // 4 + 1
    out = {}
    for yo in range(Ho):
        y0 = yo * 4 - 3
        ya, yb = max(y0, 0), min(y0 + 7, S)
        r_lo, r_hi = _axis32(rec.oy + ya, rec.h, sy)[0], _axis32(rec.oy + yb - 1, rec.h, sy)[1]
        nrows = r_hi - r_lo + 1
        for k, xc0 in enumerate(range(0, Wo, XO)):
            x_start = xc0 * 4 - 4
            xa, xb = max(x_start, 0), min(x_start + COLS, S)
            assert xb > xa
            c_lo = _axis32(rec.ox + (S - xb if rec.flip else xa), rec.w, sx)[0]
            c_hi = _axis32(rec.ox + (S - 1 - xa if rec.flip else xb - 1), rec.w, sx)[1]
            pitch = ((c_hi - c_lo + 1) * 3 + 6) & ~3
            out[(yo, k)] = nrows * pitch <= AUG_STAGE_FRAMES
    return out


def paths_of(clips):
    from svit_amd import augment
    V, T, Hs, Ws, _ = clips.frames.shape
    recs = augment.unpack_records(augment.clamp_records(clips.records, V, Hs, Ws, clips.size))
    return [staged_paths(r, clips.size) for r in recs]


# -------------------------------------------------------------------------- 1. the operand against the fp32 route ----
BOX = (6, 5, 13, 10)            # top, left, height, width: rows 6..18, columns 5..14 cross the patch edges at 8, 12, 16
HI, LO = 2 ** 31 - 1, -2 ** 31
IDENT = R(1, 3, 5, 64, 64, 64, 64)
UPSCALE = R(2, 0, 0, 96, 96, 110, 110, oy=17, ox=40)
DOWNSCALE = R(0, 0, 0, 96, 96, 64, 64)
FLIP = R(1, 10, 2, 80, 70, 64, 64, flip=1)
GARBAGE = [R(HI, HI, HI, HI, HI, HI, HI, HI, HI, HI, HI, (HI, HI, HI, HI), HI),
           R(LO, LO, LO, LO, LO, LO, LO, LO, LO, LO, LO, (LO, LO, LO, LO), LO),
           R(99, 1000, -7, 0, -3, 0, 2 ** 30, -4, 10 ** 6, 7, 9, (-3, -3, 10 ** 6, 10 ** 6), -1)]


def erase(mode, rec=IDENT, seed=77):
    return rec._replace(erase_mode=mode, et=BOX[0], el=BOX[1], eh=BOX[2], ew=BOX[3], seed=seed)


CASES = {
    # name: (source shape, S, records, validate, the paths the size predicate must report)
    "identity_b1_t1": ((3, 1, 96, 96, 3), 64, [IDENT], True, {True}),
    "resample_b2_t3": ((3, 3, 96, 96, 3), 64, [UPSCALE, DOWNSCALE], True, {True}),
    "flip_erase_b3_t4": ((3, 4, 96, 96, 3), 64, [FLIP, erase(1, DOWNSCALE), erase(2, UPSCALE)], True, {True}),
    "erase_b3_t3": ((3, 3, 96, 96, 3), 64, [erase(3), erase(3, FLIP, seed=5), erase(1)], True, {True}),
    "erase_b1_t4": ((3, 4, 96, 96, 3), 64, [erase(2, FLIP)], True, {True}),
    "garbage_b3_t4": ((3, 4, 96, 96, 3), 64, GARBAGE, False, {True}),
    # S % 4 != 0; 96 -> 30 resamples 7 output rows from 21 source rows of 294 bytes: the inner blocks gather
    "s30_b2_t3": ((3, 3, 96, 96, 3), 30, [R(0, 0, 0, 96, 96, 30, 30, flip=1), R(2, 20, 30, 30, 30, 30, 30)], True,
                  {True, False}),
    # Wo = 63: the first chunk's 248 columns are too wide to stage, the second chunk holds the single last column
    "s252_b2_t2": ((2, 2, 260, 300, 3), 252, [R(1, 0, 0, 260, 300, 252, 252), erase(3, R(0, 4, 31, 252, 252, 252, 252))],
                   True, {True, False}),
}


def build_case(name):
    from svit_amd.augment import AugClips
    shape, S, recs, validate, want_paths = CASES[name]
    u8 = (u8_video(shape[1]) if shape[2:4] == (96, 96) else random_u8(shape, 12)).cuda()
    assert tuple(u8.shape) == shape
    if validate:
        clips = AugClips(u8, S, recs, mean=MEAN, std=STD)
    else:
        clips = AugClips(u8, S, [IDENT] * len(recs), mean=MEAN, std=STD)
        clips.set_records(recs, validate=False)
    return clips, want_paths


@pytest.mark.parametrize("name", list(CASES))
def test_operand_equals_im2col_of_the_rendered_frames(ops, name):
    from svit_amd.input import FramesView
    clips, want_paths = build_case(name)
    B, _, T, S, _ = clips.shape
    view = FramesView(clips)
    assert tuple(view.shape) == (B * T, 3, 1, S, S) and view.dim() == 5 and view.device == clips.device
    got, thw = frames_cols(ops, view)
    want, thw_ref = ops.im2col_patch(as_frames(clips.render()))
    torch.cuda.synchronize()
    Ho = (S - 1) // 4 + 1
    assert thw == thw_ref == (1, Ho, Ho) and tuple(got.shape) == (B * T * Ho * Ho, 448)
    assert torch.equal(bits(got), bits(want))
    # the temporal padding: only the 147 kt = 1 columns hold anything
    live = torch.zeros(448, dtype=torch.bool)
    for c in range(3):
        live[(c * 3 + 1) * 49:(c * 3 + 2) * 49] = True
    assert bool((got[:, ~live.cuda()] == 0).all()) and bool((got[:, live.cuda()] != 0).any())
    paths = paths_of(clips)
    seen = {p for per_record in paths for p in per_record.values()}
    print(name, "staged blocks per record:", [sum(p.values()) for p in paths], "of", len(paths[0]))
    assert seen == want_paths
    if name == "s252_b2_t2":
        assert len({k for _, k in paths[0]}) == 2          # two chunks: 62 columns + 1
        assert all(not paths[0][(yo, 0)] and paths[0][(yo, 1)] for yo in range(1, 62))     # one block takes both paths


# ----------------------------------------------------------------------------------------- 2. T = 1 is the clip kernel ----
def test_single_frame_clips_give_the_clip_kernels_bytes(ops):
    from svit_amd.augment import AugClips
    from svit_amd.input import FramesView
    u8 = u8_video(1).cuda()
    clips = AugClips(u8, 64, [UPSCALE, erase(3, FLIP), erase(2, DOWNSCALE)], mean=MEAN, std=STD)
    for m in (None, _mix(1, 0.3), _mix(2, 0.75, (10, 42, 0, 32))):
        clips.mix = None if m is None else torch.from_numpy(m.pack()).cuda()
        got, _ = frames_cols(ops, FramesView(clips))
        want, _ = ops.im2col_patch_u8_aug(clips)
        assert torch.equal(bits(got), bits(want)), m


# ------------------------------------------------------------------------------------------ 3. noise keyed by the clip ----
def centre_frames(cols, N, S):
    """[N*Ho*Wo, 448] -> bf16 [N,3,S,S]: pixel (4*yo + i, 4*xo + j) is tap (kt 1, ky 3 + i, kx 3 + j) of row (yo, xo)"""
    Ho = S // 4
    v = cols[:, :441].reshape(N, Ho, Ho, 3, 3, 7, 7)[:, :, :, :, 1, 3:7, 3:7]      # [N,Ho,Wo,3,4,4]
    return v.permute(0, 3, 1, 4, 2, 5).reshape(N, 3, S, S)


def test_erase_noise_is_keyed_by_the_clip_not_by_the_frame_index(ops):
    from svit_amd.augment import AugClips
    from svit_amd.input import FramesView
    V, T, S = 3, 4, 64
    u8 = u8_video(T).cuda()
    recs = [erase(3, UPSCALE, seed=5), erase(3, FLIP, seed=6)]
    clips = AugClips(u8, S, recs, mean=MEAN, std=STD)
    got = centre_frames(frames_cols(ops, FramesView(clips))[0], len(recs) * T, S)
    want = as_frames(clips.render())[:, :, 0].to(torch.bfloat16)
    box = (slice(None), slice(None), slice(BOX[0], BOX[0] + BOX[2]), slice(BOX[1], BOX[1] + BOX[3]))
    assert torch.equal(bits(got[box].contiguous()), bits(want[box].contiguous()))
    assert torch.equal(bits(got), bits(want))
    # the "reshape the batch" shortcut: the same frames as V*T one-frame videos, one record per frame
    flat = AugClips(u8.view(V * T, 1, 96, 96, 3), S, [r._replace(video=r.video * T + t) for r in recs for t in range(T)],
                    mean=MEAN, std=STD)
    mutant = flat.render()[:, :, 0].to(torch.bfloat16)
    outside = torch.ones(S, S, dtype=torch.bool)
    outside[box[2], box[3]] = False
    assert torch.equal(bits(mutant[..., outside.cuda()]), bits(want[..., outside.cuda()]))     # the same geometry ...
    same = (mutant[box] == want[box]).float().mean(dim=(1, 2, 3))
    print("re-indexed records: share of equal box elements per frame", same.tolist())
    # ... other noise: counter (idx, clip, c*T + t) against (idx, frame, c) -- only clip 0's frame 0, channel 0 coincides
    assert float(same[0]) < 0.4 and bool((same[1:] < 0.01).all())


# ------------------------------------------------------------------------------------------------------ 4. the mix ----
MIXES = [_mix(1, 0.3), _mix(2, 0.75, (10, 42, 0, 32))]


@pytest.mark.parametrize("B", [2, 3])
def test_mix_equals_the_fp32_route(ops, B):
    from svit_amd.augment import AugClips
    from svit_amd.input import FramesView
    T, S = 3, 64
    u8 = u8_video(T).cuda()
    recs = [UPSCALE, erase(3, FLIP), erase(2, DOWNSCALE)][:B]
    clips = AugClips(u8, S, recs, mean=MEAN, std=STD)
    plain, _ = frames_cols(ops, FramesView(clips))
    render = clips.render()
    for m in MIXES:
        record = torch.from_numpy(m.pack()).cuda()
        clips.mix = record
        got, _ = frames_cols(ops, FramesView(clips))
        want, _ = ops.im2col_patch(as_frames(ops.mixup_clips(render.clone(), record)))
        assert torch.equal(bits(got), bits(want)), m
        assert not torch.equal(bits(got), bits(plain))
    clips.mix = torch.from_numpy(_mix(0, 1.0).pack()).cuda()
    assert torch.equal(bits(frames_cols(ops, FramesView(clips))[0]), bits(plain))


# ------------------------------------------------------------------------------------------------------ 5. U8Clips ----
def test_u8clips_view(ops):
    from svit_amd.augment import AugClips, AugRecord
    from svit_amd.input import FramesView, U8Clips
    V, T, S = 3, 4, 64
    u8 = u8_video(T).cuda()
    table = [(2, 3, 5), (0, 32, 31), (1, 0, 18)]
    clips = U8Clips(u8, S, torch.tensor(table, dtype=torch.int32), mean=MEAN, std=STD)
    view = FramesView(clips)
    assert tuple(view.shape) == (len(table) * T, 3, 1, S, S)
    got, thw = frames_cols(ops, view)
    per_frame = U8Clips(u8.view(V * T, 1, 96, 96, 3), S,
                        torch.tensor([(v * T + t, y0, x0) for v, y0, x0 in table for t in range(T)], dtype=torch.int32),
                        mean=MEAN, std=STD)
    want, thw_ref = ops.im2col_patch_u8(per_frame)
    assert thw == thw_ref and torch.equal(bits(got), bits(want))
    render = AugClips(u8, S, [AugRecord.identity(v, y0, x0, S) for v, y0, x0 in table], mean=MEAN, std=STD).render()
    for m in MIXES:
        record = torch.from_numpy(m.pack()).cuda()
        clips.mix = record
        mixed, _ = frames_cols(ops, FramesView(clips))
        ref, _ = ops.im2col_patch(as_frames(ops.mixup_clips(render.clone(), record)))
        assert torch.equal(bits(mixed), bits(ref)), m
        assert not torch.equal(bits(mixed), bits(got))


# ------------------------------------------------------------------------------------------------ 6. the whole step ----
@pytest.fixture(scope="module")
def net(ops):
    from svit_amd import losses
    cfg, model, spec, sd = SM.build_hip_model(4, 64)
    model.engine.reproducible = True
    cfg.SVIT.CONSISTENCY = "l2"
    loss_mod = losses.VideoImageLoss(cfg)

    def loss_fun(preds, extra, labels):
        parts = loss_mod(preds, extra, labels, {})
        assert "video_image_desc_l2_loss" in parts          # the loss depends on the frames output
        return loss_mod.total(parts)

    return model, loss_fun


TABLES = [
    [R(0, 3, 5, 64, 64, 64, 64), R(2, 6, 26, 64, 64, 64, 64)],
    [R(1, 10, 2, 80, 70, 64, 64, flip=1, mode=3, box=(8, 20, 30, 25), seed=5),
     R(0, 40, 50, 30, 41, 64, 64, mode=1, box=(0, 0, 20, 63))],
    [R(2, 0, 0, 96, 96, 110, 110, oy=17, ox=40),
     R(1, 0, 0, 96, 96, 70, 70, oy=6, ox=0, flip=1, mode=2, box=(30, 30, 30, 30), seed=9)],
]


def same_step(a, b, model, feed_a, feed_b, y, **kw):
    """replay both steps on their inputs: loss, preds and the flat gradient agree bit for bit -> the loss"""
    loss_a, (preds_a, _) = a([feed_a], y, **kw)
    torch.cuda.synchronize()
    loss_a, preds_a, grad_a = loss_a.clone(), preds_a.clone(), model.flat.grad.clone()
    loss_b, (preds_b, _) = b([feed_b], y, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(loss_a) and float(grad_a.abs().max()) > 0
    assert torch.equal(loss_a, loss_b) and torch.equal(preds_a, preds_b) and torch.equal(grad_a, model.flat.grad)
    return float(loss_a)


def test_step_from_augclips_equals_the_fp32_step(net):
    from svit_amd.augment import AugClips
    from svit_amd.graph import GraphedTrainStep
    model, loss_fun = net
    u8, y = u8_video(4).cuda(), P.labels(2).cuda()
    first = AugClips(u8, 64, TABLES[0])
    step = GraphedTrainStep(model, loss_fun, [first], y, frames_pass="u8")
    ref = GraphedTrainStep(model, loss_fun, [first.render()], y, frames_pass=True)
    assert step.n_graphs == ref.n_graphs
    seen = []
    for recs in TABLES:
        clips = AugClips(u8, 64, recs)
        seen.append(same_step(step, ref, model, clips, clips.render(), y))
    print("losses", seen)
    assert len(set(seen)) == 3                          # the records were read at replay time


def test_step_from_augclips_with_mixup_equals_the_fp32_step(net):
    from svit_amd import mixup
    from svit_amd.augment import AugClips
    from svit_amd.graph import GraphedTrainStep
    model, loss_fun = net
    fn = mixup.MixUp(0.8, 1.0, label_smoothing=0.1, num_classes=174)
    u8, y = u8_video(4).cuda(), P.labels(2).cuda()
    clips = AugClips(u8, 64, TABLES[1])
    step = GraphedTrainStep(model, loss_fun, [clips], y, frames_pass="u8", mixup=fn)
    ref = GraphedTrainStep(model, loss_fun, [clips.render()], y, frames_pass=True, mixup=fn)
    mixed = same_step(step, ref, model, clips, clips.render(), y, mix=mixup.MixRecord(1, 0.3, 0, 0, 0, 0))
    unmixed = same_step(step, ref, model, clips, clips.render(), y, mix=mixup.NO_MIX)
    assert mixed != unmixed


def test_step_from_u8clips_equals_the_fp32_step(net):
    from svit_amd.augment import AugClips, AugRecord
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.input import U8Clips
    model, loss_fun = net
    u8, y = u8_video(4).cuda(), P.labels(2).cuda()
    tables = [[(0, 3, 5), (2, 6, 26)], [(1, 32, 0), (1, 7, 19)]]

    def pair(table):
        clips = U8Clips(u8, 64, torch.tensor(table, dtype=torch.int32))
        return clips, AugClips(u8, 64, [AugRecord.identity(v, y0, x0, 64) for v, y0, x0 in table]).render()

    clips, clip32 = pair(tables[0])
    step = GraphedTrainStep(model, loss_fun, [clips], y, frames_pass="u8")
    ref = GraphedTrainStep(model, loss_fun, [clip32], y, frames_pass=True)
    seen = [same_step(step, ref, model, *pair(table), y) for table in tables]
    assert seen[0] != seen[1]                           # the crop table was read at replay time


# ----------------------------------------------------------------------------------------- 7. the chain once per step ----
def test_randaugment_chain_runs_once_per_step(net, monkeypatch):
    from svit_amd import randaug as ra
    from svit_amd.augment import AugClips
    from svit_amd.graph import GraphedTrainStep
    model, loss_fun = net
    u8, y = u8_video(4).cuda(), P.labels(2).cuda()
    table = [[ra.RandAugOp(ra.OP_INVERT), ra.RandAugOp(ra.OP_SOLARIZE, arg_i=100)],
             [ra.RandAugOp(ra.OP_POSTERIZE, arg_i=3), ra.RandAugOp(ra.OP_INVERT)],
             [ra.RandAugOp(ra.OP_SOLARIZE, arg_i=60), ra.RandAugOp(ra.OP_POSTERIZE, arg_i=5)]]
    clips = AugClips(u8, 64, TABLES[1], randaug=table)
    assert clips.ra_table.shape[1] == 2
    calls, real = [], ra.apply

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ra, "apply", counted)
    step = GraphedTrainStep(model, loss_fun, [clips], y, frames_pass="u8", warmup=1)
    assert len(calls) == 2                              # one per run of the body: the warm-up and the capture
    monkeypatch.setattr(ra, "apply", real)
    clip32 = clips.render()
    assert not torch.equal(clip32, AugClips(u8, 64, TABLES[1]).render())       # the chain does something
    ref = GraphedTrainStep(model, loss_fun, [clip32], y, frames_pass=True)
    same_step(step, ref, model, clips, clip32, y)


# ------------------------------------------------------------------------------------------------------ 8. refusals ----
def test_refusals(net):
    from svit_amd import hip
    from svit_amd.augment import AugClips
    from svit_amd.graph import GraphedTrainStep
    model, loss_fun = net
    u8, y = u8_video(4).cuda(), P.labels(2).cuda()
    clips = AugClips(u8, 64, TABLES[0])
    with pytest.raises(hip.SvitHipError, match='"u8"'):
        GraphedTrainStep(model, loss_fun, [clips], y, frames_pass=True)
    with pytest.raises(hip.SvitHipError):
        GraphedTrainStep(model, loss_fun, [clips.render()], y, frames_pass="u8")
