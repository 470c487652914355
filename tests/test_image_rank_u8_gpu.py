"""The image-rank step on uint8 stills (augment.AugClips with T = 1, per-still extents, RandAugment tables; boxes and HAOG
targets from augment.draw_still).

The tiny configuration of test_image_rank_step_parity_vs_oracle: a 4-frame model, S = 64, 3 stills.  The stills lie in a
20 x 24 buffer (two 256-pixel blocks) as 20x24, 12x16 and 3x3 (the smallest RandAugment takes); the padding around them
alternates 0 and 255, so a kernel that reads it gives other bytes.  Every value comparison is bit equality: the operand
from the stills and `svit_im2col_patch` of the rendered fp32 stills perform the same fp32 operations and one bf16
rounding, and with `engine.reproducible` the step behind equal operands is the same launches on the same bytes."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import smoke_impl as SM
from tests.test_augment_gpu import bits
from tests.test_ragged_gpu import outside_mask, padded, tight_videos

S, HS, WS = 64, 20, 24
SIZES = [(20, 24), (12, 16), (3, 3)]
AA, INTERP = "rand-m7-n4-mstd0.5-inc1", "random"
PARTS = ("boxes_l1_loss", "boxes_bce_loss", "boxes_giou_loss", "loss_contact_state")
SHEAR_BAR = 1.5         # px: 1 for the half-level crossing of a resampled edge + 0.5 for the pixel-centre convention
#                         measured on MI355X: 0.480 px over the 16 cases (and the same on the host arithmetic)


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import ops
    return ops


def still_boxes(h, w):
    """float32 [1,4,4] xyxy in the still's pixels: two hands / objects, an absent row, one near the lower left corner"""
    return np.array([[[0.20 * w, 0.25 * h, 0.70 * w, 0.80 * h], [0.50 * w, 0.10 * h, 0.95 * w, 0.60 * h],
                      [0, 0, 0, 0], [0.05 * w, 0.50 * h, 0.40 * w, 0.95 * h]]], dtype=np.float32)


def draw_batch(sizes, seed):
    """stills of `sizes` in the 20 x 24 buffer + what augment.draw_still draws for each at its OWN size
    -> (frames u8 [V,1,20,24,3] host, extents, tight stills, records, RandAugment table, meta tree on the host)"""
    from svit_amd import randaug
    from svit_amd.augment import SpatialSampler, draw_still, pack_videos
    vids = tight_videos(sizes, T=1, lo=17, span=196)
    packed, ext = pack_videos([torch.from_numpy(v) for v in vids], Hs=HS, Ws=WS)
    frames = torch.from_numpy(padded(vids, HS, WS))
    out = torch.from_numpy(np.broadcast_to(outside_mask(sizes, HS, WS), tuple(frames.shape)).copy())
    assert torch.equal(torch.where(out, torch.zeros_like(frames), frames), packed) and bool((frames[out] == 255).any())
    random.seed(seed)
    np.random.seed(seed)
    ra = randaug.RandAugSampler(AA, INTERP)
    sampler = SpatialSampler(S, scale=(0.5, 1.0), aspect=(0.75, 1.3333), re_prob=1.0, re_mode="pixel")
    drawn = [draw_still(ra, sampler, h, w, still_boxes(h, w), video=v) for v, (h, w) in enumerate(ext.tolist())]
    contact = torch.roll(P.haog_meta(len(sizes))["contact_state"], seed, 0)
    meta = {"haog_bboxes": torch.stack([t for _, _, t in drawn]), "contact_state": contact}
    assert tuple(meta["haog_bboxes"].shape) == (len(sizes), 1, 4, 4)
    return frames, ext, vids, [r for _, r, _ in drawn], [o for o, _, _ in drawn], meta


def clips_of(batch):
    from svit_amd.augment import AugClips
    frames, ext, _, recs, table, _ = batch
    return AugClips(frames.cuda(), S, recs, randaug=table, extents=ext)


def on_device(meta):
    return {k: v.cuda() for k, v in meta.items()}


# ------------------------------------------------------------------------------------------------ 1. the stills route ----
def test_stills_are_read_through_their_own_extent(ops):
    from svit_amd.augment import AugClips
    batch = draw_batch(SIZES, 1)
    frames, ext, vids, recs, table, meta = batch
    assert any(o.op for layers in table for o in layers) and all(r.erase_mode == 3 for r in recs)
    clips = clips_of(batch)
    assert tuple(clips.shape) == (3, 3, 1, S, S)
    cols, thw = ops.im2col_patch_u8_aug(clips)
    render = clips.render()
    torch.cuda.synchronize()
    assert thw == (1, 16, 16) and tuple(cols.shape) == (3 * 256, 448)
    cols = cols.view(3, 256, 448)
    for b, rec in enumerate(recs):
        # the tight still alone, its record at row b (the erase noise is keyed by the clip's row)
        alone = AugClips(torch.from_numpy(vids[b][None]).cuda(), S, [rec._replace(video=0)] * len(recs), randaug=[table[b]])
        want = ops.im2col_patch_u8_aug(alone)[0].view(3, 256, 448)[b]
        assert torch.equal(bits(cols[b]), bits(want)), (b, rec)
        assert torch.equal(bits(render[b]), bits(alone.render()[b])), (b, rec)
    # and the operand is the fp32 route's: one rounding of the rendered values
    assert torch.equal(bits(cols.view(-1, 448)), bits(ops.im2col_patch(render)[0]))
    # the targets follow the records: a flipped still has mirrored centres
    t = meta["haog_bboxes"]
    assert float(t.min()) >= 0 and float(t.max()) <= 1 and not t[:, 0, 2].any() and bool(t[:, 0, :2].any())


# ------------------------------------------------------------------- 2. the Shear boxes follow the Shear pixels ----
def test_shear_boxes_enclose_the_sheared_pixels(ops):
    """No recorded truth exists for the Shear boxes (svit_amd/randaug.py): they are held to the pixels instead.  A 255
    rectangle on 0 through `randaug.apply`; the bounding box of the bright pixels against `boxes_layer`.  The affine
    fill is 128, so "bright" is > 128 rather than > 127: on a 0 -> 255 edge the half-level crossing moves by 1/255 px."""
    from svit_amd import randaug
    H, W = 40, 48
    x0, y0, x1, y1 = 14, 12, 30, 26
    img = np.zeros((1, 1, H, W, 3), dtype=np.uint8)
    img[:, :, y0:y1, x0:x1] = 255
    box = np.array([[[x0, y0, x1, y1], [0, 0, 0, 0]]], dtype=np.float32)
    cases = [(name, f, filt) for name in ("ShearX", "ShearY") for f in (0.21, -0.21, 0.3, -0.09) for filt in (0, 1)]
    src = torch.from_numpy(np.repeat(img, len(cases), axis=0)).cuda()
    table = torch.from_numpy(randaug.pack_table([[randaug.make_op(n, (f,), (filt,), H, W)] for n, f, filt in cases])).cuda()
    dst = torch.empty_like(src)
    ws = torch.zeros(randaug.workspace_bytes(len(cases), 1), dtype=torch.uint8, device="cuda")
    randaug.apply(src, table, dst, None, ws)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.array_equal(out, randaug.apply_host(img.repeat(len(cases), 0), table.cpu().numpy()))
    worst = 0.0
    for c, (name, f, filt) in enumerate(cases):
        bright = out[c, 0, :, :, 0] > 128
        ys, xs = np.nonzero(bright.any(1))[0], np.nonzero(bright.any(0))[0]
        seen = np.array([xs[0], ys[0], xs[-1] + 1, ys[-1] + 1], dtype=np.float64)
        moved = randaug.boxes_layer(name, (f,), box, H, W)
        assert not moved[0, 1].any()
        dev = float(np.abs(seen - moved[0, 0]).max())
        worst = max(worst, dev)
        assert dev <= SHEAR_BAR, (name, f, filt, seen, moved[0, 0])
        assert float(np.abs(moved[0, 0] - box[0, 0]).max()) > 1                  # the shear moved the box
    print("Shear boxes against the pixels: max deviation %.3f px (bar %.1f)" % (worst, SHEAR_BAR))


# ----------------------------------------------------------------------------------------------------- 3. the step ----
@pytest.fixture(scope="module")
def net(ops):
    from svit_amd import losses
    cfg, model, spec, sd = SM.build_hip_model(4, 64)
    model.engine.reproducible = True
    return cfg, model, losses.VideoImageLoss(cfg, is_video_rank=False)


def eager_step(model, fn, x, meta):
    model.flat.grad.zero_()
    logits, extra = model([x], meta)
    parts = fn(logits, extra, None, meta)
    loss = fn.total(parts)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: parts[k].detach().clone() for k in PARTS}, model.flat.grad.clone()


def test_step_from_stills_equals_the_fp32_step(net):
    cfg, model, fn = net
    seen = []
    for sizes, seed in ((SIZES, 1), ([(12, 16), (20, 24), (7, 9)], 2)):
        batch = draw_batch(sizes, seed)
        clips, meta = clips_of(batch), on_device(batch[5])
        got = eager_step(model, fn, clips, meta)
        want = eager_step(model, fn, clips.render(), meta)
        assert torch.isfinite(got[0]) and float(got[2].abs().max()) > 0
        assert torch.equal(got[0], want[0]), (float(got[0]), float(want[0]))
        for k in PARTS:
            assert torch.equal(got[1][k], want[1][k]), k
        assert float(got[1]["boxes_l1_loss"]) > 0
        assert torch.equal(got[2], want[2]), int((got[2] != want[2]).sum())
        seen.append(float(got[0]))
    assert seen[0] != seen[1]


def test_one_captured_step_serves_every_draw():
    """GraphedTrainStep(..., optimizer=guarded) captured on one draw and replayed on two further ones (other sizes,
    tables, records, targets, contact states) against the eager step + guarded optimizer on a twin model: loss, gradient,
    weights and both moments agree bit for bit after every step"""
    from svit_amd import losses, optim
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.hip import SvitHipError
    cfg, ma, _, _ = SM.build_hip_model(4, 64)
    _, mb, _, _ = SM.build_hip_model(4, 64)
    ma.engine.reproducible = mb.engine.reproducible = True
    fn = losses.VideoImageLoss(cfg, is_video_rank=False)

    def loss_fun(preds, extra, labels):
        return fn.total(fn(preds, extra, None, labels))

    a = optim.GuardedClipAdamW(ma, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    b = optim.GuardedClipAdamW(mb, lr=1e-3, weight_decay=0.05, clip_grad_l2norm=1.0)
    first = draw_batch(SIZES, 1)
    step = GraphedTrainStep(ma, loss_fun, [clips_of(first)], on_device(first[5]), optimizer=a)
    torch.cuda.synchronize()
    assert torch.equal(ma.flat.data, mb.flat.data) and a.stats()["applied"] == 0
    seen = []
    for sizes, seed in (([(12, 16), (20, 24), (7, 9)], 2), ([(3, 3), (20, 19), (16, 24)], 3)):
        batch = draw_batch(sizes, seed)
        clips, meta = clips_of(batch), on_device(batch[5])
        loss, _ = step([clips], meta)
        torch.cuda.synchronize()
        want = eager_step(mb, fn, clips_of(batch), meta)
        b.step()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and torch.equal(loss, want[0]), (sizes, float(loss), float(want[0]))
        assert torch.equal(ma.flat.grad, mb.flat.grad), sizes
        for name, x, y in (("weights", ma.flat.data, mb.flat.data), ("exp_avg", a.exp_avg, b.exp_avg),
                           ("exp_avg_sq", a.exp_avg_sq, b.exp_avg_sq)):
            assert torch.equal(x, y), (sizes, name, int((x != y).sum()))
        seen.append(float(loss))
    assert seen[0] != seen[1] and a.stats()["applied"] == 2
    other = draw_batch(SIZES, 4)
    with pytest.raises(SvitHipError, match="captured for a frame buffer"):
        step([AugClipsOver(other, 28)], on_device(other[5]))


def AugClipsOver(batch, Ws):
    """the same batch in a wider buffer"""
    from svit_amd.augment import AugClips
    frames, ext, _, recs, table, _ = batch
    wide = torch.zeros((frames.shape[0], 1, HS, Ws, 3), dtype=torch.uint8)
    wide[:, :, :, :WS] = frames
    return AugClips(wide.cuda(), S, recs, randaug=table, extents=ext)
