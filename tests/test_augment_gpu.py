"""Device-side augmentation of uint8 clips (svit_amd/augment.py; svit_im2col_patch_u8_aug, svit_u8_clips_render).

The value of an output pixel is a formula (include/svit_hip.h), so the yardstick is that formula in float64 over the
fp32 normalisation table, and the bar is worked out, not measured: per record
    tol = 6 * 2^-24 * max(h, w, out) * R + 4 * 2^-24 * M        (R = range of the table, M = its largest magnitude)
-- the first term bounds what fp32 rounding of the two source coordinates (quotient + one fma each, <= 2^-24 * in per
axis) moves a value that is Lipschitz with constant R per axis, the second the three lerps.  F.interpolate on the CPU and
the reference's own recorded outputs (tests/golden/augment.npz) carry their own fp32 error of the same kind, hence 2 * tol
against them."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import smoke_impl as SM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEAN, STD = [0.45, 0.40, 0.5], [0.225, 0.25, 0.2]
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import ops
    return ops


def R(video, i, j, h, w, out_h, out_w, oy=0, ox=0, flip=0, mode=0, box=(0, 0, 0, 0), seed=0):
    from svit_amd.augment import AugRecord
    return AugRecord(video, i, j, h, w, out_h, out_w, oy, ox, flip, mode, *box, seed)


# ------------------------------------------------------------------------------------------ the float64 formula ----
def _axis64(dst, n_in, n_out):
    scale = np.float64(n_in) / np.float64(n_out)
    src = np.maximum(scale * (dst + 0.5) - 0.5, 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = np.clip(src - i0, 0.0, 1.0)
    return i0, i1, 1.0 - l1, l1


def exact_clips(u8, lut, recs, S, offset=False):
    """float64 [B,3,T,S,S] of the resampling formula (no erasing): weights in float64, taps from the fp32 table.
    offset=True: a mutant WITHOUT the half-pixel offset (src = scale * dst), to show the bar tells the two apart."""
    V, T, Hs, Ws, _ = u8.shape
    lut64 = lut.double().numpy()
    out = np.zeros((len(recs), 3, T, S, S))
    for b, r in enumerate(recs):
        y, x = np.arange(S), np.arange(S)
        xs = S - 1 - x if r.flip else x
        if offset:
            def ax(dst, n_in, n_out):
                src = np.float64(n_in) / np.float64(n_out) * dst
                i0 = np.minimum(src.astype(np.int64), n_in - 1)
                return i0, i0 + (i0 < n_in - 1), 1.0 - np.clip(src - i0, 0, 1), np.clip(src - i0, 0, 1)
        else:
            ax = _axis64
        r0, r1, l0y, l1y = ax(r.oy + y, r.h, r.out_h)
        c0, c1, l0x, l1x = ax(r.ox + xs, r.w, r.out_w)
        fr = u8[r.video].numpy()                                      # [T,Hs,Ws,3]
        for c in range(3):
            t = lut64[c][fr[:, r.i:r.i + r.h, r.j:r.j + r.w, c]]      # [T,h,w]
            a, bb = t[:, r0][:, :, c0], t[:, r0][:, :, c1]
            cc, d = t[:, r1][:, :, c0], t[:, r1][:, :, c1]
            out[b, c] = l0y[None, :, None] * (l0x * a + l1x * bb) + l1y[None, :, None] * (l0x * cc + l1x * d)
    return torch.from_numpy(out)


def tolerances(lut, recs):
    """[B,1,1,1,1] float64"""
    rng = float((lut.max(1).values - lut.min(1).values).max())
    mag = float(lut.abs().max())
    t = [6 * EPS * max(r.h, r.w, r.out_h, r.out_w) * rng + 4 * EPS * mag for r in recs]
    return torch.tensor(t, dtype=torch.float64).view(-1, 1, 1, 1, 1)


def interpolate_clips(u8, lut, recs, S):
    """the reference's way on the CPU: normalise, F.interpolate the rectangle, cut the window, flip"""
    outs = []
    for r in recs:
        fr = u8[r.video].long()                                       # [T,Hs,Ws,3]
        norm = torch.stack([lut[c][fr[..., c]] for c in range(3)])   # [3,T,Hs,Ws] f32
        img = F.interpolate(norm[:, :, r.i:r.i + r.h, r.j:r.j + r.w], size=(r.out_h, r.out_w), mode="bilinear",
                            align_corners=False)
        win = img[:, :, r.oy:r.oy + S, r.ox:r.ox + S]
        outs.append(win.flip(-1) if r.flip else win)
    return torch.stack(outs)


def ref_im2col(clip, pad_value=0.0):
    """[B,3,T,S,S] -> [rows, 448] with the kernel's column order ((c*3 + kt)*7 + ky)*7 + kx; padding taps and the 7 pad
    columns hold `pad_value`"""
    x = F.pad(clip, (3, 3, 3, 3, 1, 1), value=pad_value)
    u = x.unfold(2, 3, 2).unfold(3, 7, 4).unfold(4, 7, 4)             # [B,3,To,Ho,Wo,kt,ky,kx]
    u = u.permute(0, 2, 3, 4, 1, 5, 6, 7).reshape(-1, 441)
    return F.pad(u, (0, 7), value=pad_value)


def aug_cols(clips):
    """svit_im2col_patch_u8_aug into a buffer pre-filled with bf16 NaNs: an element the kernel leaves out stays NaN"""
    from svit_amd import hip
    fr = clips.frames
    V, T, Hs, Ws, _ = fr.shape
    B, S = clips.records.shape[0], clips.size
    rows = B * ((T - 1) // 2 + 1) * ((S - 1) // 4 + 1) ** 2
    cols = torch.full((rows, 448), float("nan"), device=fr.device, dtype=torch.bfloat16)
    hip.call("svit_im2col_patch_u8_aug", fr.data_ptr(), fr.numel(), clips.lut_f32.data_ptr(), clips.records.data_ptr(),
             None if clips.mix is None else clips.mix.data_ptr(), cols.data_ptr(), B, T, Hs, Ws, S)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(cols).any()), "elements left out"
    return cols


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ------------------------------------------------------------------------------------------------- the cases ----
def small_records():
    S = 32
    return [
        R(0, 2, 3, 38, 50, S, S),                       # downscale; (j*3) & 3 = 1
        R(1, 5, 10, 12, 9, S, S, flip=1),               # upscale, flipped; (j*3) & 3 = 2
        R(2, 39, 0, 1, 56, S, S),                       # h = 1 (the last row of the last video)
        R(0, 0, 55, 40, 1, S, S),                       # w = 1 (the last column)
        R(2, 20, 26, 20, 30, S, S),                     # ends at the last byte of the last video
        R(1, 0, 0, 40, 56, 45, 63, oy=7, ox=20, flip=1),   # short-side jitter form: out != S, offsets, flip
        R(1, 3, 5, S, S, S, S),                         # identity
        R(0, 1, 7, 37, 41, 40, 33, oy=8, ox=1),         # rectangle + out != S + offsets; (j*3) & 3 = 1
    ]


def big_records():
    return [R(0, 10, 21, 280, 270, 256, 256),           # too wide for the LDS staging budget: the gather path
            R(0, 0, 0, 300, 300, 320, 320, oy=30, ox=64, flip=1)]


class Case:
    def __init__(self, ops, shape, S, recs, seed):
        from svit_amd.augment import AugClips
        g = torch.Generator().manual_seed(seed)
        self.u8 = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        self.S, self.recs = S, recs
        self.clips = AugClips(self.u8.cuda(), S, recs, mean=MEAN, std=STD)
        self.lut = self.clips.lut_f32.cpu()
        self.render = self.clips.render()
        torch.cuda.synchronize()
        self.cols = aug_cols(self.clips)
        self.exact = exact_clips(self.u8, self.lut, recs, S)
        self.tol = tolerances(self.lut, recs)


@pytest.fixture(scope="module")
def small(ops):
    return Case(ops, (3, 4, 40, 56, 3), 32, small_records(), 11)


@pytest.fixture(scope="module")
def big(ops):
    return Case(ops, (1, 2, 300, 300, 3), 256, big_records(), 12)


@pytest.fixture(scope="module", params=["small", "big"])
def case(request, small, big):
    return small if request.param == "small" else big


# ------------------------------------------------------------------------------------------- 1. the geometry ----
def test_render_within_the_worked_out_bar_of_the_float64_formula(case):
    assert tuple(case.render.shape) == (len(case.recs), 3, case.u8.shape[1], case.S, case.S)
    err = (case.render.cpu().double() - case.exact).abs()
    ratio = err / case.tol
    print("render vs float64 formula: max err / tol per record", ratio.flatten(1).max(1).values.tolist())
    assert bool((err <= case.tol).all())
    # the bar tells a wrong formula apart: without the half-pixel offset most resampled elements are outside
    mutant = exact_clips(case.u8, case.lut, case.recs, case.S, offset=True)
    resampled = [b for b, r in enumerate(case.recs) if (r.h, r.w) != (r.out_h, r.out_w) and r.h > 1 and r.w > 1]
    outside = ((case.render.cpu().double() - mutant).abs() > case.tol)[resampled].double().mean()
    print("mutant without the half-pixel offset: %.3f of the resampled elements outside" % float(outside))
    assert float(outside) > 0.9


def test_render_against_f_interpolate(case):
    ref = interpolate_clips(case.u8, case.lut, case.recs, case.S).double()
    own = (ref - case.exact).abs() / case.tol
    print("F.interpolate vs float64 formula: max err / tol", float(own.max()))
    assert bool(((case.render.cpu().double() - ref).abs() <= 2 * case.tol).all())


def test_im2col_operand_brackets_and_equals_im2col_of_render(ops, case):
    lo = (case.exact - case.tol).float().to(torch.bfloat16).float()
    hi = (case.exact + case.tol).float().to(torch.bfloat16).float()
    lo_c, hi_c = ref_im2col(lo), ref_im2col(hi)                 # padding taps and pad columns: 0 on both sides
    v = case.cols.cpu().float()
    assert v.shape == lo_c.shape
    assert bool(((v >= lo_c) & (v <= hi_c)).all())
    live = ref_im2col(torch.ones_like(lo)) != 0
    # every column a frame reaches is live: all 441 from three frames on (a 2-frame clip never fills the kt = 0 taps)
    T = case.u8.shape[1]
    kts = {kt for to in range((T - 1) // 2 + 1) for kt in range(3) if 0 <= 2 * to - 1 + kt < T}
    assert int(live[:, :441].any(0).sum()) == 147 * len(kts) and not bool(live[:, 441:].any())
    assert len(kts) == 3 or T < 3
    assert bool((v[~live] == 0).all())
    # the same function, one rounding: bit for bit the fp32 im2col of render()
    ref_cols, thw = ops.im2col_patch(case.render)
    own, thw2 = ops.im2col_patch_u8_aug(case.clips)
    torch.cuda.synchronize()
    assert thw == thw2
    assert torch.equal(bits(ref_cols), bits(case.cols)) and torch.equal(bits(own), bits(case.cols))


def test_reference_outputs_recorded_in_the_fixture(ops):
    """tests/golden/augment.npz: the reference's spatial_sampling (+ const erasing) on the closed-form clip"""
    from svit_amd.augment import AugClips
    gold = np.load(os.path.join(GOLDEN, "augment.npz"))
    shape, S = (2, 4, 40, 56, 3), int(gold["out_size"])
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    u8 = torch.from_numpy((((i * 131) % 251 + 3 * (i % 2)) % 256).astype(np.uint8).reshape(shape))
    keys = list(gold["out_keys"])
    recs = []
    for row in gold["out_meta"]:
        m = dict(zip(keys, (int(v) for v in row)))
        recs.append(R(m["video"], m["i"], m["j"], m["h"], m["w"], m["out_h"], m["out_w"], m["oy"], m["ox"], m["flip"],
                      1 if m["erased"] else 0, (m["et"], m["el"], m["eh"], m["ew"])))
    assert any(r.flip for r in recs) and any(r.erase_mode for r in recs) and any(r.out_h != S for r in recs)
    assert any((r.h, r.w) != (40, 56) for r in recs)
    clips = AugClips(u8.cuda(), S, recs, mean=[float(v) for v in gold["mean"]], std=[float(v) for v in gold["std"]])
    got = clips.render().cpu().double()
    tol = tolerances(clips.lut_f32.cpu(), recs)
    ref = torch.from_numpy(gold["out_clips"]).double()
    print("render vs the reference's outputs: max err / tol", float(((got - ref).abs() / tol).max()))
    assert bool(((got - ref).abs() <= 2 * tol).all())
    for b, r in enumerate(recs):
        if r.erase_mode:
            assert bool((got[b, :, :, r.et:r.et + r.eh, r.el:r.el + r.ew] == 0).all())


# ------------------------------------------------------------------------- 2. identity geometry = the plain kernels ----
def _mix(mode, lam, box=(0, 0, 0, 0)):
    from svit_amd.mixup import MixRecord
    return MixRecord(mode, lam, *box)


@pytest.mark.parametrize("shape,S,table", [
    ((3, 4, 40, 56, 3), 32, [(0, 3, 5), (2, 8, 24), (1, 0, 7)]),                   # odd B
    ((3, 4, 40, 56, 3), 32, [(0, 3, 5), (1, 0, 21), (2, 6, 0), (1, 6, 18)]),
    ((1, 2, 300, 300, 3), 256, [(0, 0, 0), (0, 44, 43)]),                          # two chunks per row
    ((1, 3, 41, 59, 3), 37, [(0, 4, 22), (0, 1, 0)]),       # 21771 bytes = 3 mod 4, clip 0 ends on the last byte
])
def test_identity_geometry_is_bit_equal_to_the_plain_u8_kernels(ops, shape, S, table):
    from svit_amd.augment import AugClips
    from svit_amd.input import U8Clips
    g = torch.Generator().manual_seed(S + len(table))
    u8 = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda()
    Hs, Ws = shape[2], shape[3]
    plain = U8Clips(u8, S, torch.tensor(table, dtype=torch.int32), mean=MEAN, std=STD)
    # both identity forms: the rectangle IS the crop; the whole frame "resampled" to its own size + the crop as offset
    forms = [[R(v, y, x, S, S, S, S) for v, y, x in table],
             [R(v, 0, 0, Hs, Ws, Hs, Ws, oy=y, ox=x) for v, y, x in table]]
    mixes = [None, _mix(0, 1.0), _mix(1, 0.3), _mix(1, 0.8125), _mix(2, 0.5, (5, 20, 3, 29)), _mix(2, 0.5, (0, S, 0, S)),
             _mix(2, 1.0, (7, 7, 1, 9))]
    for recs in forms:
        clips = AugClips(u8, S, recs, mean=MEAN, std=STD)
        for m in mixes:
            plain.mix = clips.mix = None if m is None else torch.from_numpy(m.pack()).cuda()
            want, _ = ops.im2col_patch_u8(plain)
            got = aug_cols(clips)
            assert torch.equal(bits(got), bits(want)), (recs[0], m)


# ------------------------------------------------------------------------------------------------ 3. erasing ----
BOX = (4, 6, 10, 12)            # top, left, height, width


def _erased(small, mode, box=BOX, seed=77):
    from svit_amd.augment import AugClips
    recs = [r._replace(erase_mode=mode, et=box[0], el=box[1], eh=box[2], ew=box[3], seed=seed + b)
            for b, r in enumerate(small.recs)]
    clips = AugClips(small.clips.frames, small.S, recs, mean=MEAN, std=STD)
    render = clips.render()
    torch.cuda.synchronize()
    return clips, render, aug_cols(clips)


def _inside(S, box=BOX):
    m = torch.zeros(S, S, dtype=torch.bool)
    m[box[0]:box[0] + box[2], box[1]:box[1] + box[3]] = True
    return m


def _clip_index_cols(B, T, S):
    """for every element of cols the flat index of the clip element it copies (-1: padding)"""
    idx = torch.arange(B * 3 * T * S * S, dtype=torch.float64).view(B, 3, T, S, S)
    return ref_im2col(idx, pad_value=-1.0).long()


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_erasing(ops, small, mode):
    S, T, B = small.S, small.u8.shape[1], len(small.recs)
    clips, render, cols = _erased(small, mode)
    inside = _inside(S)
    r, base = render.cpu(), small.render.cpu()
    # outside the box nothing moves; the operand is still the one rounding of render()
    assert torch.equal(bits(r[..., ~inside]), bits(base[..., ~inside]))
    assert torch.equal(bits(ops.im2col_patch(render)[0]), bits(cols))
    idx = _clip_index_cols(B, T, S)
    in_cols = (idx >= 0) & inside.flatten()[idx.clamp(min=0) % (S * S)]
    c, c0 = cols.cpu(), small.cols.cpu()
    assert torch.equal(bits(c)[~in_cols], bits(c0)[~in_cols])
    box = r[..., inside].view(B, 3, T, BOX[2], BOX[3])
    if mode == 1:
        assert bool((box == 0).all()) and bool((c.float()[in_cols] == 0).all())
        return
    assert bool(torch.isfinite(box).all()) and float(box.abs().max()) < 6.0
    if mode == 2:
        assert bool((box == box[..., :1, :1]).all())                   # one value per (clip, channel, frame)
        v = box[..., 0, 0]
        assert len(torch.unique(v)) == v.numel()                       # ... and another for every frame, channel, clip
        return
    assert len(torch.unique(box)) > 0.99 * box.numel()                 # one value per element
    # every im2col copy of a pixel holds the same bf16 value: scatter cols back to the clip, min == max per element
    flat_idx, vals = idx[in_cols], bits(c)[in_cols].long()
    n = B * 3 * T * S * S
    lo = torch.full((n,), 1 << 20).scatter_reduce(0, flat_idx, vals, "amin")
    hi = torch.full((n,), -(1 << 20)).scatter_reduce(0, flat_idx, vals, "amax")
    seen = hi > -(1 << 20)
    assert int(seen.sum()) == B * 3 * T * BOX[2] * BOX[3] and bool((lo[seen] == hi[seen]).all())
    # the same seed gives the same values, another seed others
    _, again, cols_again = _erased(small, mode)
    assert torch.equal(bits(again), bits(render)) and torch.equal(bits(cols_again), bits(cols))
    _, other, _ = _erased(small, mode, seed=78)
    assert not bool((other.cpu()[..., inside] == r[..., inside]).any(-1).all())
    assert torch.equal(bits(other.cpu()[..., ~inside]), bits(base[..., ~inside]))


def test_empty_box_and_mode_0_change_nothing(small):
    for mode, box in ((3, (4, 6, 0, 12)), (2, (4, 6, 10, 0)), (1, (32, 32, 0, 0)), (0, BOX)):
        _, render, cols = _erased(small, mode, box)
        assert torch.equal(bits(render), bits(small.render)) and torch.equal(bits(cols), bits(small.cols)), (mode, box)


def test_pixel_noise_is_standard_normal(ops):
    """a 16 x 96 x 96 box (x 3 channels = 4.4e5 samples): |mean| < 0.01 and |var - 1| < 0.02, about 6 sigma of the two
    estimators (sigma_mean = 1.5e-3, sigma_var = 2.1e-3); the bf16 rounding is not in render()"""
    from svit_amd.augment import AugClips
    u8 = torch.zeros((1, 16, 96, 96, 3), dtype=torch.uint8).cuda()
    clips = AugClips(u8, 96, [R(0, 0, 0, 96, 96, 96, 96, mode=3, box=(0, 0, 96, 96), seed=20240229)])
    z = clips.render().double().flatten()
    assert z.numel() == 3 * 16 * 96 * 96
    mean, var = float(z.mean()), float(z.var())
    print("pixel noise: mean %.5f var %.5f max |z| %.3f" % (mean, var, float(z.abs().max())))
    assert abs(mean) < 0.01 and abs(var - 1.0) < 0.02
    # and over the channels / frames separately it is not one pattern repeated
    planes = z.view(3 * 16, -1)
    assert float(torch.corrcoef(planes).fill_diagonal_(0).abs().max()) < 0.05


# ------------------------------------------------------------------------------------------------- 4. bounds ----
def test_out_of_range_records_are_clamped_on_the_device(ops, small):
    """a table rewritten on the device (no host check) runs and gives what the clamped table gives, on a frames buffer of
    exactly V*T*Hs*Ws*3 bytes"""
    from svit_amd import augment
    from svit_amd.augment import AugClips
    V, T, Hs, Ws, _ = small.u8.shape
    S = small.S
    big, lo, hi = 10 ** 6, -2 ** 31, 2 ** 31 - 1
    bad = [
        R(99, 1000, -7, 0, -3, 0, 2 ** 30, -4, big, 7, 9, (-3, -3, big, big), -1),
        R(-5, -1, 1000, big, big, big, 0, big, -4, -1, 3, (big, big, big, big), 5),
        R(hi, hi, hi, hi, hi, hi, hi, hi, hi, hi, hi, (hi, hi, hi, hi), hi),
        R(lo, lo, lo, lo, lo, lo, lo, lo, lo, lo, lo, (lo, lo, lo, lo), lo),
        R(1, 30, 50, 20, 20, 16, 16, 3, 3, 0, 3, (28, 28, 10, 10), 9),       # window larger than the resampled image
        R(2, 39, 55, 5, 5, S, S, 0, 0, 1, 2, (0, 0, S, S), 4),
    ]
    table = augment.pack_records(bad)
    frames = small.u8.cuda()
    assert frames.numel() == V * T * Hs * Ws * 3
    clips = AugClips(frames, S, [small.recs[0]] * len(bad), mean=MEAN, std=STD)
    clips.records.copy_(table.cuda())                                   # rewritten on the device: no host check
    clamped = AugClips(frames, S, [small.recs[0]] * len(bad), mean=MEAN, std=STD)
    clamped.set_records(augment.clamp_records(table, V, Hs, Ws, S), validate=False)
    a, b = clips.render(), clamped.render()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(bits(a), bits(b))
    assert torch.equal(bits(aug_cols(clips)), bits(aug_cols(clamped)))
    with pytest.raises(ValueError):
        AugClips(frames, S, bad[:1], mean=MEAN, std=STD)                # the host check refuses the same table
    with pytest.raises(ValueError):
        clips.set_records(bad)


# ---------------------------------------------------------------------------------------------- 5. the model ----
def _u8_video():
    video = P.frames(3, 4, 96)                                   # [V,3,T,96,96], |x| <= 1.7 -> bytes in [17, 212]
    return ((video * 0.225 + 0.45) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()


def test_graph_replay_reads_the_records_at_replay_time():
    """one capture with mixup, one without; three record tables (the third replayed under a mixup record): loss and flat
    gradient of every replay are bit-equal to the eager step on the same records (reproducible weight gradients, drop
    rates 0: both run the same kernels on the same operands)"""
    from svit_amd import losses, mixup
    from svit_amd.augment import AugClips
    from svit_amd.graph import GraphedTrainStep
    cfg, model, spec, sd = SM.build_hip_model(4, 64)
    model.engine.reproducible = True
    fn = mixup.MixUp(0.8, 1.0, label_smoothing=0.1, num_classes=174)
    u8 = _u8_video().cuda()
    y = P.labels(2).cuda()
    S = 64
    tables = [
        [R(0, 3, 5, 64, 64, S, S), R(2, 6, 26, 64, 64, S, S)],
        [R(1, 10, 2, 80, 70, S, S, flip=1, mode=3, box=(8, 20, 30, 25), seed=5), R(0, 40, 50, 30, 41, S, S, mode=1, box=(0, 0, 20, 63))],
        [R(2, 0, 0, 96, 96, 110, 110, oy=17, ox=40), R(1, 0, 0, 96, 96, 70, 70, oy=6, ox=0, flip=1, mode=2, box=(30, 30, 30, 30), seed=9)],
    ]
    mixes = [mixup.NO_MIX, mixup.NO_MIX, mixup.MixRecord(1, 0.3, 0, 0, 0, 0), mixup.MixRecord(2, 0.75, 10, 42, 0, 32)]

    def loss_fun(preds, extra, labels):
        return losses.cross_entropy(preds, labels)

    def eager(clips, rec):
        clips = clips.clone()
        labels = y
        if rec is not None:
            _, labels = fn.mix(clips, y, record=rec)
        model.flat.grad.zero_()
        logits, _ = model([clips], {})
        loss = losses.cross_entropy(logits, labels)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), model.flat.grad.clone()

    first = AugClips(u8, S, tables[0])
    step = GraphedTrainStep(model, loss_fun, [first], y, mixup=fn)
    plain = GraphedTrainStep(model, loss_fun, [first], y)
    assert step.n_graphs == plain.n_graphs
    seen = []
    for recs, m in zip(tables + [tables[2]], mixes):
        clips = AugClips(u8, S, recs)
        want_loss, want_grad = eager(clips, m)
        loss, _ = step([clips], y, mix=m)
        torch.cuda.synchronize()
        assert torch.equal(loss, want_loss) and torch.equal(model.flat.grad, want_grad), (recs, m)
        seen.append(float(loss))
        if m.mode == 0:
            want_loss, want_grad = eager(clips, None)
            loss, _ = plain([clips], y)
            torch.cuda.synchronize()
            assert torch.equal(loss, want_loss) and torch.equal(model.flat.grad, want_grad), recs
    assert len(set(seen)) == len(seen)                  # the records (and the mix) were read at replay time
    assert first.mix is None                            # the caller's clips are not tagged: the step's copy is
    # the fp32 route on render() is the same step: the operand is bit-equal (test_im2col_operand...), so is the result
    clips = AugClips(u8, S, tables[1])
    model.flat.grad.zero_()
    logits, _ = model([clips.render()], {})
    loss = losses.cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    want_loss, want_grad = eager(clips, None)
    assert torch.equal(loss.detach(), want_loss) and torch.equal(model.flat.grad, want_grad)
    with pytest.raises(Exception):
        GraphedTrainStep(model, loss_fun, [first], y, frames_pass=True)
