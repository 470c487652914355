"""Device-side training augmentation for uint8 clips: random-resized crop / scale jitter + crop, flip, random erasing.

The reference's loader normalises the decoded frames and then, per clip and on the host in fp32, runs
`utils.spatial_sampling` (slowfast/datasets/utils.py:110-192: `random_resized_crop` or `random_short_side_scale_jitter` +
`random_crop`, `horizontal_flip`; test time: the short-side rescale + `uniform_crop`; datasets/transform.py:47-105,154-191,
248-348,596-683) and `RandomErasing` (datasets/random_erasing.py, called from ssv2.py:345-426).  Here the frames stay uint8
`[V,T,Hs,Ws,3]` in device memory, as with `input.U8Clips`; what was drawn for a clip is a 64-byte RECORD (`AugRecord`,
`struct SvitAug` of include/svit_hip.h) in device memory next to them, and the patch-embedding im2col evaluates the whole
pipeline per output pixel while it assembles its operand (`svit_im2col_patch_u8_aug`): bilinear taps from the fp32
normalisation table, one bf16 rounding.  Every kernel reads the records at run time, so one captured `GraphedTrainStep`
serves every draw -- a step only rewrites B x 64 bytes (and the frames).

    sampler = build_sampler(cfg, "train")                       # cfg.DATA.* and, where the yaml brings it, cfg.AUG.*
    records = [sampler.draw(Hs, Ws, video=v) for v in range(B)] # host: Python's `random` / `np.random`, reference order
    clips = AugClips(frames_u8, cfg.DATA.TRAIN_CROP_SIZE, records, cfg.DATA.MEAN, cfg.DATA.STD)
    model([clips], meta)          # or GraphedTrainStep(model, loss, [clips], labels[, mixup=...])
    clips.render()                # the same values unrounded, fp32 [B,3,T,S,S]

The draws.  `SpatialSampler.draw` consumes the two global streams exactly as the reference does for the same cfg, so after
the same `random.seed` / `np.random.seed` it returns the reference's numbers: `_get_param_spatial_crop` (per try
`random.uniform` for the area, `random.uniform` for the log aspect, one `np.random.uniform` the reference draws for its
unused `switch_hw`; on success two `random.randint`; after 10 failures the central fallback), or the jitter size from
`np.random.uniform` (its reciprocal form with INV_UNIFORM_SAMPLE) and the crop offsets from `np.random.randint` (y then x,
each only where the rescaled side exceeds the crop); then `np.random.uniform` for the flip when DATA.RANDOM_FLIP; then
`RandomErasing._erase_cube`: `random.random` against RE_PROB, up to 100 tries of two `random.uniform` and, on a fit, two
`random.randint`.  ONE draw is added that the reference does not make: when a box was found and RE_MODE is `rand` or
`pixel`, the record's noise seed comes last from `random.getrandbits(31)` (the reference draws the noise itself from
torch's generator; here it is Philox keyed by that seed -- as random, not the same numbers).  At test time the reference
still draws the (degenerate) jitter size from `np.random.uniform`, and so does `draw`.

Where the reference itself fails, `draw` raises or does the evident thing: a rescaled frame that is already crop x crop
makes the reference's `random_crop` return a bare tensor that `spatial_sampling` cannot unpack -- here the offsets are 0
and nothing is drawn; a rescaled side SHORTER than the crop (a crop of the wrong size there) raises.

RandAugment (cfg.AUG.AA_TYPE, the stage BEFORE this pipeline) runs on the device as well: `AugClips(..., randaug=table)`
with the table of svit_amd/randaug.py keeps the raw frames and runs the chain raw -> `frames` ahead of every read.

Videos of different sizes in one batch (Something-Something v2 is distributed at a fixed height and a width that varies
from video to video; the reference augments each clip alone at its own size and batches only after the crop): the buffer
is padded to a common `[V,T,Hs,Ws,3]` and a table `extents` int32 [V,2] = (h_v, w_v) in device memory says where each
video lies -- rows [0, h_v), columns [0, w_v) of each of its frames, row pitch Ws.  Draw every clip for its OWN size:

    frames, extents = pack_videos(videos)                       # host u8 [T,h_v,w_v,3] each -> padded buffer + table
    table = pack_table([ra.draw(T, h, w, video=v) for v, (h, w) in enumerate(extents.tolist())])
    records = [sampler.draw(h, w, video=v) for v, (h, w) in enumerate(extents.tolist())]
    clips = AugClips(frames.cuda(), size, records, mean, std, randaug=table, extents=extents)

Every clip then gets the bytes it would get if its video had been augmented alone: RandAugment treats the extent as the
whole image and the records are validated (host) and clamped (device) against their own video, never the padding.  The
kernels read the table at run time, so one captured step serves any mix of sizes up to the captured (Hs, Ws).
`extents=None` is every video filling the buffer: the launches and bytes of before.

Image ranks (IMAGE_TRAIN.GPU_IDS; the reference's `Ssv2_frames`, ssv2_frames.py:296-362,373-452): a still is a clip with
T = 1 and runs the same pixel pipeline, and its hand / object boxes move with the pixels.  The boxes stay on the host --
16 floats per still, NumPy in the reference too -- and follow the draws: `ra.draw(1, h, w, boxes=b)` (svit_amd/randaug.py),
`sampler.draw(h, w, boxes=b)` (`boxes_through`: the reference's float32 arithmetic for `random_resized_crop`, the scale
jitter + `random_crop` / `uniform_crop`, `horizontal_flip`; erasing leaves boxes alone) and `haog_targets(b, S)` (divide by
S, clip to [0, 1], cxcywh, rows no larger than 0.05 zeroed).  `draw_still` does the three in the reference's order:

    stills, extents = pack_videos([img[None] for img in images])            # host u8 [1,h,w,3] each
    drawn = [draw_still(ra, sampler, h, w, boxes[v], video=v) for v, (h, w) in enumerate(extents.tolist())]
    clips = AugClips(stills.cuda(), size, [r for _, r, _ in drawn], mean, std, randaug=pack_table([o for o, _, _ in drawn]),
                     extents=extents)
    meta = {"haog_bboxes": torch.stack([t for _, _, t in drawn]).cuda(), "contact_state": contact.cuda()}
    model([clips], meta)          # or GraphedTrainStep(model, haog_loss, [clips], meta[, optimizer=...])

One captured step serves every draw: a replay uploads stills, records, tables and extents through `AugClips.copy_` and
the targets / contact states through the label tree.  The Shear boxes are geometric, not the reference's (randaug.py).

Out of scope: tightly packed storage with per-video offsets on the device (feeder.py packs tightly for the upload and
unpacks into this padded layout), per-frame sizes inside one video, colour jitter
(AUG.COLOR_JITTER, which the reference's loader never reads), DATA.TRAIN_JITTER_MOTION_SHIFT, the dataset class of the
image ranks (JSON parsing, `match_haog`, JPEG decoding), mixup on image ranks, AUG.RE_COUNT > 1 and bicubic
resampling.  The reference's frames pass reads the same frames and
records: `input.FramesView(clips)` is the B*T frames as single-frame clips (`svit_im2col_patch_u8_aug_frames`; frame
(b, t) through clip b's record, erase noise and mix partner included) and `GraphedTrainStep(..., frames_pass="u8")` runs
it inside the replayed step; `frames_pass=True` stays the fp32 route and refuses an `AugClips`.
"""
import collections
import math
import random

import numpy as np
import torch

from .input import U8Input, normalize_lut_f32

ERASE_NONE, ERASE_CONST, ERASE_RAND, ERASE_PIXEL = 0, 1, 2, 3
ERASE_MODES = {"": ERASE_CONST, "const": ERASE_CONST, "rand": ERASE_RAND, "pixel": ERASE_PIXEL}
FIELDS = "video i j h w out_h out_w oy ox flip erase_mode et el eh ew seed"
MAX_OUT = 1 << 24           # (AUG_MAX_OUT of csrc/input.hip: resampled sizes stay exact in fp32)


class AugRecord(collections.namedtuple("AugRecord", FIELDS)):
    """One clip's draw, the 16 int32 words of `struct SvitAug` in order (include/svit_hip.h): source video; source
    rectangle (i, j, h, w); the size (out_h, out_w) it is resampled to; the offset (oy, ox) of the S x S window in that
    image; flip; erase mode (0 none, 1 const, 2 rand, 3 pixel), erase box (et, el, eh, ew) in output coordinates; seed."""
    __slots__ = ()

    def pack(self):
        return np.array(self, dtype=np.int32)

    @classmethod
    def unpack(cls, words):
        return cls(*(int(w) for w in np.asarray(words).reshape(16)))

    @classmethod
    def identity(cls, video, y0, x0, size):
        """the integer crop (video, y0, x0) of a U8Clips row: in == out, weights exactly 1 and 0"""
        return cls(video, y0, x0, size, size, size, size, 0, 0, 0, 0, 0, 0, 0, 0, 0)


def pack_records(records):
    """list of AugRecord (or an int [B,16] array / tensor) -> int32 [B,16] tensor on the host"""
    if torch.is_tensor(records):
        t = records.to(torch.int32)
    elif isinstance(records, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(records.astype(np.int32)))
    else:
        t = torch.from_numpy(np.stack([AugRecord(*r).pack() for r in records]))
    if t.dim() != 2 or t.shape[1] != 16:
        raise ValueError("the record table is int32 [B,16], got %s" % (tuple(t.shape),))
    return t.contiguous()


def unpack_records(table):
    return [AugRecord.unpack(row) for row in table.detach().cpu().numpy()]


def pack_extents(extents, V, Hs, Ws, min_side=1):
    """list of (h, w) or an int [V,2] array / tensor -> int32 [V,2] tensor on the host; ValueError for an extent above
    the Hs x Ws buffer or below min_side (3 under RandAugment)"""
    from .randaug import pack_extents as pack
    return torch.from_numpy(pack(extents, V, Hs, Ws, min_side))


def clamp_extents(extents, Hs, Ws):
    """What the kernels make of ANY int32 [V,2] table: every extent clamped into [1,Hs] x [1,Ws] (int64 NumPy [V,2])"""
    e = np.array(torch.as_tensor(extents).detach().cpu().numpy(), dtype=np.int64).reshape(-1, 2)
    return np.stack([np.clip(e[:, 0], 1, Hs), np.clip(e[:, 1], 1, Ws)], axis=1)


def validate_records(table, V, Hs, Ws, S, extents=None):
    """ValueError unless every row describes a rectangle inside the frame, a window inside the resampled image and a
    box inside the window (the device additionally clamps: `clamp_records`).  extents (int [V,2], validated): the
    rectangle must lie inside the record's own video, not merely the buffer."""
    t = table.to(torch.int64)
    f = {n: t[:, k] for k, n in enumerate(FIELDS.split())}
    where, hv, wv = "%dx%d frame" % (Hs, Ws), Hs, Ws
    if extents is not None:
        e = torch.as_tensor(extents).to(t.device, torch.int64)[f["video"].clamp(0, V - 1)]
        where, hv, wv = "extent of its video", e[:, 0], e[:, 1]
    checks = (
        ("video outside [0, %d)" % V, (f["video"] >= 0) & (f["video"] < V)),
        ("source rectangle outside the %s" % where,
         (f["h"] >= 1) & (f["w"] >= 1) & (f["i"] >= 0) & (f["j"] >= 0) & (f["i"] + f["h"] <= hv) & (f["j"] + f["w"] <= wv)),
        ("resampled size outside [1, 2^24]",
         (f["out_h"] >= 1) & (f["out_w"] >= 1) & (f["out_h"] <= MAX_OUT) & (f["out_w"] <= MAX_OUT)),
        ("%dx%d window outside the resampled image" % (S, S),
         (f["oy"] >= 0) & (f["ox"] >= 0) & (f["oy"] + S <= f["out_h"]) & (f["ox"] + S <= f["out_w"])),
        ("erase mode outside 0..3", (f["erase_mode"] >= 0) & (f["erase_mode"] <= 3)),
        ("erase box outside the window",
         (f["et"] >= 0) & (f["el"] >= 0) & (f["eh"] >= 0) & (f["ew"] >= 0) & (f["et"] + f["eh"] <= S) & (f["el"] + f["ew"] <= S)),
    )
    for what, ok in checks:
        if not bool(ok.all()):
            raise ValueError("augmentation record %d: %s" % (int((~ok).nonzero()[0, 0]), what))


def clamp_records(table, V, Hs, Ws, S, extents=None):
    """What the kernels make of ANY int32 [B,16] table (aug_geom of csrc/input.hip) -- a valid table is unchanged except
    that flip becomes 0 / 1.  extents: ANY int [V,2] table; the rectangle is clamped into the (clamped) extent of the
    record's (clamped) video."""
    t = np.array(torch.as_tensor(table).detach().cpu().numpy(), dtype=np.int64).reshape(-1, 16)
    f = {n: t[:, k].copy() for k, n in enumerate(FIELDS.split())}
    f["video"] = np.clip(f["video"], 0, V - 1)
    if extents is not None:
        e = clamp_extents(extents, Hs, Ws)[f["video"]]
        Hs, Ws = e[:, 0], e[:, 1]
    f["h"], f["w"] = np.clip(f["h"], 1, Hs), np.clip(f["w"], 1, Ws)
    f["i"], f["j"] = np.clip(f["i"], 0, Hs - f["h"]), np.clip(f["j"], 0, Ws - f["w"])
    f["out_h"], f["out_w"] = np.clip(f["out_h"], 1, MAX_OUT), np.clip(f["out_w"], 1, MAX_OUT)
    f["oy"] = np.clip(f["oy"], 0, np.maximum(f["out_h"] - S, 0))
    f["ox"] = np.clip(f["ox"], 0, np.maximum(f["out_w"] - S, 0))
    f["flip"] = (f["flip"] != 0).astype(np.int64)
    f["erase_mode"] = np.where((f["erase_mode"] >= 1) & (f["erase_mode"] <= 3), f["erase_mode"], 0)
    f["et"], f["el"] = np.clip(f["et"], 0, S), np.clip(f["el"], 0, S)
    f["eh"], f["ew"] = np.clip(f["eh"], 0, S - f["et"]), np.clip(f["ew"], 0, S - f["el"])
    return torch.from_numpy(np.stack([f[n] for n in FIELDS.split()], axis=1).astype(np.int32))


def pack_videos(videos, Hs=None, Ws=None, out=None, pin_memory=False):
    """Videos of different sizes -> one padded batch.  videos: a list of V host u8 [T,h_v,w_v,3] tensors (one T).
    -> (frames u8 [V,T,Hs,Ws,3] on the host, zero outside each video; extents int32 [V,2] = (h_v, w_v)).  Hs / Ws default
    to the batch maxima; give the captured step's so that every batch has its buffer shape (a larger video raises).
    out: a buffer of that shape to reuse (e.g. a pinned one from an earlier call); pin_memory: allocate a pinned one."""
    if len(videos) == 0:
        raise ValueError("pack_videos needs at least one video")
    for v, x in enumerate(videos):
        if not torch.is_tensor(x) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3 or x.is_cuda:
            raise ValueError("video %d: expected a host uint8 [T,h,w,3] tensor" % v)
        if x.shape[0] != videos[0].shape[0]:
            raise ValueError("video %d has %d frames, video 0 has %d" % (v, x.shape[0], videos[0].shape[0]))
        if x.shape[1] < 1 or x.shape[2] < 1:
            raise ValueError("video %d is empty: %s" % (v, tuple(x.shape)))
    Hs = max(x.shape[1] for x in videos) if Hs is None else int(Hs)
    Ws = max(x.shape[2] for x in videos) if Ws is None else int(Ws)
    for v, x in enumerate(videos):
        if x.shape[1] > Hs or x.shape[2] > Ws:
            raise ValueError("video %d is %dx%d, larger than the %dx%d buffer" % (v, x.shape[1], x.shape[2], Hs, Ws))
    shape = (len(videos), videos[0].shape[0], Hs, Ws, 3)
    if out is None:
        out = torch.zeros(shape, dtype=torch.uint8, pin_memory=bool(pin_memory))
    else:
        if out.dtype != torch.uint8 or tuple(out.shape) != shape or out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous host uint8 %s tensor, got %s %s" % (shape, out.dtype, tuple(out.shape)))
        out.zero_()
    for v, x in enumerate(videos):
        out[v, :, :x.shape[1], :x.shape[2]] = x
    return out, torch.tensor([[x.shape[1], x.shape[2]] for x in videos], dtype=torch.int32)


class AugClips(U8Input):
    """B augmented clips over V uint8 videos: `frames` u8 [V,T,Hs,Ws,3] on the GPU, `size` = S, `records` a list of
    AugRecord (or an int32 [B,16] table).  Quacks like `input.U8Clips` where the model and GraphedTrainStep look at it;
    `mix` (the device mix record of svit_amd/mixup.py) is set by MixUp.mix / GraphedTrainStep.
    randaug: the int32 [V,N,16] table of svit_amd/randaug.py (`pack_table`) -- the object then keeps the frames it was
    given as `raw` (never written), the table in device memory and one scratch buffer, and `frames` becomes the chain's
    output: ops.im2col_patch_u8_aug / ops.u8_clips_render launch the 2N kernels raw -> frames first, eager and inside a
    captured step alike.  None: the same launches and bytes as ever.
    extents: a list of (h, w) or an int [V,2] table -- `frames` is a padded buffer and video v its top-left h_v x w_v
    corner (module docstring; `pack_videos`).  The table lives in device memory next to the records and every kernel of
    the route reads it (`svit_*_ext`); records are checked against their own video.  None: every video fills the
    buffer, the same launches and bytes as ever."""

    _rows = "records"

    def __init__(self, frames, size, records, mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225), lut_f32=None,
                 randaug=None, extents=None):
        V, T, Hs, Ws = self._take_frames(frames)
        self.size = int(size)
        if self.size < 1:
            raise ValueError("size must be positive")
        self._min_side = 1 if randaug is None else 3           # (RandAugment: the Hs, Ws >= 3 rule, per video)
        ext = None if extents is None else pack_extents(extents, V, Hs, Ws, self._min_side)
        table = pack_records(records)
        validate_records(table, V, Hs, Ws, self.size, ext)     # one tiny reduction + sync; the kernels also clamp
        self.records = table.to(frames.device)
        self.extents = None if ext is None else ext.to(frames.device)
        self.mean, self.std = tuple(mean), tuple(std)
        # the fp32 table is built here, outside any capture
        self.lut_f32 = normalize_lut_f32(mean, std, frames.device) if lut_f32 is None else lut_f32
        self.mix = None
        self.raw = self.ra_table = self.ra_tmp = self.ra_ws = None
        if randaug is not None:
            from . import randaug as ra
            table = self._pack_randaug(randaug)
            self.raw, self.frames = self.frames, torch.empty_like(self.frames)
            self.ra_table = table.to(frames.device)
            self.ra_tmp = torch.empty_like(self.frames) if table.shape[1] > 1 else None
            self.ra_ws = torch.empty(ra.workspace_bytes(V, T), dtype=torch.uint8, device=frames.device)

    def _pack_randaug(self, table):
        from . import randaug as ra
        t = table.to(torch.int32).contiguous() if torch.is_tensor(table) else torch.from_numpy(ra.pack_table(table))
        if t.dim() != 3 or t.shape[0] != self.frames.shape[0] or t.shape[1] < 1 or t.shape[2] != 16:
            raise ValueError("the RandAugment table is int32 [%d,N,16], got %s" % (self.frames.shape[0], tuple(t.shape)))
        return t

    def run_randaug(self):
        """raw -> frames through the table's N layers (2N launches on the current stream); nothing without a table"""
        if self.ra_table is not None:
            from . import randaug as ra
            ra.apply(self.raw, self.ra_table, self.frames, self.ra_tmp, self.ra_ws, extents=self.extents)

    def data_ptr(self):
        return (self.frames if self.raw is None else self.raw).data_ptr()

    def clone(self):
        ext = None if self.extents is None else self.extents.clone()
        if self.raw is not None:
            return AugClips(self.raw.clone(), self.size, self.records.clone(), mean=self.mean, std=self.std,
                            lut_f32=self.lut_f32, randaug=self.ra_table.clone(), extents=ext)
        return AugClips(self.frames.clone(), self.size, self.records.clone(), mean=self.mean, std=self.std,
                        lut_f32=self.lut_f32, extents=ext)

    def copy_(self, other, non_blocking=False):
        if (self.raw is None) != (other.raw is None) or (self.raw is not None and self.ra_table.shape != other.ra_table.shape):
            raise ValueError("copy_ between AugClips with and without RandAugment, or with tables of different shapes")
        if (self.extents is None) != (other.extents is None):
            raise ValueError("copy_ between AugClips with and without extents")
        if self.frames.shape != other.frames.shape:
            raise ValueError("copy_ between AugClips over buffers of different shapes: %s and %s"
                             % (tuple(self.frames.shape), tuple(other.frames.shape)))
        if self.extents is not None:
            self.extents.copy_(other.extents, non_blocking=non_blocking)
        if self.raw is not None:
            self.raw.copy_(other.raw, non_blocking=non_blocking)
            self.ra_table.copy_(other.ra_table, non_blocking=non_blocking)
        else:
            self.frames.copy_(other.frames, non_blocking=non_blocking)
        self.records.copy_(other.records, non_blocking=non_blocking)
        return self

    def set_randaug(self, table):
        """rewrite the RandAugment table in place (same [V,N,16]; the kernels clamp whatever it holds)"""
        if self.raw is None:
            raise ValueError("this AugClips was built without RandAugment")
        t = self._pack_randaug(table)
        if t.shape != self.ra_table.shape:
            raise ValueError("the RandAugment table is int32 %s, got %s" % (tuple(self.ra_table.shape), tuple(t.shape)))
        self.ra_table.copy_(t, non_blocking=True)
        return self

    def set_extents(self, extents, validate=True):
        """rewrite the extents table in place (same V) -- BEFORE set_records, which checks against the table it finds;
        validate=False skips the host check (the kernels clamp into the buffer)"""
        if self.extents is None:
            raise ValueError("this AugClips was built without extents")
        V, _, Hs, Ws, _ = self.frames.shape
        if validate:
            ext = pack_extents(extents, V, Hs, Ws, self._min_side)
        else:
            ext = torch.as_tensor(extents).to(torch.int32).reshape(V, 2).contiguous()
        self.extents.copy_(ext, non_blocking=True)
        return self

    def set_records(self, records, validate=True):
        """rewrite the record table in place (same B); validate=False skips the host check (the kernels clamp)"""
        table = pack_records(records)
        if table.shape != self.records.shape:
            raise ValueError("the record table is int32 %s, got %s" % (tuple(self.records.shape), tuple(table.shape)))
        if validate:
            V, _, Hs, Ws, _ = self.frames.shape
            validate_records(table, V, Hs, Ws, self.size, self.extents)
        self.records.copy_(table, non_blocking=True)
        return self

    def render(self):
        """fp32 [B,3,T,S,S]: the values the im2col rounds, unrounded (svit_u8_clips_render; no mix)"""
        from . import ops
        return ops.u8_clips_render(self)


class SpatialSampler:
    """The reference's random spatial pipeline for one clip as an AugRecord.  mode "train" / "val" / "test" as the
    reference's dataset (ssv2.py:252-292): AUG applies in "train" only."""

    def __init__(self, crop_size, jitter_scales=(256, 320), scale=None, aspect=None, random_flip=True,
                 inverse_uniform_sampling=False, re_prob=0.0, re_mode="const", re_count=1, spatial_sampling="random",
                 min_area=0.02, max_area=1 / 3, min_aspect=0.3):
        if (scale is None) != (aspect is None):
            raise ValueError("TRAIN_JITTER_SCALES_RELATIVE and TRAIN_JITTER_ASPECT_RELATIVE come together")
        if re_count not in (None, 0, 1):
            raise NotImplementedError("AUG.RE_COUNT > 1 (several erase boxes per clip) is not supported")
        if str(re_mode).lower() not in ERASE_MODES:
            raise ValueError("AUG.RE_MODE %r" % (re_mode,))
        if spatial_sampling not in ("random", "uniform"):
            raise ValueError(spatial_sampling)
        self.size = int(crop_size)
        self.min_scale, self.max_scale = jitter_scales
        self.scale = None if scale is None else tuple(scale)
        self.aspect = None if aspect is None else tuple(aspect)
        self.random_flip = bool(random_flip)
        self.inverse = bool(inverse_uniform_sampling)
        self.re_prob = float(re_prob)
        self.re_mode = ERASE_MODES[str(re_mode).lower()]
        self.min_area, self.max_area = min_area, max_area
        self.log_aspect = (math.log(min_aspect), math.log(1 / min_aspect))
        self.uniform = spatial_sampling == "uniform"
        # what the last draw() went through (tests pin the rare branches on these)
        self.trace = {}

    # ---- transform._get_param_spatial_crop ---------------------------------------------------
    def _resized_crop(self, height, width):
        scale, ratio = self.scale, self.aspect
        for n in range(10):
            target_area = random.uniform(*scale) * (height * width)
            aspect_ratio = math.exp(random.uniform(math.log(ratio[0]), math.log(ratio[1])))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            np.random.uniform()             # the reference's `np.random.uniform() < 0.5 and switch_hw` (switch_hw False)
            if 0 < w <= width and 0 < h <= height:
                i = random.randint(0, height - h)
                j = random.randint(0, width - w)
                self.trace.update(tries=n + 1, fallback=False)
                return i, j, h, w
        in_ratio = float(width) / float(height)
        if in_ratio < min(ratio):
            w = width
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = height
            w = int(round(h * max(ratio)))
        else:
            w, h = width, height
        self.trace.update(tries=10, fallback=True)
        return (height - h) // 2, (width - w) // 2, h, w

    # ---- transform.random_short_side_scale_jitter: the rescaled size ------------------------
    def _jitter(self, height, width, min_size, max_size, inverse):
        if inverse:
            size = int(round(1.0 / np.random.uniform(1.0 / max_size, 1.0 / min_size)))
        else:
            size = int(round(np.random.uniform(min_size, max_size)))
        if (width <= height and width == size) or (height <= width and height == size):
            self.trace.update(jitter_size=size, jitter_identity=True)
            return height, width
        new_h = new_w = size
        if width < height:
            new_h = int(math.floor((float(height) / width) * size))
        else:
            new_w = int(math.floor((float(width) / height) * size))
        self.trace.update(jitter_size=size, jitter_identity=False)
        return new_h, new_w

    def _check_covers(self, new_h, new_w):
        if new_h < self.size or new_w < self.size:
            raise ValueError("the rescaled frame %dx%d is smaller than the %d crop" % (new_h, new_w, self.size))

    def _erase(self):
        """RandomErasing._erase_cube on a [T,3,S,S] clip, count 1 -> (top, left, h, w) or None"""
        if random.random() > self.re_prob:
            return None
        area = self.size * self.size
        for n in range(100):
            target_area = random.uniform(self.min_area, self.max_area) * area / 1
            aspect_ratio = math.exp(random.uniform(*self.log_aspect))
            h = int(round(math.sqrt(target_area * aspect_ratio)))
            w = int(round(math.sqrt(target_area / aspect_ratio)))
            if w < self.size and h < self.size:
                top = random.randint(0, self.size - h)
                left = random.randint(0, self.size - w)
                self.trace.update(erase_tries=n + 1)
                return top, left, h, w
        self.trace.update(erase_tries=100)
        return None

    def draw(self, Hs, Ws, video=0, spatial_idx=1, boxes=None):
        """One clip's record for a Hs x Ws source.  spatial_idx: the test-time crop (0, 1, 2), "uniform" sampling only.
        boxes: float32 [..., 4] xyxy in source pixels -> (record, boxes_out) with the boxes in the S x S window's pixels
        (`boxes_through`; the draws are the same with and without them, erasing does not touch boxes)."""
        rec = self._draw(Hs, Ws, video, spatial_idx)
        if boxes is None:
            return rec
        return rec, boxes_through(rec, boxes, self.size, resized_crop=not self.uniform and self.scale is not None)

    def _draw(self, Hs, Ws, video, spatial_idx):
        S = self.size
        self.trace = {}
        if self.uniform:
            if spatial_idx not in (0, 1, 2):
                raise ValueError("spatial_idx must be 0, 1 or 2")
            new_h, new_w = self._jitter(Hs, Ws, S, S, False)          # (the reference draws the degenerate size too)
            self._check_covers(new_h, new_w)
            oy, ox = int(math.ceil((new_h - S) / 2)), int(math.ceil((new_w - S) / 2))
            if new_h > new_w:
                oy = 0 if spatial_idx == 0 else new_h - S if spatial_idx == 2 else oy
            else:
                ox = 0 if spatial_idx == 0 else new_w - S if spatial_idx == 2 else ox
            return AugRecord(video, 0, 0, Hs, Ws, new_h, new_w, oy, ox, 0, 0, 0, 0, 0, 0, 0)
        if self.scale is None:
            new_h, new_w = self._jitter(Hs, Ws, self.min_scale, self.max_scale, self.inverse)
            self._check_covers(new_h, new_w)
            oy = ox = 0
            if new_h == S and new_w == S:
                self.trace.update(crop_skipped=True)
            else:
                if new_h > S:
                    oy = int(np.random.randint(0, new_h - S))
                if new_w > S:
                    ox = int(np.random.randint(0, new_w - S))
            geom = (0, 0, Hs, Ws, new_h, new_w, oy, ox)
        else:
            geom = self._resized_crop(Hs, Ws) + (S, S, 0, 0)
        flip = int(np.random.uniform() < 0.5) if self.random_flip else 0
        mode, box, seed = ERASE_NONE, (0, 0, 0, 0), 0
        if self.re_prob > 0:
            found = self._erase()
            if found is not None:
                mode, box = self.re_mode, found
                if mode in (ERASE_RAND, ERASE_PIXEL):
                    seed = random.getrandbits(31)       # the ONE draw the reference does not make (module docstring)
        return AugRecord(video, *geom, flip, mode, *box, seed)


def boxes_through(rec, boxes, S, resized_crop):
    """The boxes of a clip through its record, in the reference's float32 arithmetic (datasets/transform.py): boxes
    float32 [..., 4] xyxy in source pixels -> the same shape in the S x S window's pixels.
    resized_crop: `random_resized_crop` -- shift by (j, i), clip to [0, w] / [0, h], scale by S / w, S / h.  Otherwise
    `random_short_side_scale_jitter` (ONE factor for both axes, none on its early return) and `crop_clip_boxes` with the
    window's offsets (`random_crop`, `uniform_crop`).  Then `horizontal_flip`: S - boxes[:, [2, 0]] - 1."""
    from .randaug import as_boxes
    src = as_boxes(boxes)
    b = src.reshape(-1, 4)
    out = b.copy()
    if resized_crop:
        out[:, [0, 2]] = np.clip(b[:, [0, 2]] - rec.j, 0, rec.w) * float(S) / rec.w
        out[:, [1, 3]] = np.clip(b[:, [1, 3]] - rec.i, 0, rec.h) * float(S) / rec.h
    else:
        if (rec.out_h, rec.out_w) != (rec.h, rec.w):
            b = b * float(rec.out_h) / rec.h if rec.w < rec.h else b * float(rec.out_w) / rec.w
        out[:, [0, 2]] = np.clip(b[:, [0, 2]] - rec.ox, 0, S)
        out[:, [1, 3]] = np.clip(b[:, [1, 3]] - rec.oy, 0, S)
    if rec.flip:
        out[:, [0, 2]] = S - out[:, [2, 0]] - 1
    return out.reshape(src.shape)


def haog_targets(boxes, S):
    """The HAOG box targets of ssv2_frames.py:347-353: boxes float32 [T,O,4] xyxy in the S x S window's pixels -> float32
    tensor [T,O,4] cxcywh in [0, 1]; a box no wider or no higher than 0.05 (an absent or cropped-away object) is a zero
    row (`box_ops.zero_empty_boxes`)."""
    from .randaug import as_boxes
    b = as_boxes(boxes)
    b = np.clip(b / int(S), 0, 1)
    x0, y0, x1, y1 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    out = np.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], axis=-1)
    if bool((out[..., 2:] < 0).any()):
        raise ValueError("a box with x1 < x0 or y1 < y0 (the reference asserts on it as well)")
    out[(out[..., 2:] <= 0.05).any(axis=-1)] = 0
    return torch.from_numpy(out)


def draw_still(randaug, sampler, Hs, Ws, boxes, video=0, spatial_idx=1):
    """One still of an image rank in the reference's order (ssv2_frames.py:373-452: RandAugment BEFORE the spatial draw,
    erasing last): boxes float32 [1,O,4] xyxy in the still's pixels -> (ops, record, target).  ops: the N RandAugOp of
    `randaug.draw` (None without a RandAugSampler: AUG off, val / test); record: the AugRecord; target: `haog_targets`
    of the boxes moved through both stages, float32 [1,O,4]."""
    ops = None
    if randaug is not None:
        ops, boxes = randaug.draw(1, Hs, Ws, video=video, boxes=boxes)
    rec, boxes = sampler.draw(Hs, Ws, video=video, spatial_idx=spatial_idx, boxes=boxes)
    return ops, rec, haog_targets(boxes, sampler.size)


def build_sampler(cfg, mode="train"):
    """SpatialSampler from cfg.DATA.* and cfg.AUG.* as the reference's dataset reads them (ssv2.py:95-100,252-292,377-422).
    AUG is not a key of this build's default tree (the reference's yaml brings it): absent = the reference's defaults,
    ENABLE False."""
    if mode not in ("train", "val", "test"):
        raise ValueError("mode %r" % (mode,))
    d = cfg.DATA
    if mode == "test":
        return SpatialSampler(d.TEST_CROP_SIZE, spatial_sampling="uniform", random_flip=False)
    a = getattr(cfg, "AUG", None)
    aug = mode == "train" and a is not None and bool(getattr(a, "ENABLE", False))
    scale = aspect = None
    re_prob, re_mode, re_count = 0.0, "const", 1
    if aug:
        if getattr(d, "TRAIN_JITTER_MOTION_SHIFT", False):
            raise NotImplementedError("DATA.TRAIN_JITTER_MOTION_SHIFT is not supported")
        scl, asp = list(d.TRAIN_JITTER_SCALES_RELATIVE), list(d.TRAIN_JITTER_ASPECT_RELATIVE)
        scale, aspect = (scl or None), (asp or None)
        re_prob = float(getattr(a, "RE_PROB", 0.25))
        re_mode, re_count = getattr(a, "RE_MODE", "pixel"), getattr(a, "RE_COUNT", 1)
    return SpatialSampler(d.TRAIN_CROP_SIZE, jitter_scales=tuple(d.TRAIN_JITTER_SCALES), scale=scale, aspect=aspect,
                          random_flip=d.RANDOM_FLIP, inverse_uniform_sampling=d.INV_UNIFORM_SAMPLE, re_prob=re_prob,
                          re_mode=re_mode, re_count=re_count)
