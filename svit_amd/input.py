"""Decoded uint8 frames as the model input.

The reference's loader normalises on the host and ships fp32 `[B,3,T,S,S]` clips
(slowfast/datasets/ssv2.py:297-327, datasets/utils.py:287-303, utils/misc.py:374-387).  `U8Clips`
keeps what the decoder produced -- uint8 `[V,T,Hs,Ws,3]` -- on the device and describes each
clip as (source video, y0, x0) + size; normalisation, the T H W C -> C T H W permute and the crop
(datasets/transform.py:288-348) happen inside the patch-embedding im2col
(`svit_im2col_patch_u8`).  `model([clips], meta)` accepts it wherever it accepts the fp32 tensor;
the numbers are bit-identical to feeding the reference-normalised fp32 crop.  `FramesView(clips)` is the
same clips (or an `augment.AugClips`) as B*T single frames: the input of the reference's frames pass.
"""
import torch

from . import hip


def normalize_lut_f32(mean, std, device):
    """f32 [3,256]: tensor_normalize (datasets/utils.py:287-303) of every uint8 value, with the reference's fp32
    operation order -- what the mixup route blends (`svit_im2col_patch_u8_mix`: normalise, mix in fp32, round once)."""
    t = torch.arange(256, dtype=torch.float32) / 255.0
    t = t[None, :] - torch.tensor(list(mean), dtype=torch.float32)[:, None]
    t = t / torch.tensor(list(std), dtype=torch.float32)[:, None]
    return t.contiguous().to(device)


def normalize_lut(mean, std, device):
    """bf16 [3,256]: the same table after the bf16 rounding the patch-embed operand gets."""
    return normalize_lut_f32(mean, std, "cpu").to(torch.bfloat16).to(device)


class U8Input:
    """uint8 frames [V,T,Hs,Ws,3] on the GPU + a table with one row per clip (`_rows` names it), standing in for the
    fp32 clip tensor [B,3,T,S,S]: the parts of the tensor interface the model path and GraphedTrainStep touch."""
    _rows = None

    def _take_frames(self, frames):
        if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3:
            raise ValueError("frames must be uint8 [V,T,H,W,3], got %s %s" % (frames.dtype, tuple(frames.shape)))
        if not frames.is_cuda:
            raise hip.SvitHipError("%s lives on the GPU (the host ships uint8, a quarter of the bytes)"
                                   % type(self).__name__)
        self.frames = frames.contiguous()
        return frames.shape[:4]

    @property
    def shape(self):
        return torch.Size((getattr(self, self._rows).shape[0], 3, self.frames.shape[1], self.size, self.size))

    @property
    def device(self):
        return self.frames.device

    def dim(self):
        return 5

    def detach(self):
        return self

    def contiguous(self):
        return self


class U8Clips(U8Input):
    """B clips cut from V uint8 videos.  Quacks like the fp32 clip tensor where the model and
    GraphedTrainStep look at it (`shape`, `dim()`, `device`, `detach/clone/contiguous/copy_`)."""
    _rows = "crops"

    def __init__(self, frames, size, crops=None, mean=(0.45, 0.45, 0.45), std=(0.225, 0.225, 0.225),
                 lut=None, lut_f32=None, extents=None):
        V, T, Hs, Ws = self._take_frames(frames)
        self.size = int(size)
        if self.size > Hs or self.size > Ws:
            raise ValueError("crop %d larger than the frames %dx%d" % (self.size, Hs, Ws))
        if crops is None:
            crops = torch.tensor([[v, 0, 0] for v in range(V)], dtype=torch.int32)
        crops = torch.as_tensor(crops, dtype=torch.int32)
        if crops.dim() != 2 or crops.shape[1] != 3:
            raise ValueError("crops must be int32 [B,3] = (video, y0, x0)")
        # range check wherever the table lives (one tiny reduction + one sync at construction; the
        # kernel additionally clamps, so a table rewritten later through copy_ cannot read outside)
        c = crops
        ok = ((c[:, 0] >= 0) & (c[:, 0] < V) & (c[:, 1] >= 0) & (c[:, 1] + self.size <= Hs) &
              (c[:, 2] >= 0) & (c[:, 2] + self.size <= Ws))
        if not bool(ok.all()):
            raise ValueError("crop table outside the frames")
        # extents (list of (h, w) or int [V,2]; augment.pack_videos): `frames` is a padded buffer and video v its
        # top-left h_v x w_v corner.  Checked here, on the host, row by row; the kernel neither reads nor needs them.
        self.extents = None
        if extents is not None:
            from .augment import pack_extents
            self.extents = pack_extents(extents, V, Hs, Ws)
            e = self.extents.to(c.device, torch.int64)[c[:, 0].to(torch.int64)]
            ok = (c[:, 1] + self.size <= e[:, 0]) & (c[:, 2] + self.size <= e[:, 1])
            if not bool(ok.all()):
                raise ValueError("crop %d reaches outside the extent of its video" % int((~ok).nonzero()[0, 0]))
        self.crops = crops.to(frames.device).contiguous()
        self.lut = normalize_lut(mean, std, frames.device) if lut is None else lut
        self.mean, self.std = tuple(mean), tuple(std)
        self._lut_f32 = lut_f32
        # cfg.MIXUP: the device mix record (svit_amd/mixup.py) -- set by MixUp.mix / GraphedTrainStep, routes
        # ops.im2col_patch_u8 to svit_im2col_patch_u8_mix; None = the plain kernel
        self.mix = None

    @property
    def lut_f32(self):
        """the fp32 table of the mixup route (built on first use; shared by clones)"""
        if self._lut_f32 is None:
            if self.lut is not None and not torch.equal(
                    self.lut, normalize_lut(self.mean, self.std, self.frames.device)):
                raise ValueError("U8Clips was given a bf16 table that is not normalize_lut(mean, std): "
                                 "pass the matching lut_f32 for the mixup route")
            self._lut_f32 = normalize_lut_f32(self.mean, self.std, self.frames.device)
        return self._lut_f32

    def data_ptr(self):
        return self.frames.data_ptr()

    def clone(self):
        return U8Clips(self.frames.clone(), self.size, self.crops.clone(), mean=self.mean, std=self.std,
                       lut=self.lut, lut_f32=self._lut_f32, extents=self.extents)

    def copy_(self, other, non_blocking=False):
        if self.frames.shape != other.frames.shape:
            raise ValueError("copy_ between U8Clips over buffers of different shapes: %s and %s"
                             % (tuple(self.frames.shape), tuple(other.frames.shape)))
        self.frames.copy_(other.frames, non_blocking=non_blocking)
        self.crops.copy_(other.crops, non_blocking=non_blocking)
        self.extents = other.extents            # (host side: what the crop table was checked against)
        return self

    def render(self):
        """fp32 [B,3,T,S,S]: the normalised crops as a clip tensor (no mix) -- the values whose bf16 rounding the im2col
        reads, and the coordinates of an input gradient (svit_amd/saliency.py); the identity records of the crop table
        through augment.AugClips.render"""
        from .augment import AugClips
        return AugClips(self.frames, self.size, identity_records(self.crops, self.size), mean=self.mean, std=self.std,
                        lut_f32=self.lut_f32).render()


def identity_records(crops, size):
    """int32 [B,3] crop table (video, y0, x0) -> the int32 [B,16] augmentation records of the same integer crops
    (`augment.AugRecord.identity` row by row: rectangle = window = size x size, nothing else), on the table's device:
    three small launches, so a captured step rebuilds them from the table it finds at replay time."""
    rec = torch.zeros((crops.shape[0], 16), dtype=torch.int32, device=crops.device)
    rec[:, 0:3] = crops
    rec[:, 3:7] = int(size)
    return rec


class FramesView(U8Input):
    """The B*T frames of a U8Clips or an augment.AugClips as single-frame clips -- the input of the reference's frames
    pass (tools/train_net.py:105-110: `inputs[0].transpose(1, 2).flatten(0, 1).unsqueeze(2)`) without the fp32 clip.
    Nothing is copied: the view reads the clips' `frames`, records (or crop table), `lut_f32` and `mix` when it is
    used, and `svit_im2col_patch_u8_aug_frames` evaluates frame n = b*T + t with clip b's record (and, under a mix, the
    partner clip's).  Quacks like the fp32 tensor [B*T,3,1,S,S] where the model path looks.
    fresh: the caller promises that `clips.frames` already holds this step's RandAugment output (the clip forward of
    the same step ran the chain), so `ops.im2col_patch_u8_aug_frames` does not run it again."""

    def __init__(self, clips, fresh=False):
        from .augment import AugClips
        if not isinstance(clips, (U8Clips, AugClips)):
            raise TypeError("FramesView takes a U8Clips or an AugClips, got %s" % type(clips).__name__)
        self.clips = clips
        self.fresh = bool(fresh)

    frames = property(lambda self: self.clips.frames)
    lut_f32 = property(lambda self: self.clips.lut_f32)
    mix = property(lambda self: self.clips.mix)
    size = property(lambda self: self.clips.size)
    # the device extents table of an AugClips (a U8Clips checks its crops on the host: its kernels take none)
    extents = property(lambda self: self.clips.extents if hasattr(self.clips, "records") else None)

    def device_records(self):
        """the int32 [B,16] records the kernel reads: the AugClips' own table, or the identity records of the crop table"""
        rec = getattr(self.clips, "records", None)
        return identity_records(self.clips.crops, self.clips.size) if rec is None else rec

    @property
    def shape(self):
        B, _, T, S, _ = self.clips.shape
        return torch.Size((B * T, 3, 1, S, S))


def spatial_crops_u8(frames, size, num_crops=3, **kw):
    """The test-time crops of every video as a crop TABLE over the shared uint8 frames (no copy):
    clip v*num_crops + j = crop j of video v (transform.uniform_crop offsets)."""
    from .evaluate import uniform_crop_offsets
    V, T, Hs, Ws, _ = frames.shape
    idx = [1] if num_crops == 1 else list(range(num_crops))
    table = [[v, *uniform_crop_offsets(Hs, Ws, size, s)] for v in range(V) for s in idx]
    return U8Clips(frames, size, torch.tensor(table, dtype=torch.int32), **kw)
