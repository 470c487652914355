"""The host side of the frames pass from uint8 clips (svit_im2col_patch_u8_aug_frames, input.FramesView): the entry point's
argument checks, which all happen before any launch, and the tensor logic that needs no GPU."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "svit_im2col_patch_u8_aug_frames"
OK, ERR_SHAPE, ERR_ALIGN, ERR_ARG = 0, -2, -3, -4


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    return hip.load()


def test_symbol_is_exported_declared_and_bound():
    from svit_amd import hip
    assert NAME in hip.EXPORTS
    header = open(os.path.join(ROOT, "include", "svit_hip.h")).read()
    assert re.search(r"\bint %s\(const uint8_t\* frames, int64_t frames_bytes, const float\* lut_f32" % NAME, header)
    fn = getattr(_lib(), NAME)
    assert len(fn.argtypes) == 12 and fn.argtypes == getattr(hip.load(), "svit_im2col_patch_u8_aug").argtypes


def test_argument_checks_without_gpu():
    fn = getattr(_lib(), NAME)
    T, Hs, Ws, S = 2, 8, 8, 4
    video = T * Hs * Ws * 3
    P_ = 64                                                 # any aligned non-NULL address: nothing is dereferenced

    def call(frames=P_, nbytes=video, lut=P_, aug=P_, mix=None, cols=P_, B=1, T=T, S=S):
        return fn(frames, nbytes, lut, aug, mix, cols, B, T, Hs, Ws, S, None)

    assert call(frames=None) == ERR_ARG
    assert call(aug=None) == ERR_ARG
    assert call(cols=None) == ERR_ARG
    assert call(lut=None) == ERR_ARG
    assert call(B=0) == ERR_SHAPE
    assert call(S=0) == ERR_SHAPE
    assert call(T=0) == ERR_SHAPE
    assert call(nbytes=video - 1) == ERR_SHAPE              # less than one video
    assert call(cols=P_ + 8) == ERR_ALIGN                   # cols is written in 16-byte pieces
    assert call(mix=P_ + 2) == ERR_ALIGN
    assert call(aug=P_ + 2) == ERR_ALIGN
    assert call(B=1 << 20, T=1 << 11, S=16384, nbytes=(1 << 11) * Hs * Ws * 3) == ERR_SHAPE     # B*T*Ho = 2^43 blocks


def _stub(cls, **attrs):
    """an instance without the constructor (which wants the GPU): FramesView only reads attributes"""
    obj = cls.__new__(cls)
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def test_frames_view_reports_single_frame_clips():
    import pytest
    from svit_amd.augment import AugClips
    from svit_amd.input import FramesView, U8Clips
    frames = torch.zeros((3, 5, 12, 16, 3), dtype=torch.uint8)
    mix = torch.zeros(8, dtype=torch.int32)
    u8 = _stub(U8Clips, frames=frames, size=8, crops=torch.tensor([[0, 1, 2], [2, 4, 8]], dtype=torch.int32), mix=None)
    aug = _stub(AugClips, frames=frames, size=6, records=torch.zeros((4, 16), dtype=torch.int32), mix=mix)
    for clips, B, S in ((u8, 2, 8), (aug, 4, 6)):
        view = FramesView(clips)
        assert tuple(clips.shape) == (B, 3, 5, S, S)
        assert tuple(view.shape) == (B * 5, 3, 1, S, S) and isinstance(view.shape, torch.Size)
        assert view.dim() == 5 and view.device == frames.device and view.size == S
        assert view.detach() is view and view.contiguous() is view
        assert view.frames is frames and view.mix is clips.mix and not view.fresh        # shared, not copied
    assert FramesView(aug).device_records() is aug.records
    assert FramesView(aug, fresh=True).fresh
    u8.mix = mix                                            # the view reads the clips when it is used
    assert FramesView(u8).mix is mix
    with pytest.raises(TypeError):
        FramesView(frames)


def test_identity_records_equal_augrecord_identity():
    from svit_amd.augment import AugRecord, pack_records, unpack_records
    from svit_amd.input import FramesView, U8Clips, identity_records
    crops = torch.tensor([[0, 0, 0], [2, 5, 7], [1, 31, 0], [2, 5, 7]], dtype=torch.int32)
    rec = identity_records(crops, 64)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (4, 16) and rec.device == crops.device
    assert rec.is_contiguous()
    for row, (v, y0, x0) in zip(unpack_records(rec), crops.tolist()):
        assert row == AugRecord.identity(v, y0, x0, 64)
        assert tuple(row) == (v, y0, x0, 64, 64, 64, 64) + (0,) * 9
    assert torch.equal(rec, pack_records([AugRecord.identity(v, y0, x0, 64) for v, y0, x0 in crops.tolist()]))
    # a view over a U8Clips feeds exactly these, rebuilt from the table it finds
    u8 = _stub(U8Clips, frames=torch.zeros((3, 2, 96, 96, 3), dtype=torch.uint8), size=64, crops=crops, mix=None)
    view = FramesView(u8)
    assert torch.equal(view.device_records(), rec)
    crops[1, 1] = 9
    assert int(view.device_records()[1, 1]) == 9
