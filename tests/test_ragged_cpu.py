"""Per-video extents on the uint8 input route, host side: `augment.pack_videos`, records validated / clamped against their
own video, the NumPy RandAugment yardstick on a padded batch, the refusals, and the ABI of the `_ext` entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from svit_amd import augment as A
from svit_amd import randaug as RA
from tests import randaug_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_NAMES = ["svit_im2col_patch_u8_aug_ext", "svit_im2col_patch_u8_aug_frames_ext", "svit_u8_clips_render_ext",
             "svit_randaug_stats_ext", "svit_randaug_apply_ext"]


def videos(sizes, T=2):
    """host u8 [T,h,w,3] per size: the closed-form source of randaug_cases, a different video each"""
    return [torch.from_numpy(RC.source((k + 1, T, h, w, 3))[k]) for k, (h, w) in enumerate(sizes)]


# ---- pack_videos ------------------------------------------------------------------------------------------------------
def test_pack_videos_pads_with_zeros_and_returns_the_table():
    sizes = [(12, 16), (9, 16), (12, 11), (3, 3)]
    vids = videos(sizes)
    frames, ext = A.pack_videos(vids)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (4, 2, 12, 16, 3) and frames.is_contiguous()
    assert ext.dtype == torch.int32 and ext.tolist() == [list(s) for s in sizes]
    for v, (h, w) in enumerate(sizes):
        assert torch.equal(frames[v, :, :h, :w], vids[v])
        pad = frames[v].clone()
        pad[:, :h, :w] = 0
        assert int(pad.sum()) == 0
    # a given buffer size, and a reused buffer that held something else
    big, ext2 = A.pack_videos(vids, Hs=20, Ws=24)
    assert tuple(big.shape) == (4, 2, 20, 24, 3) and torch.equal(ext2, ext)
    assert torch.equal(big[:, :, :12, :16], frames) and int(big[:, :, 12:].sum()) == 0 and int(big[:, :, :, 16:].sum()) == 0
    dirty = torch.full((4, 2, 12, 16, 3), 255, dtype=torch.uint8)
    again, _ = A.pack_videos(vids, out=dirty)
    assert again is dirty and torch.equal(dirty, frames)


def test_pack_videos_error_paths():
    vids = videos([(12, 16), (9, 16)])
    with pytest.raises(ValueError, match="video 0 is 12x16, larger than the 10x16 buffer"):
        A.pack_videos(vids, Hs=10)
    with pytest.raises(ValueError, match="larger than the 12x15 buffer"):
        A.pack_videos(vids, Ws=15)
    with pytest.raises(ValueError, match="at least one"):
        A.pack_videos([])
    with pytest.raises(ValueError, match="video 1 has 3 frames"):
        A.pack_videos([vids[0], torch.zeros((3, 9, 16, 3), dtype=torch.uint8)])
    with pytest.raises(ValueError, match="video 1: expected a host uint8"):
        A.pack_videos([vids[0], vids[1].float()])
    with pytest.raises(ValueError, match="video 0: expected a host uint8"):
        A.pack_videos([vids[0][0]])
    with pytest.raises(ValueError, match="out must be"):
        A.pack_videos(vids, out=torch.zeros((2, 2, 12, 17, 3), dtype=torch.uint8))


# ---- records against their own video ----------------------------------------------------------------------------------
def R(video, i, j, h, w, out_h=8, out_w=8, oy=0, ox=0):
    return A.AugRecord(video, i, j, h, w, out_h, out_w, oy, ox, 0, 0, 0, 0, 0, 0, 0)


def test_validate_records_checks_each_record_against_its_own_video():
    ext = A.pack_extents([(12, 16), (9, 16), (12, 11), (3, 3)], 4, 12, 16)
    good = A.pack_records([R(0, 0, 0, 12, 16), R(1, 1, 0, 8, 16), R(2, 0, 3, 12, 8), R(3, 0, 0, 3, 3), R(3, 2, 2, 1, 1)])
    A.validate_records(good, 4, 12, 16, 8, ext)
    # each of these lies inside the 12x16 buffer, and outside its video
    for k, bad in enumerate([R(1, 2, 0, 8, 16), R(2, 0, 4, 12, 8), R(3, 0, 0, 4, 3), R(1, 0, 0, 10, 16)]):
        table = A.pack_records([R(0, 0, 0, 12, 16)] * k + [bad])
        A.validate_records(table, 4, 12, 16, 8)
        with pytest.raises(ValueError, match="augmentation record %d: source rectangle outside the extent" % k):
            A.validate_records(table, 4, 12, 16, 8, ext)
    with pytest.raises(ValueError, match="record 0: video outside"):
        A.validate_records(A.pack_records([R(4, 0, 0, 1, 1)]), 4, 12, 16, 8, ext)


def test_clamp_records_equals_a_numpy_restatement():
    rng = np.random.RandomState(5)
    V, Hs, Ws, S = 4, 12, 16, 8
    table = rng.randint(-6, 24, size=(200, 16)).astype(np.int32)
    table[::7, 3:5] = 10 ** 9
    table[::11, 1:3] = -10 ** 9
    for ext in ([(12, 16), (9, 16), (12, 11), (3, 3)], [(0, 0), (-5, 10 ** 9), (Hs + 1, 1), (7, 5)]):
        got = A.clamp_records(torch.from_numpy(table), V, Hs, Ws, S, np.array(ext, dtype=np.int64)).numpy()
        e = np.array(ext, dtype=np.int64)
        for b in range(table.shape[0]):
            r = [int(x) for x in table[b]]
            v = min(max(r[0], 0), V - 1)
            hv, wv = min(max(int(e[v, 0]), 1), Hs), min(max(int(e[v, 1]), 1), Ws)
            h, w = min(max(r[3], 1), hv), min(max(r[4], 1), wv)
            i, j = min(max(r[1], 0), hv - h), min(max(r[2], 0), wv - w)
            assert got[b, :5].tolist() == [v, i, j, h, w], (ext, b)
            assert i + h <= hv and j + w <= wv
        # everything but the rectangle is the clamp without extents
        plain = A.clamp_records(torch.from_numpy(table), V, Hs, Ws, S).numpy()
        assert np.array_equal(got[:, 5:], plain[:, 5:]) and np.array_equal(got[:, 0], plain[:, 0])
    # a table that validates is unchanged, and full extents are no extents
    good = A.pack_records([R(1, 1, 0, 8, 16), R(3, 2, 2, 1, 1)])
    assert torch.equal(A.clamp_records(good, V, Hs, Ws, S, [(12, 16), (9, 16), (12, 11), (3, 3)]), good)
    assert torch.equal(A.clamp_records(torch.from_numpy(table), V, Hs, Ws, S, [(Hs, Ws)] * V),
                       A.clamp_records(torch.from_numpy(table), V, Hs, Ws, S))
    assert A.clamp_extents([(0, 0), (-5, 10 ** 9), (Hs + 1, 1)], Hs, Ws).tolist() == [[1, 1], [1, Ws], [Hs, 1]]


# ---- the NumPy yardstick on a padded batch ----------------------------------------------------------------------------
SIZES = [(12, 16), (9, 16), (12, 11), (3, 3), (17, 19)]


def case_ops(name, args, filt, T, h, w):
    return [RA.make_op(name, args, () if filt is None else (filt,) * T, h, w)]


def test_apply_host_with_extents_equals_every_tight_video():
    """every operation of randaug_cases: the [h_v, w_v] corner is apply_host of the tight video, the padding (a
    pattern, not zeros) comes out as it went in"""
    T = 2
    vids = videos(SIZES, T)
    Hs, Ws = 20, 24
    frames, ext = A.pack_videos(vids, Hs=Hs, Ws=Ws)
    frames = frames.numpy()
    pad = np.ones(frames.shape[2:4], dtype=bool)
    padded = (RC.source(frames.shape) ^ 0x5A).astype(np.uint8)
    for v, (h, w) in enumerate(SIZES):
        padded[v, :, :h, :w] = frames[v, :, :h, :w]
    for name, args, filt in RC.single_cases():
        table = [case_ops(name, args, filt, T, h, w) for h, w in SIZES]
        got = RA.apply_host(padded, table, ext)
        for v, (h, w) in enumerate(SIZES):
            want = RA.apply_host(vids[v].numpy()[None], [table[v]])[0]
            assert np.array_equal(got[v, :, :h, :w], want), (name, args, filt, v)
            outside = pad.copy()
            outside[:h, :w] = False
            assert np.array_equal(got[v][:, outside], padded[v][:, outside]), (name, v)
    # the statistics really are the video's own: without the extents the padding changes the bytes inside
    table = [[RA.RandAugOp(RA.OP_EQUALIZE)] for _ in SIZES]
    assert not np.array_equal(RA.apply_host(padded, table)[1, :, :9, :16], RA.apply_host(padded, table, ext)[1, :, :9, :16])
    # None and full extents are the same thing
    assert np.array_equal(RA.apply_host(padded, table), RA.apply_host(padded, table, [(Hs, Ws)] * len(SIZES)))


def test_extents_are_refused_where_they_cannot_hold():
    frames = np.zeros((2, 1, 12, 16, 3), dtype=np.uint8)
    table = [[RA.RandAugOp(RA.OP_INVERT)]] * 2
    for bad, what in (([(12, 16), (2, 16)], "extent 1: 2x16 is smaller than 3x3"),
                      ([(12, 2), (12, 16)], "extent 0: 12x2 is smaller than 3x3"),
                      ([(13, 16), (12, 16)], "extent 0: 13x16 is larger than the 12x16 buffer"),
                      ([(12, 16), (12, 17)], "extent 1: 12x17 is larger than the 12x16 buffer")):
        with pytest.raises(ValueError, match=what):
            RA.apply_host(frames, table, bad)
    with pytest.raises(ValueError, match=r"extents are int \[2,2\]"):
        RA.apply_host(frames, table, [(12, 16)])
    with pytest.raises(ValueError, match="extents are int"):
        RA.pack_extents(np.array([[12.0, 16.0], [3.0, 3.0]]), 2, 12, 16)
    # without RandAugment an extent of 1 x 1 is a video; 0 is not
    assert A.pack_extents([(1, 1), (12, 16)], 2, 12, 16).tolist() == [[1, 1], [12, 16]]
    with pytest.raises(ValueError, match="extent 0: 0x4 is smaller than 1x1"):
        A.pack_extents([(0, 4), (12, 16)], 2, 12, 16)
    with pytest.raises(ValueError, match="smaller than 3x3"):
        A.pack_extents([(2, 2), (12, 16)], 2, 12, 16, min_side=3)


# ---- the ABI of the new entry points ----------------------------------------------------------------------------------
def test_header_binding_and_signatures_agree_on_the_new_entry_points():
    from svit_amd import hip
    text = open(os.path.join(ROOT, "include", "svit_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    types = {"int": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
    for name in EXT_NAMES:
        assert name in hip.EXPORTS
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        want = [C.c_void_p if "*" in p else types[p.split()[0]] for p in params]
        res, args = hip._SIGS[name]
        assert res is C.c_int32 and args == want, name
        # the plain entry point's parameters plus `extents`, right behind the records
        plain = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name[:-4], text).group(1)
        plain = [re.sub(r"\s+", " ", p.strip()) for p in plain.split(",")]
        mine = [re.sub(r"\s+", " ", p) for p in params]
        k = mine.index("const int32_t* extents")
        assert mine[:k] + mine[k + 1:] == plain and mine[k - 1] in ("const void* aug", "const void* records"), name
