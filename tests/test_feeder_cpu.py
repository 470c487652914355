"""Host side of the batch feeder (svit_amd/feeder.py) and the argument checks of svit_feed_unpack (csrc/feed.hip) -- no GPU.
`unpack_host` is the kernel's yardstick, so it is held here to `pack_videos` on valid batches and, on wild tables, to the
header's rule applied byte by byte with every slot index asserted inside the slot (tests/feeder_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import feeder_cases as FC


@pytest.fixture(scope="module")
def F():
    from svit_amd import feeder
    return feeder


@pytest.mark.parametrize("case", FC.shape_cases(), ids=lambda c: "%dx%d_T%d_%s" % (c[0], c[1], c[2], "_".join("%dx%d" % s for s in c[3])))
def test_unpack_of_pack_tight_is_pack_videos(F, case):
    from svit_amd.augment import pack_videos
    Hs, Ws, T, sizes = case
    vids = FC.random_videos(sizes, T, seed=Hs * 100 + Ws + T)
    poisoned = np.full(F.tight_bytes(sizes, T) + 32, 0xA7, dtype=np.uint8)
    slot, offsets, extents = F.pack_tight(vids, out=poisoned)
    assert slot.size % 16 == 0 and slot.size == F.tight_bytes(sizes, T) and slot.base is poisoned
    assert offsets.dtype == np.int64 and extents.dtype == np.int32 and extents.tolist() == [list(s) for s in sizes]
    # 16-byte aligned, ordered, end to end: each start is the previous end rounded up
    assert all(int(o) % 16 == 0 for o in offsets) and offsets[0] == 0
    for v in range(1, len(sizes)):
        end = int(offsets[v - 1]) + T * sizes[v - 1][0] * sizes[v - 1][1] * 3
        assert int(offsets[v]) == (end + 15) // 16 * 16
    # nothing zeroed: the gaps and the bytes behind the batch keep the poison
    used = np.zeros(poisoned.size, dtype=bool)
    for v, (h, w) in enumerate(sizes):
        used[int(offsets[v]):int(offsets[v]) + T * h * w * 3] = True
    assert bool((poisoned[~used] == 0xA7).all())
    want, ext = pack_videos([torch.from_numpy(x) for x in vids], Hs=Hs, Ws=Ws)
    got = F.unpack_host(slot, offsets, extents, T, Hs, Ws)
    assert got.shape == tuple(want.shape) and np.array_equal(got, want.numpy()) and np.array_equal(extents, ext.numpy())
    # torch videos and a fresh buffer give the same bytes where bytes were written
    slot2, offsets2, _ = F.pack_tight([torch.from_numpy(x) for x in vids])
    assert np.array_equal(offsets2, offsets) and np.array_equal(F.unpack_host(slot2, offsets2, extents, T, Hs, Ws), got)
    # fill and swap_rb: padding 255, channels reversed inside the extents
    swapped = F.unpack_host(slot, offsets, extents, T, Hs, Ws, fill=255, swap_rb=True)
    for v, (h, w) in enumerate(sizes):
        assert np.array_equal(swapped[v, :, :h, :w], vids[v][..., ::-1])
        assert bool((swapped[v, :, h:] == 255).all()) and bool((swapped[v, :, :, w:] == 255).all())


def test_pack_tight_refusals(F):
    a, b = np.zeros((2, 3, 3, 3), np.uint8), np.zeros((1, 3, 3, 3), np.uint8)
    with pytest.raises(ValueError, match="at least one"):
        F.pack_tight([])
    with pytest.raises(ValueError, match="has 1 frames"):
        F.pack_tight([a, b])
    with pytest.raises(ValueError, match="uint8"):
        F.pack_tight([a.astype(np.int32)])
    with pytest.raises(ValueError, match="needs"):
        F.pack_tight([a], out=np.zeros(16, np.uint8))


@pytest.mark.parametrize("swap_rb", [False, True])
def test_unpack_host_on_wild_tables_stays_inside_the_slot(F, swap_rb):
    Hs, Ws, T = 12, 16, 2
    sizes = [(12, 16), (3, 3), (12, 11), (11, 16)]
    vids = FC.random_videos(sizes, T, seed=5)
    slot, offsets, extents = F.pack_tight(vids)
    n = slot.size
    tables = FC.wild_tables(n, T, Hs, Ws, offsets, extents)
    assert len(tables) >= 4 * 5 + 6 + 6
    absent = 0
    for offs, exts in tables:
        outs = []
        for sentinel in (0x00, 0xFF):              # the slot inside a larger array: nothing behind it reaches the result
            big = np.full(n + 4096, sentinel, dtype=np.uint8)
            big[2048:2048 + n] = slot
            outs.append(F.unpack_host(big[2048:2048 + n], offs, exts, T, Hs, Ws, fill=77, swap_rb=swap_rb))
        assert np.array_equal(outs[0], outs[1])
        assert np.array_equal(outs[0], FC.slow_unpack(slot, offs, exts, T, Hs, Ws, 77, swap_rb)), (offs, exts)
        for v in range(4):
            h, w = FC.clamp(exts[v], Hs, Ws)
            if offs[v] < 0 or offs[v] > n - T * h * w * 3:        # a video that does not fit is all fill
                assert bool((outs[0][v] == 77).all())
                absent += 1
    assert absent >= 4 * 4


def test_wild_extents_clamp_as_the_other_kernels_do(F):
    from svit_amd.augment import clamp_extents
    Hs, Ws = 12, 16
    wild = FC.WILD_EXTENTS(Hs)
    assert [list(FC.clamp(e, Hs, Ws)) for e in wild] == clamp_extents(wild, Hs, Ws).tolist() == [[1, 1], [1, Ws], [Hs, 1]]
    slot = np.arange(16 * 40, dtype=np.int64).astype(np.uint8)
    got = F.unpack_host(slot, [0, 16, 32], wild, 1, Hs, Ws, fill=9)
    assert got[0, 0, 0, 0].tolist() == [0, 1, 2] and int((got[0] != 9).sum()) <= 3
    assert np.array_equal(got[1, 0, 0].reshape(-1), slot[16:16 + Ws * 3]) and bool((got[1, 0, 1:] == 9).all())
    assert np.array_equal(got[2, 0, :, 0].reshape(-1), slot[32:32 + Hs * 3]) and bool((got[2, 0, :, 1:] == 9).all())


def test_slot_layout_is_aligned_and_fits(F):
    for V, T, Hs, Ws, B, N, ext, labels in [(4, 2, 12, 16, 4, 4, True, [32]), (3, 1, 20, 24, 3, 2, True, [3 * 64, 3 * 8]),
                                            (2, 4, 20, 24, 2, 0, False, [16]), (1, 1, 3, 3, 5, 1, True, [1, 7, 0])]:
        lay = F.layout_for(V, T, Hs, Ws, B, randaug_layers=N, extents=ext, label_bytes=labels)
        names = [n for n, _ in lay.parts]
        assert names[0] == "records" and names[-1] == "offsets" and ("extents" in names) == ext and ("randaug" in names) == bool(N)
        assert lay.slot_bytes % 16 == 0 and lay.frames_max == F.tight_bytes([(Hs, Ws)] * V, T)
        for frames_bytes in (0, 16, 27, lay.frames_max // 2, lay.frames_max):
            where, total = lay.at(frames_bytes)
            assert total % 16 == 0 and 16 <= total <= lay.slot_bytes
            at = frames_bytes
            for name, nbytes in lay.parts:               # in order, 16-byte aligned, no overlap, inside the slot
                assert where[name] % 16 == 0 and where[name] >= at
                at = where[name] + nbytes
            assert at <= total
        assert lay.at(lay.frames_max)[1] == lay.slot_bytes
        with pytest.raises(ValueError):
            lay.at(lay.frames_max + 1)


# ------------------------------------------------------------------------------------------------- the library ----
def test_entry_point_is_bound():
    from svit_amd import hip
    assert "svit_feed_unpack" in hip.EXPORTS
    assert C.sizeof(hip.FeedSeg) == 24 and C.sizeof(hip.FeedArgs) == 5 * 8 + 8 * 4 + 8 * 24


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    return hip.load()


def good_args():
    from svit_amd import hip
    a = hip.FeedArgs()
    a.slot, a.slot_bytes, a.frames = 4096, 1024, 8192
    a.V, a.T, a.Hs, a.Ws, a.fill, a.swap_rb, a.n_seg = 2, 2, 5, 7, 0, 0, 2
    a.seg[0].src_off, a.seg[0].dst, a.seg[0].bytes = 512, 16384, 64
    a.seg[1].src_off, a.seg[1].dst, a.seg[1].bytes = 1008, 16516, 16
    return a


MALFORMED = [
    ("null slot", lambda a: setattr(a, "slot", None), -4),
    ("null frames", lambda a: setattr(a, "frames", None), -4),
    ("slot not 16-byte aligned", lambda a: setattr(a, "slot", 4096 + 8), -3),
    ("frames not 16-byte aligned", lambda a: setattr(a, "frames", 8192 + 4), -3),
    ("slot_bytes not a multiple of 16", lambda a: setattr(a, "slot_bytes", 1000), -3),
    ("offsets not 8-byte aligned", lambda a: setattr(a, "offsets", 4096 + 4), -3),
    ("extents not 4-byte aligned", lambda a: setattr(a, "extents", 4096 + 2), -3),
    ("V = 0", lambda a: setattr(a, "V", 0), -2),
    ("T = 0", lambda a: setattr(a, "T", 0), -2),
    ("Hs < 0", lambda a: setattr(a, "Hs", -3), -2),
    ("Ws = 0", lambda a: setattr(a, "Ws", 0), -2),
    ("slot_bytes = 0", lambda a: setattr(a, "slot_bytes", 0), -2),
    ("a video of 2^31 bytes", lambda a: (setattr(a, "T", 1024), setattr(a, "Hs", 1024), setattr(a, "Ws", 683)), -2),
    ("fill = 256", lambda a: setattr(a, "fill", 256), -4),
    ("fill = -1", lambda a: setattr(a, "fill", -1), -4),
    ("n_seg = 9", lambda a: setattr(a, "n_seg", 9), -4),
    ("n_seg = -1", lambda a: setattr(a, "n_seg", -1), -4),
    ("segment past the slot", lambda a: setattr(a.seg[1], "bytes", 17), -4),
    ("segment starting past the slot", lambda a: setattr(a.seg[0], "src_off", 1024 + 16), -4),
    ("segment with negative bytes", lambda a: setattr(a.seg[0], "bytes", -1), -4),
    ("segment with a negative offset", lambda a: setattr(a.seg[0], "src_off", -16), -4),
    ("segment with a null target", lambda a: setattr(a.seg[1], "dst", None), -4),
    ("segment offset not a multiple of 16", lambda a: setattr(a.seg[0], "src_off", 520), -3),
    ("segment target not 4-byte aligned", lambda a: setattr(a.seg[1], "dst", 16518), -3),
]


@pytest.mark.parametrize("what,spoil,code", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_library_refuses_malformed_arguments_before_any_launch(lib, what, spoil, code):
    """every pointer here is a made-up number: a call that got as far as a launch would fault or return a hipError_t,
    not the header's negative code"""
    a = good_args()
    spoil(a)
    assert lib.svit_feed_unpack(C.byref(a), None) == code, what


def test_null_argument_struct_is_refused(lib):
    assert lib.svit_feed_unpack(None, None) == -4
