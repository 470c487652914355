"""Shapes and tables shared by tests/test_feeder_cpu.py and tests/test_feeder_gpu.py (svit_amd/feeder.py, csrc/feed.hip).

Buffers (Hs, Ws) with row pitches of 9, 15, 21, 48 and 72 bytes: a 16-byte chunk of the destination spans three rows, two
rows, a row and its padding, exactly a third of a row, and rows astride.  Four videos per case from 1x1, 3x3, the full
buffer, one column short, one row short, 12x11 (33-byte rows) and 20x19 (57-byte rows), as they fit."""
import numpy as np

BUFFERS = [(3, 3), (4, 5), (5, 7), (12, 16), (20, 24)]


def WILD_EXTENTS(Hs):
    return [(0, 0), (-5, 10 ** 9), (Hs + 1, 1)]           # (clamped: (1,1), (1,Ws), (Hs,1))


def candidates(Hs, Ws):
    out = []
    for h, w in [(1, 1), (3, 3), (Hs, Ws), (Hs, Ws - 1), (Hs - 1, Ws), (12, 11), (20, 19)]:
        if 1 <= h <= Hs and 1 <= w <= Ws and (h, w) not in out:
            out.append((h, w))
    return out


def shape_cases():
    """[(Hs, Ws, T, four sizes)]: every candidate of every buffer at T = 1 and T = 2"""
    cases = []
    for Hs, Ws in BUFFERS:
        cand = candidates(Hs, Ws)
        for T in (1, 2):
            for d in range((len(cand) + 3) // 4):
                cases.append((Hs, Ws, T, [cand[(4 * d + i) % len(cand)] for i in range(4)]))
    return cases


def random_videos(sizes, T, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(T, h, w, 3), dtype=np.uint8) for h, w in sizes]


def clamp(extent, Hs, Ws):
    return min(max(int(extent[0]), 1), Hs), min(max(int(extent[1]), 1), Ws)


def wild_offsets(slot_bytes, n_v, valid):
    """the issue's list for a video of n_v bytes: before the slot, at its end, far outside, one byte too far, and a
    valid offset that is not a multiple of anything"""
    odd = valid + 1 if valid + 1 <= slot_bytes - n_v else max(slot_bytes - n_v - 1, 0) | 1
    if odd > slot_bytes - n_v:
        odd = slot_bytes - n_v
    return [-1, slot_bytes, 2 ** 40, slot_bytes - n_v + 1, odd]


def wild_tables(slot_bytes, T, Hs, Ws, offsets, extents, seeds=6):
    """[(offsets, extents)] over four videos: each wild offset and each wild extent on one video with the others valid,
    every wild extent at an offset where the clamped video no longer fits, then random mixtures"""
    offsets, extents = [int(o) for o in offsets], [tuple(int(x) for x in e) for e in extents]
    V = len(offsets)
    out = []
    for v in range(V):
        n_v = T * extents[v][0] * extents[v][1] * 3
        for o in wild_offsets(slot_bytes, n_v, offsets[v]):
            out.append((offsets[:v] + [o] + offsets[v + 1:], list(extents)))
    for k, e in enumerate(WILD_EXTENTS(Hs)):
        v = k % V
        h, w = clamp(e, Hs, Ws)
        out.append((list(offsets), extents[:v] + [e] + extents[v + 1:]))
        out.append((offsets[:v] + [slot_bytes - T * h * w * 3 + 1] + offsets[v + 1:], extents[:v] + [e] + extents[v + 1:]))
    for seed in range(seeds):
        rng = np.random.default_rng(100 + seed)
        offs, exts = [], []
        for v in range(V):
            e = (WILD_EXTENTS(Hs) + [extents[v], (Hs, Ws)])[int(rng.integers(0, 5))]
            h, w = clamp(e, Hs, Ws)
            n_v = T * h * w * 3
            pool = wild_offsets(slot_bytes, n_v, offsets[v]) + [offsets[v], int(rng.integers(0, slot_bytes))]
            offs.append(pool[int(rng.integers(0, len(pool)))])
            exts.append(e)
        out.append((offs, exts))
    return out


def slow_unpack(slot, offsets, extents, T, Hs, Ws, fill, swap_rb):
    """the header's rule byte by byte, with every slot index asserted inside the slot"""
    n = len(slot)
    V = len(offsets)
    out = np.full((V, T, Hs, Ws, 3), fill, dtype=np.uint8)
    for v in range(V):
        h, w = clamp(extents[v], Hs, Ws)
        n_v, off = T * h * w * 3, int(offsets[v])
        if off < 0 or off > n - n_v:
            continue
        for t in range(T):
            for y in range(h):
                for x in range(w):
                    for c in range(3):
                        i = off + ((t * h + y) * w + x) * 3 + (2 - c if swap_rb else c)
                        assert 0 <= i < n
                        out[v, t, y, x, c] = slot[i]
    return out
