"""Closed-form uint8 sources and the case lists shared by tools/gen_randaug_golden.py (which records the reference's
outputs for them) and tests/test_randaug_*.py (which regenerate the sources and read the recorded outputs)."""
import numpy as np

SET_NAMES = ["ssv2_bicubic", "ssv2_random", "default_bilinear", "weighted"]
SETS = [("rand-m7-n4-mstd0.5-inc1", "bicubic"), ("rand-m7-n4-mstd0.5-inc1", "random"),
        ("rand-m9-mstd0.5-inc1", "bilinear"), ("rand-m5-n3-w0", "bicubic")]
N_SEEDS, N_CHAINS = 32, 4
SHAPES = [(2, 3, 24, 32, 3), (2, 3, 32, 24, 3)]         # both orientations: translate-x scales with the width
STREAM_SIZE, STREAM_T = (240, 320), 2                   # the clip of the draw + SpatialSampler.draw stream case


def _mix(i):
    """a 32-bit integer hash of the flat index (xorshift-multiply), closed form"""
    x = (i.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    return x.astype(np.int64)


def source(shape):
    """u8 `shape` = [V,T,H,W,3]: a smooth ramp per channel plus 3 hashed bits, different in every frame"""
    V, T, H, W, _ = shape
    v, t, y, x, c = np.meshgrid(*(np.arange(n, dtype=np.int64) for n in shape), indexing="ij")
    ramp = (x * (5 + c) + y * (7 - 2 * c) + 40 * t + 90 * v) % 248
    noise = _mix(np.arange(int(np.prod(shape)), dtype=np.int64)).reshape(shape) & 7
    return (ramp + noise).astype(np.uint8)


def special_frames():
    """u8 [3,1,24,32,3], one frame each: a single colour (AutoContrast / Equalize identity); fewer than 255 pixels
    outside the top bin (Equalize step == 0); hash-like with ONE pixel in the top bin (Equalize quotient 256)"""
    H, W = 24, 32
    flat = np.full((H, W, 3), 93, dtype=np.uint8)
    few = np.full((H * W, 3), 200, dtype=np.uint8)
    few[:100] = (_mix(np.arange(300, dtype=np.int64)) % 200).reshape(100, 3)
    noisy = (_mix(np.arange(H * W * 3, dtype=np.int64) + 7) % 255).astype(np.uint8).reshape(H * W, 3)
    noisy[5] = 255
    return np.stack([flat, few.reshape(H, W, 3), noisy.reshape(H, W, 3)])[:, None]


def single_cases(shape_index=0):
    """[(name, level arguments, filter or None)]: every operation at two magnitudes and both signs, the geometric ones
    under both filters.  The arguments are what the reference's level functions return for magnitudes 3 and 7.
    shape_index 1: only the operations whose map depends on the frame's size (Rotate, Translate*Rel)."""
    if shape_index == 1:
        return [c for c in single_cases(0) if c[0] in ("Rotate", "TranslateXRel", "TranslateYRel")]
    cases = [("AutoContrast", (), None), ("Equalize", (), None), ("Invert", (), None)]
    for lvl in (3.0, 7.0):
        cases += [("Posterize", (int(lvl / 10 * 4),), None), ("PosterizeIncreasing", (4 - int(lvl / 10 * 4),), None),
                  ("Solarize", (int(lvl / 10 * 256),), None), ("SolarizeIncreasing", (256 - int(lvl / 10 * 256),), None),
                  ("SolarizeAdd", (int(lvl / 10 * 110),), None)]
        for sign in (1.0, -1.0):
            for name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
                cases.append((name, (1.0 + sign * (lvl / 10 * 0.9),), None))
            for filt in (0, 1):
                cases.append(("Rotate", (sign * (lvl / 10 * 30.0),), filt))
                cases += [(n, (sign * (lvl / 10 * 0.3),), filt) for n in ("ShearX", "ShearY")]
                cases += [(n, (sign * (lvl / 10 * 0.45),), filt) for n in ("TranslateXRel", "TranslateYRel")]
    # half-pixel shifts: an output column / row maps exactly onto the frame's far edge
    cases += [("TranslateXRel", (0.5 / 32,), 0), ("TranslateYRel", (0.5 / 32,), 1), ("Posterize", (8,), None)]
    return cases


def single_source(shape_index):
    """the one frame the single operations are recorded on: video 1, frame 2 of SHAPES[shape_index] -> [1,1,H,W,3]"""
    return source(SHAPES[shape_index])[1:2, 2:3]
