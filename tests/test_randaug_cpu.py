"""svit_amd.randaug on the host (no GPU): the grammar, the draws against the reference's recorded ones
(tests/golden/randaug.npz, tools/gen_randaug_golden.py) and `apply_host` against PIL's recorded bytes."""
import os
import random

import numpy as np
import pytest

from svit_amd import randaug
from svit_amd.augment import build_sampler
from svit_amd.config import CfgNode, get_cfg
from svit_amd.randaug import RandAugOp, RandAugSampler, apply_host, build_randaug, parse_aa_type

from . import randaug_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def yaml_cfg():
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(GOLDEN, "ssv2.yaml"))
    return cfg


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "randaug.npz")))


def test_module_does_not_import_pil():
    src = open(randaug.__file__).read()
    assert "import PIL" not in src and "from PIL" not in src


def test_parser():
    p = parse_aa_type("rand-m7-n4-mstd0.5-inc1")
    assert (p["magnitude"], p["num_layers"], p["magnitude_std"]) == (7, 4, 0.5)
    assert p["transforms"] == randaug.RAND_INCREASING_TRANSFORMS and p["weights"] is None
    p = parse_aa_type("rand")
    assert (p["magnitude"], p["num_layers"], p["magnitude_std"]) == (10, 2, 0.0)
    assert p["transforms"] == randaug.RAND_TRANSFORMS
    assert parse_aa_type("rand-mstd1-w0")["magnitude_std"] == 1.0
    assert parse_aa_type("rand-m9-mstd0.5-mstd2")["magnitude_std"] == 0.5      # setdefault: the first holds
    assert parse_aa_type("rand-m9-foo-n3")["num_layers"] == 3                  # a section without a digit is passed over
    with pytest.raises(NotImplementedError):
        parse_aa_type("augmix-m5")


def test_parser_quirks():
    # bool("0") is true: inc0 selects the increasing set as inc1 does
    assert parse_aa_type("rand-m9-inc0")["transforms"] == randaug.RAND_INCREASING_TRANSFORMS
    assert parse_aa_type("rand-m9")["transforms"] == randaug.RAND_TRANSFORMS
    # w0: the weights by the plain set's names, normalised; Posterize and Invert never drawn
    w = parse_aa_type("rand-m5-n3-w0")["weights"]
    assert w.shape == (15,) and abs(w.sum() - 1) < 1e-12
    assert w[randaug.RAND_TRANSFORMS.index("Rotate")] == 0.3 / np.sum([randaug.RAND_CHOICE_WEIGHTS_0[k]
                                                                        for k in randaug.RAND_TRANSFORMS])
    assert w[randaug.RAND_TRANSFORMS.index("Invert")] == 0 and w[randaug.RAND_TRANSFORMS.index("Posterize")] == 0
    wi = parse_aa_type("rand-m5-n3-w0-inc1")
    assert wi["transforms"] == randaug.RAND_INCREASING_TRANSFORMS and (wi["weights"] == w).all()


def test_build_randaug_reads_cfg():
    cfg = yaml_cfg()
    ra = build_randaug(cfg)
    assert (ra.aa_type, ra.interpolation, ra.num_layers, ra.magnitude) == ("rand-m7-n4-mstd0.5-inc1", "bicubic", 4, 7)
    cfg.AUG = CfgNode({"ENABLE": True})
    ra = build_randaug(cfg)                 # the reference's defaults
    assert (ra.aa_type, ra.filter, ra.num_layers) == ("rand-m9-mstd0.5-inc1", randaug.BICUBIC, 2)
    cfg.AUG = CfgNode({"ENABLE": False, "AA_TYPE": "rand-m7"})
    assert build_randaug(cfg) is None
    del cfg["AUG"]
    assert build_randaug(cfg) is None


def test_record_round_trip():
    r = RandAugOp(randaug.OP_AFFINE, 3, 1.2999999523162842, 0x80000005, (1, 0.25, -3.5, 1e300, float("inf"), -0.0))
    w = r.pack()
    assert w.dtype == np.int32 and w.shape == (16,)
    assert RandAugOp.unpack(w) == r
    assert w[4:6].view(np.float64)[0] == 1.0


@pytest.mark.parametrize("s", range(len(C.SETS)))
def test_draw_reproduces_the_reference(gold, s):
    aa, interp = C.SETS[s]
    assert (str(gold["set_aa"][s]), str(gold["set_interp"][s])) == (aa, interp)
    names = [str(n) for n in gold["names"]]
    sampler = RandAugSampler(aa, interp)
    N = int(gold["n_layers"][s])
    ran = 0
    for k in range(C.N_SEEDS):
        _, T, Hs, Ws, _ = C.SHAPES[k % 2]
        random.seed(k)
        np.random.seed(k)
        ops = sampler.draw(T, Hs, Ws, video=k % 2)
        assert len(ops) == N == len(sampler.trace)
        for n, (name, args, filters) in enumerate(sampler.trace):
            g = int(gold["draw_op"][s, k, n])
            if g < 0:
                assert name == "" and ops[n].op == randaug.OP_NONE, (s, k, n)
                continue
            ran += 1
            assert name == names[g], (s, k, n)
            ga = gold["draw_arg"][s, k, n]
            assert (args == ()) if np.isnan(ga) else (float(args[0]) == ga), (s, k, n, args, ga)
            gf = [int(f) for f in gold["draw_filter"][s, k, n]]
            assert (list(filters) == gf) if gf[0] >= 0 else (filters == ()), (s, k, n)
        # both streams stand where the reference left them
        assert [random.random(), np.random.uniform()] == list(gold["tail"][s, k]), (s, k)
    assert ran > N * C.N_SEEDS // 4


def test_random_interpolation_is_drawn_per_frame(gold):
    f = gold["draw_filter"][1]
    mixed = [(k, n) for k in range(C.N_SEEDS) for n in range(4) if f[k, n, 0] >= 0 and len(set(f[k, n].tolist())) == 2]
    assert mixed                              # the fixture holds layers whose frames got different filters
    with pytest.raises(NotImplementedError):
        RandAugSampler(C.SETS[1][0], "random").draw(33, 24, 32)


def test_draw_then_spatial_draw_leaves_the_streams_where_the_loader_does(gold):
    cfg = yaml_cfg()
    cfg.AUG.INTERPOLATION = "random"
    ra, sp = build_randaug(cfg), build_sampler(cfg, "train")
    Hs, Ws = C.STREAM_SIZE
    for k in range(C.N_SEEDS):
        random.seed(k)
        np.random.seed(k)
        ra.draw(C.STREAM_T, Hs, Ws)
        rec = sp.draw(Hs, Ws)
        ref_r, ref_np, ref_seed, ref_r_after_seed = gold["stream_tail"][k]
        assert np.random.uniform() == ref_np, k
        if rec.erase_mode:                    # the ONE draw SpatialSampler adds: the noise seed (svit_amd/augment.py)
            assert rec.seed == int(ref_seed) and random.random() == ref_r_after_seed, k
        else:
            assert random.random() == ref_r, k


def _single_table(name, args, filt, Hs, Ws):
    return [[randaug.make_op(name, args, () if filt is None else (filt,), Hs, Ws)]]


@pytest.mark.parametrize("si", range(2))
def test_apply_host_single_operations_equal_pil(gold, si):
    src = C.single_source(si)
    Hs, Ws = src.shape[2:4]
    cases = C.single_cases(si)
    assert len(cases) == len(gold["single_%d" % si])
    for (name, args, filt), ref in zip(cases, gold["single_%d" % si]):
        got = apply_host(src, _single_table(name, args, filt, Hs, Ws))[0, 0]
        assert np.array_equal(got, ref), (name, args, filt, int((got != ref).sum()))


def test_apply_host_special_frames_equal_pil(gold):
    """single colour (identity tables), Equalize step == 0, and the Equalize quotient of 256 that PIL clamps"""
    sp = C.special_frames()
    h = np.bincount(sp[2, 0, ..., 0].ravel(), minlength=256)
    step = (int(h.sum()) - int(h[255])) // 255
    assert h[255] == 1 and (step // 2 + int(h[:255].sum())) // step == 256
    h = np.bincount(sp[1, 0, ..., 0].ravel(), minlength=256)
    assert (int(h.sum()) - int(h[200])) // 255 == 0
    for f in range(3):
        for j, op in enumerate((randaug.OP_AUTOCONTRAST, randaug.OP_EQUALIZE)):
            got = apply_host(sp[f:f + 1], [[RandAugOp(op)]])[0, 0]
            assert np.array_equal(got, gold["special"][f, j]), (f, op)


def test_apply_host_chains_equal_pil(gold):
    for s, (aa, interp) in enumerate(C.SETS):
        sampler = RandAugSampler(aa, interp)
        for k in range(C.N_CHAINS):
            src = C.source(C.SHAPES[k % 2])[k % 2:k % 2 + 1]
            random.seed(k)
            np.random.seed(k)
            ops = sampler.draw(*src.shape[1:4])
            got = apply_host(src, [ops])[0]
            ref = gold["chain_%d_%d" % (s, k)]
            assert np.array_equal(got, ref), (s, k, sampler.trace, int((got != ref).sum()))


def test_apply_host_survives_any_record():
    src = C.source((1, 2, 17, 23, 3))
    nan, big = float("nan"), 1e300
    for rec in (RandAugOp(99), RandAugOp(-1)):
        assert np.array_equal(apply_host(src, [[rec]]), src)
    for m in ((big, 0, 0, 0, big, 0), (-big, 0, 0, 0, -big, 0), (nan,) * 6, (1, 0, nan, 0, 1, 0), (1, 0, 0, 0, 1, big)):
        for mask in (0, 3):
            assert (apply_host(src, [[RandAugOp(randaug.OP_AFFINE, bicubic_mask=mask, m=m)]]) == 128).all(), m


def test_build_flags_per_source():
    """randaug.hip alone is compiled without -ffast-math and with -ffp-contract=off; it keeps -fno-slp-vectorize"""
    from svit_amd import build
    f = build.flags_for("randaug.hip")
    assert "-ffast-math" not in f and "-ffp-contract=off" in f and "-fno-slp-vectorize" in f
    assert "randaug.hip" in build.SOURCES
    for src in build.SOURCES:
        if src != "randaug.hip":
            assert build.flags_for(src) == build.FLAGS
