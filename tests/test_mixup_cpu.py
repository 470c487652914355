"""cfg.MIXUP on the host (svit_amd/mixup.py, svit_amd/losses.py): the draws, the mixed clip and the soft target must be
what the reference's slowfast/datasets/mixup.py::MixUp produces after the same `np.random.seed` -- recorded by
tools/gen_mixup_golden.py in tests/golden/mixup.npz for four parameter sets (the reference's ssv2.yaml values; PROB 0.5;
mixup only; CutMix only) x seeds 0..31, plus mixed tiny clips.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from svit_amd import config, losses, mixup

TINY = (4, 3, 2, 16, 16)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "mixup.npz"))


def _fn(gold, s):
    alpha, cm_alpha, prob, switch = gold["set_params"][s]
    return mixup.MixUp(mixup_alpha=alpha, cutmix_alpha=cm_alpha, mix_prob=prob, switch_prob=switch,
                       label_smoothing=float(gold["smoothing"]), num_classes=int(gold["num_classes"]))


def tiny_clip():
    """the generator's closed-form input: ((37 i) mod 101 - 50) / 16 over the flat index, exact in fp32"""
    n = int(np.prod(TINY))
    v = ((np.arange(n, dtype=np.int64) * 37) % 101 - 50).astype(np.float32) / np.float32(16)
    return v.reshape(TINY)


def test_fixture_covers_the_cases(gold):
    lam, cm, box = gold["lam"], gold["cutmix"], gold["box"].astype(np.int64)
    assert (~cm & (lam != 1.0)).any() and (lam == 1.0).any()
    h, w = box[..., 1] - box[..., 0], box[..., 3] - box[..., 2]
    assert (cm & (h != w)).any()                              # a box clipped by a border: lam was corrected
    tb = gold["tiny_box"].astype(np.int64)
    assert (gold["tiny_cutmix"] & ((tb[..., 0] == tb[..., 1]) | (tb[..., 2] == tb[..., 3]))).any()   # an empty box


def test_draw_equals_the_reference_for_every_seed_and_set(gold):
    for s in range(len(gold["set_params"])):
        fn = _fn(gold, s)
        for k in range(gold["lam"].shape[1]):
            np.random.seed(k)
            rec = fn.draw((4, 3, 16, 224, 224))
            assert rec.lam == gold["lam"][s, k], (s, k, rec)           # exact float64
            assert rec.use_cutmix == bool(gold["cutmix"][s, k]), (s, k, rec)
            assert rec.box == tuple(int(v) for v in gold["box"][s, k]), (s, k, rec)
            assert rec.mode == (2 if rec.use_cutmix else (0 if rec.lam == 1.0 else 1))
        for j, k in enumerate(gold["tiny_seeds"][s]):
            np.random.seed(int(k))
            rec = fn.draw(TINY)
            assert rec.lam == gold["tiny_lam"][s, j] and rec.use_cutmix == bool(gold["tiny_cutmix"][s, j])
            assert rec.box == tuple(int(v) for v in gold["tiny_box"][s, j])


def test_draw_leaves_the_random_stream_where_the_reference_leaves_it(gold):
    """two draws in a row after one seed: the second only matches if the first consumed what the reference consumes --
    checked against re-seeding arithmetic: rand, [rand], beta, [randint, randint]"""
    fn = _fn(gold, 0)
    np.random.seed(5)
    a = fn.draw((4, 3, 16, 224, 224))
    nxt = np.random.rand()
    np.random.seed(5)
    np.random.rand()
    cut = np.random.rand() < 0.5
    np.random.beta(1.0, 1.0) if cut else np.random.beta(0.8, 0.8)
    if cut:
        np.random.randint(0, 224)
        np.random.randint(0, 224)
    assert a.use_cutmix == cut and np.random.rand() == nxt


def test_record_packing():
    rec = mixup.MixRecord(2, 0.3, 1, 5, 2, 9)
    w = rec.pack()
    assert w.dtype == np.int32 and w.shape == (8,) and w.nbytes == 32
    assert w[0] == 2 and list(w[3:7]) == [1, 5, 2, 9] and w[7] == 0
    lam, oml = w[1:3].view(np.float32)
    assert lam == np.float32(0.3)
    assert oml == np.float32(1.0 - 0.3)                       # the subtraction in double ...
    lam = 0.1 + 2.0 ** -30
    w = mixup.MixRecord(1, lam, 0, 0, 0, 0).pack()
    assert w[1:3].view(np.float32)[1] == np.float32(1.0 - lam)
    none = mixup.NO_MIX.pack()
    assert none[0] == 0 and tuple(none[1:3].view(np.float32)) == (1.0, 0.0)


def test_oml_is_not_one_minus_the_rounded_lambda(gold):
    """... and the fixture holds lambdas for which 1 - float32(lam) would round differently"""
    lam = gold["lam"].ravel()
    a = (1.0 - lam).astype(np.float32)
    b = np.float32(1.0) - lam.astype(np.float32)
    assert (a != b).any()


def test_call_on_host_tensors_equals_the_reference_bit_for_bit(gold):
    labels = torch.from_numpy(gold["labels"])
    for s in range(len(gold["set_params"])):
        fn = _fn(gold, s)
        for k in range(gold["lam"].shape[1]):
            np.random.seed(k)
            x = torch.zeros(4, 1, 1, 224, 224)
            out, target = fn(x, labels)
            assert out is x and target.dtype == torch.float32
            assert np.array_equal(target.numpy(), gold["target"][s, k]), (s, k)
        for j, k in enumerate(gold["tiny_seeds"][s]):
            np.random.seed(int(k))
            x = torch.from_numpy(tiny_clip())
            out, target = fn(x, labels)
            assert np.array_equal(out.numpy().view(np.int32), gold["tiny_mixed"][s, j].view(np.int32)), (s, k)
            assert np.array_equal(target.numpy(), gold["tiny_target"][s, j]), (s, k)
    with pytest.raises(AssertionError):
        fn(torch.zeros(1, 3, 2, 16, 16), labels[:1])


def test_mixed_labels_dense_equals_the_reference_target(gold):
    labels = torch.from_numpy(gold["labels"])
    for s in range(len(gold["set_params"])):
        fn = _fn(gold, s)
        for k in range(gold["lam"].shape[1]):
            np.random.seed(k)
            x = torch.zeros(4, 1, 1, 224, 224)
            out, mixed = fn.mix(x, labels)
            assert isinstance(mixed, mixup.MixedLabels) and mixed.labels is labels
            assert mixed.record.dtype == torch.int32 and mixed.record.numel() == 8
            assert np.array_equal(mixed.dense().numpy(), gold["target"][s, k]), (s, k)
    # the fused route mixes a host clip like the reference's call does
    s, j = 0, 0
    np.random.seed(int(gold["tiny_seeds"][s][j]))
    out, mixed = _fn(gold, s).mix(torch.from_numpy(tiny_clip()), labels)
    assert np.array_equal(out.numpy().view(np.int32), gold["tiny_mixed"][s, j].view(np.int32))
    # and an explicit record is applied as given
    rec = mixup.MixRecord(2, 0.75, 0, 8, 4, 16)
    x = torch.from_numpy(tiny_clip())
    out, _ = _fn(gold, s).mix(x, labels, record=rec)
    want = torch.from_numpy(tiny_clip())
    want[..., 0:8, 4:16] = want.flip(0)[..., 0:8, 4:16]
    assert torch.equal(out, want)


def test_build_mixup(golden_dir):
    assert mixup.build_mixup(config.get_cfg()) is None          # no MIXUP section in the default tree
    assert "MIXUP" not in config.get_cfg()
    cfg = config.get_cfg()
    cfg.merge_from_file(os.path.join(golden_dir, "ssv2.yaml"))
    assert "MIXUP" in cfg and mixup.build_mixup(cfg) is None     # the shipped yaml: ENABLE false
    cfg.MIXUP.ENABLE = True
    fn = mixup.build_mixup(cfg)
    assert isinstance(fn, mixup.MixUp)
    assert (fn.mixup_alpha, fn.cutmix_alpha, fn.mix_prob, fn.switch_prob, fn.label_smoothing, fn.num_classes,
            fn.correct_lam) == (0.8, 1.0, 1.0, 0.5, 0.1, 174, True)
    cfg.MIXUP.PROB, cfg.MIXUP.CUTMIX_ALPHA = 0.25, 0.0
    fn = mixup.build_mixup(cfg)
    assert fn.mix_prob == 0.25 and fn.cutmix_alpha == 0.0


def test_out_of_scope_is_refused_loudly():
    with pytest.raises(NotImplementedError):
        mixup.MixUp(num_classes={"noun": 300, "verb": 97})
    with pytest.raises(NotImplementedError):
        mixup.MixUp(num_classes=5)(torch.zeros(2, 3, 1, 4, 4), {"noun": torch.tensor([0, 1])})
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    fn = losses.VideoImageLoss(cfg, is_video_rank=False)          # an image rank, training
    with pytest.raises(NotImplementedError):
        fn(torch.randn(2, 174), {}, torch.full((2, 174), 1 / 174.0), {})


def test_soft_targets_through_video_image_loss_on_the_host(gold):
    """float [B,C] targets and MixedLabels go through VideoImageLoss / losses.cross_entropy and match F.cross_entropy on
    the dense target, value and gradient; int64 labels are untouched."""
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    fn = losses.VideoImageLoss(cfg)
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(4, 174, generator=g, requires_grad=True)
    labels = torch.from_numpy(gold["labels"])
    np.random.seed(0)
    _, mixed = _fn(gold, 0).mix(torch.zeros(4, 1, 1, 16, 16), labels)
    dense = mixed.dense()
    assert np.array_equal(dense.numpy(), gold["target"][0, 0])
    ref = F.cross_entropy(logits, dense)
    (gref,) = torch.autograd.grad(ref, logits)
    for y in (dense, mixed):
        d = fn(logits, {}, y, {})
        assert set(d) == {"loss_ce"}
        assert float(d["loss_ce"]) == float(ref)
        (gy,) = torch.autograd.grad(fn.total(d), logits)
        assert torch.equal(gy, gref)
    d = fn(logits, {}, labels, {})
    assert float(d["loss_ce"]) == float(F.cross_entropy(logits, labels))
    assert float(losses.VideoImageLoss(cfg, reduction="sum")(logits, {}, mixed, {})["loss_ce"]) == pytest.approx(
        float(F.cross_entropy(logits, dense, reduction="sum")))


def test_abi_names_are_bound():
    from svit_amd import hip
    for name in ("svit_mixup_clips", "svit_im2col_patch_u8_mix", "svit_ce_loss_soft"):
        assert name in hip.EXPORTS


def test_argument_validation_without_gpu():
    """host-side checks of the three entry points reject bad calls before any launch"""
    import __graft_entry__
    __graft_entry__.build()
    from svit_amd import hip
    lib = hip.load()
    assert lib.svit_mixup_clips(None, 16, 2, 6, 8, 8, None) == -4
    assert lib.svit_mixup_clips(16, None, 2, 6, 8, 8, None) == -4
    assert lib.svit_mixup_clips(16, 16, 0, 6, 8, 8, None) == -2
    assert lib.svit_mixup_clips(16, 16, 2, 1 << 20, 1 << 10, 1 << 10, None) == -2      # clip of 2^40 elements
    assert lib.svit_mixup_clips(18, 16, 2, 6, 8, 8, None) == -3
    assert lib.svit_im2col_patch_u8_mix(16, 1 << 20, 16, None, None, 16, 2, 4, 64, 64, 64, None) == -4
    assert lib.svit_im2col_patch_u8_mix(16, 1 << 20, 16, None, 16, 16, 2, 4, 64, 64, 80, None) == -2
    assert lib.svit_im2col_patch_u8_mix(16, 100, 16, None, 16, 16, 2, 4, 64, 64, 64, None) == -2   # buffer < one video
    assert lib.svit_ce_loss_soft(16, None, None, None, 1.0, 0.0, 2, 5, 16, 16, None) == -4      # neither target nor labels
    assert lib.svit_ce_loss_soft(16, 16, 16, None, 1.0, 0.0, 2, 5, 16, 16, None) == -4          # both
    assert lib.svit_ce_loss_soft(16, 16, None, 16, 1.0, 0.0, 2, 5, 16, 16, None) == -4          # dense + record
    assert lib.svit_ce_loss_soft(16, None, 16, None, 1.0, 0.0, 0, 5, 16, 16, None) == -2
