"""Captured evaluation steps on the uint8 route, on the device: the eval-mode head in one launch (svit_head_eval) against
its float64 restatement, graph.GraphedEvalStep against its eager twin and against today's fp32 route, the test
ensemble's fold and the validation meter's push inside the replay, and the two loops fed by feeder.ClipFeeder.

Tiny configuration of tests/smoke_impl.py: 4 frames, S = 64 (final width 768, 174 classes, O = 4).  The head's bar is
tests/eval_u8_cases.py's: 4 x the error of the stock ATen eval head on the same device and inputs, floored at 2^-24."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import eval_u8_cases as EC
from tests import smoke_impl as SM

TIMING = ("time_diff", "eta", "mem", "gpu_mem", "RAM")
CANARY = 64
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def net():
    import __graft_entry__
    __graft_entry__.build()
    cfg, model, _, _ = SM.build_hip_model(4, 64, train=False)
    cfg.LOG_PERIOD = 2
    cfg.TRAIN.FORWARD_VIDEO_FRAMES = True
    cfg.SVIT.CONSISTENCY = "l2"
    cfg.TEST.NUM_ENSEMBLE_VIEWS = 2
    return cfg, model


# --------------------------------------------------------------------------------------------------- 1. the kernel ----
def guarded(shape, fill=-7.0):
    """an f32 tensor of `shape` between two 64-byte canaries -> (tensor, check())"""
    n = int(np.prod(shape)) * 4
    pad = (-n) % 16
    raw = torch.full((n + pad + 2 * CANARY,), 0x5C, dtype=torch.uint8, device="cuda")
    t = raw[CANARY:CANARY + n].view(torch.float32).view(shape)
    t.fill_(fill)

    def check():
        assert bool((raw[:CANARY] == 0x5C).all()) and bool((raw[CANARY + n:] == 0x5C).all()), "canary overwritten"
    return t, check


def head_args(tokens, params, T, O, outs):
    from svit_amd import ops
    return ops._head_args(tokens, T, O, None, params, outs)


def device_case(B, N, Cw, T, O, n_cls, seed):
    tokens, params = EC.make_case(B, N, Cw, T, O, n_cls, seed)
    dev = (torch.from_numpy(tokens).cuda(), [(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()) for w, b in params])
    return tokens, params, dev


@pytest.mark.parametrize("n_cls", [1, 5, 174])
@pytest.mark.parametrize("Cw", [100, 768])
def test_head_eval_against_float64(net, Cw, n_cls):
    """T in {1, 2}, both activations, N = 1 + 7 + T*O and the smallest legal N = 1 + T*O; B = 3 (cls blocks and more
    than one object block: 3 * 2 * 4 = 24 rows over blocks of 8); C = 768 is the model's final width, C = 100 a width
    whose last 256-channel step is partial.  The batch carries a +120 class logit and a +120 contact logit, and class,
    objectness and box logits of -800 (eval_u8_cases.make_case): a sigmoid whose exp overflows must give 0, not NaN."""
    from svit_amd import hip
    from svit_amd.evaluate import head_eval_host
    B, O = 3, 4
    worst = 0.0
    for T in (1, 2):
        for N in (1 + 7 + T * O, 1 + T * O):
            tokens, params, (tok_d, par_d) = device_case(B, N, Cw, T, O, n_cls, seed=100 * T + N)
            for act in (0, 1):
                outs, checks = zip(*[guarded(s) for s in ((B, n_cls), (B, T, O, 5), (B, T, 2, 5), (B, T, O, Cw))])
                a = head_args(tok_d, par_d, T, O, outs)
                hip.call("svit_head_eval", C.byref(a), act)
                torch.cuda.synchronize()
                for chk in checks:
                    chk()
                want64 = head_eval_host(tokens, params, T, O, act)
                yard = EC.errors(EC.aten_head(tokens, params, T, O, act, device="cuda"), want64)
                bars = EC.bar(yard)
                err = EC.errors(outs, want64)
                ratio = max(e / max(y, EC.FLOOR / 4) for e, y in zip(err, yard))
                worst = max(worst, ratio)
                print("C %d n_cls %d T %d N %d act %d: error %s, ATen %s, ratio %.2f" % (Cw, n_cls, T, N, act, err, yard, ratio))
                assert all(e <= b for e, b in zip(err, bars)), (T, N, act, err, bars)
                assert torch.equal(outs[3], tok_d[:, N - T * O:].reshape(B, T, O, Cw))
                rows = [outs[2].double().sum(-1)] + ([outs[0].double().sum(-1)] if act == 0 else [])
                for s in rows:                          # softmax rows sum to 1 within 4 ulp of fp32
                    assert float((s - 1.0).abs().max()) <= 4 * ULP, float((s - 1.0).abs().max())
                if act == 0:
                    assert float(outs[0][B - 1, 0]) == 1.0                  # the +120 row
                assert all(bool(torch.isfinite(o).all()) for o in outs)
                assert EC.cold_outputs(outs, n_cls, act) == [0.0] * (3 if act == 1 else 2)       # the -800 rows
                for name in EC.MUTANTS:
                    if name == "cls_from_row_1" and n_cls == 1 and act == 0:
                        continue                        # (a softmax over one class is 1 whatever row it reads)
                    assert EC.caught(name, tokens, params, T, O, act, want64, bars) >= 10.0, (name, T, N, act)
                # without xobj: the same three outputs
                outs2 = [torch.empty_like(o) for o in outs[:3]] + [None]
                hip.call("svit_head_eval", C.byref(head_args(tok_d, par_d, T, O, outs2)), act)
                assert all(torch.equal(p, q) for p, q in zip(outs[:3], outs2[:3]))
    print("svit_head_eval: worst error / ATen error over the cases of C %d, n_cls %d: %.2f" % (Cw, n_cls, worst))


def test_head_eval_refusals_launch_nothing(net):
    from svit_amd import hip
    lib = hip.load()
    B, T, O, Cw, n_cls = 2, 2, 4, 768, 174
    N = 1 + 3 + T * O
    _, _, (tok_d, par_d) = device_case(B, N, Cw, T, O, n_cls, seed=5)
    shapes = ((B, n_cls), (B, T, O, 5), (B, T, 2, 5), (B, T, O, Cw))
    outs = [torch.full(s, -7.0, device="cuda") for s in shapes]
    keep = torch.ones((B, 1 + T * O, Cw), device="cuda")

    def rc(act=0, **change):
        a = head_args(tok_d, par_d, T, O, outs)
        for k, v in change.items():
            setattr(a, k, v)
        return lib.svit_head_eval(C.byref(a), act, None)
    assert lib.svit_head_eval(None, 0, None) == -4
    assert rc(keep=keep.data_ptr()) == -4
    for field in ("tokens", "w_proj", "b_proj", "w_box", "b_box", "w_bce", "b_bce", "w_con", "b_con", "logits", "boxes",
                  "contact"):
        assert rc(**{field: None}) == -4, field
    assert rc(C=770) == -2 and rc(n_cls=0) == -2 and rc(n_cls=1025) == -2 and rc(N=T * O) == -2
    assert rc(act=2) == -2 and rc(act=-1) == -2
    # what the entry point refuses beyond that list (include/svit_hip.h): no contact objects, empty batch, misalignment
    assert rc(O=1) == -2 and rc(B=0) == -2 and rc(T=0) == -2
    for field in ("tokens", "w_proj", "w_box", "w_bce", "w_con", "xobj"):
        t = {"tokens": tok_d, "w_proj": par_d[0][0], "w_box": par_d[1][0], "w_bce": par_d[2][0], "w_con": par_d[3][0],
             "xobj": outs[3]}[field]
        assert rc(**{field: t.data_ptr() + 4}) == -3, field
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)                   # nothing was launched
    assert rc(xobj=None) == 0 and rc(n_cls=1) == 0                      # xobj alone may be NULL
    torch.cuda.synchronize()
    assert bool((outs[0][:, 0] != -7.0).all())


# ------------------------------------------------------------------------------------- 2. the step: shared pieces ----
def videos_of(sizes, seed, T=4):
    g = np.random.default_rng(seed)
    return [torch.from_numpy(g.integers(0, 256, (T, h, w, 3), dtype=np.uint8)) for h, w in sizes]


def patterned(videos, Hs, Ws):
    """the videos in the top-left corners of a u8 [V,T,Hs,Ws,3] buffer whose padding alternates 0 and 255 (never zeros
    only: a kernel that reads the padding gives other numbers)"""
    V, T = len(videos), videos[0].shape[0]
    idx = np.arange(V * T * Hs * Ws * 3).reshape(V, T, Hs, Ws, 3)
    buf = torch.from_numpy(np.where((idx // 3 + idx // 7) % 2 == 0, 0, 255).astype(np.uint8))
    for v, x in enumerate(videos):
        buf[v, :, :x.shape[1], :x.shape[2]] = x
    return buf


def clips_of(cfg, sizes, seed, Hs, Ws, num_crops, first=0):
    """-> (AugClips over a patterned Hs x Ws buffer with extents, clip ids, host videos, records)"""
    from svit_amd.augment import AugClips, build_sampler
    from svit_amd.evaluate import test_views
    vids = videos_of(sizes, seed)
    recs, ids = test_views(build_sampler(cfg, "test"), sizes, first, num_crops)
    clips = AugClips(patterned(vids, Hs, Ws).cuda(), 64, recs, cfg.DATA.MEAN, cfg.DATA.STD, extents=sizes)
    return clips, ids, vids, recs


def same(a, b):
    """bit equality of two (preds, extra) pairs, frames-pass outputs included"""
    assert torch.equal(a[0], b[0])
    assert sorted(a[1]) == sorted(b[1])
    for k, v in a[1].items():
        if k == "frames_output":
            assert torch.equal(v["preds"], b[1][k]["preds"])
            assert sorted(v["extra_preds"]) == sorted(b[1][k]["extra_preds"])
            for kk, vv in v["extra_preds"].items():
                assert torch.equal(vv, b[1][k]["extra_preds"][kk]), kk
        else:
            assert torch.equal(v, b[1][k]), k


def numbers(stats):
    return None if stats is None else {k: v for k, v in stats.items() if k not in TIMING}


# ----------------------------------------------------------------------------------------- 3. captured = eager ----
def test_captured_step_equals_its_eager_twin_bit_for_bit(net):
    """a 20 x 24 buffer, videos 20x24, 12x16 and 3x3 (the test-time rescale upsamples them to a 64 short side), two views
    per video; two further size mixes through the same capture; the frames pass on the uint8 route"""
    from svit_amd.graph import GraphedEvalStep
    cfg, model = net
    mixes = [[(20, 24), (12, 16), (3, 3)], [(3, 3), (20, 24), (12, 16)], [(16, 12), (20, 17), (9, 24)]]
    y = torch.tensor([3, 50, 7, 9, 100, 20]).cuda()
    first = clips_of(cfg, mixes[0], 1, 20, 24, 2)[0]
    before = (model.flat.data.clone(), model.flat.grad.clone(),
              None if model._rng_state is None else model._rng_state.clone())
    step = GraphedEvalStep(model, [first], y, frames_pass="u8")
    assert step.static_inputs[0] is step.x and step.static_labels is step.labels
    seen = []
    for k, sizes in enumerate(mixes):
        clips = clips_of(cfg, sizes, 10 + k, 20, 24, 2)[0]
        want = step.eager([clips_of(cfg, sizes, 10 + k, 20, 24, 2)[0]], y)
        got = step([clips], y)
        torch.cuda.synchronize()
        assert tuple(got[0].shape) == (6, 174) and tuple(got[1]["frames_output"]["preds"].shape) == (24, 174)
        assert set(got[1]) == {"obj_desc", "pred_bboxes", "pred_contact_state", "frames_output"}
        assert bool(torch.isfinite(got[0]).all())
        same(got, want)
        seen.append(got[0].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    # against the ATen head on the same tokens: the fused head inside the step is the eval head
    clips = clips_of(cfg, mixes[2], 12, 20, 24, 2)[0]
    with torch.no_grad():
        ref = model([clips], {})
    assert float((ref[0] - seen[2]).abs().max()) <= 1e-5
    after = (model.flat.data, model.flat.grad, model._rng_state)
    # (the optimizer's moments cannot move either: the step takes no optimizer and launches none of its kernels)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert (before[2] is None and after[2] is None) or torch.equal(before[2], after[2])


# ------------------------------------------------------------------------------------ 4. against today's route ----
def test_step_agrees_with_the_fp32_route_within_the_head_bar(net):
    """sources whose short side equals S (64x88, 88x64): the test-time rescale is the identity, so the step's operand is
    the fp32 route's (host-normalised video, evaluate.spatial_crops) bit for bit, and the probabilities differ by the
    two heads' rounding only"""
    from svit_amd import evaluate
    from svit_amd.graph import GraphedEvalStep
    cfg, model = net
    sizes = [(64, 88), (88, 64)]
    clips, ids, vids, recs = clips_of(cfg, sizes, 21, 88, 88, 3)
    y = torch.zeros(6, dtype=torch.int64).cuda()
    step = GraphedEvalStep(model, [clips], y)
    probs, extra = step([clips], y)
    crops = []
    for x in vids:
        t = (x.float() / 255.0 - torch.tensor(cfg.DATA.MEAN)) / torch.tensor(cfg.DATA.STD)
        crops.append(evaluate.spatial_crops(t.permute(3, 0, 1, 2)[None].contiguous().cuda(), 64, 3))
    crops = torch.cat(crops)
    with torch.no_grad():
        tok_u8 = model.engine.forward(clips, None, save=False)[0]
        tok_f32 = model.engine.forward(crops, None, save=False)[0]
        old = model([crops], {})
    assert torch.equal(tok_u8, tok_f32)
    params = [(w.detach().cpu().numpy(), b.detach().cpu().numpy()) for w, b in model.head.param_pairs()]
    want64 = evaluate.head_eval_host(tok_u8.cpu().numpy(), params, 4, 4, 0)
    yard = EC.errors((old[0], old[1]["pred_bboxes"], old[1]["pred_contact_state"]), want64)
    bars = EC.bar(yard)
    err = EC.errors((probs, extra["pred_bboxes"], extra["pred_contact_state"]), want64)
    print("step vs float64 %s, fp32 route vs float64 %s" % (err, yard))
    assert all(e <= b for e, b in zip(err, bars)), (err, bars)
    assert float((probs - old[0]).abs().max()) <= bars[0] + yard[0]


# -------------------------------------------------------------------------------------------- 5. test ensemble ----
def test_ensemble_fold_inside_the_replay(net):
    """4 videos x 3 views in two batches, every view folded twice: the meter the replays fed equals one fed eagerly"""
    from svit_amd.evaluate import TestMeter
    from svit_amd.graph import GraphedEvalStep
    cfg, model = net
    sizes = [[(20, 24), (12, 16)], [(16, 12), (20, 17)]]
    labels_v = torch.tensor([5, 17, 101, 33])
    batches = []
    for k, sz in enumerate(sizes):
        clips, ids, _, _ = clips_of(cfg, sz, 30 + k, 20, 24, 3, first=2 * k)
        batches.append((clips, {"labels": labels_v[ids // 3].cuda(), "clip_ids": ids.cuda()}))
    captured, eager = TestMeter(4, 3, 174, 2), TestMeter(4, 3, 174, 2)
    step = GraphedEvalStep(model, [batches[0][0]], batches[0][1], test_meter=captured, repeat=2)
    plain = GraphedEvalStep(model, [batches[0][0]], batches[0][1])
    assert int(captured.clip_count.sum()) == 0 and float(captured.video_preds.abs().max()) == 0     # empty after the warm-up
    for clips, tree in batches:
        step([clips], tree)
        p, _ = plain.eager([clips], tree)
        eager.update_stats(p, tree["labels"], tree["clip_ids"], repeat=2)
    torch.cuda.synchronize()
    assert captured.clip_count.tolist() == [6, 6, 6, 6]
    for name in ("video_preds", "video_labels", "clip_count", "errors"):
        assert torch.equal(getattr(captured, name), getattr(eager, name)), name
    assert captured.finalize_metrics((1, 5)) == eager.finalize_metrics((1, 5))


# ------------------------------------------------------------------------------------------------ 6. val meter ----
def _eager_twin():
    from svit_amd.graph import GraphedEvalStep

    class EagerTwin(GraphedEvalStep):
        """the same step, every call through its uncaptured body"""

        def __call__(self, inputs, labels):
            return self.eager(inputs, labels)
    return EagerTwin


def _run_val(cfg, step_cls, model, loader, first, feeder=False):
    from svit_amd import meters, train
    from svit_amd.feeder import ClipFeeder
    meter = meters.ValMeter(len(loader), cfg)
    step = step_cls(model, [first[0]], first[1], cfg=cfg, frames_pass="u8", val_meter=meter)
    assert meter.state.tolist() == [0, 0]                              # the warm-up only fixed the columns
    lines, log_iter = [], meter.log_iter_stats
    meter.log_iter_stats = lambda e, i: lines.append(numbers(log_iter(e, i)))
    fd = ClipFeeder.for_step(step) if feeder else None
    try:
        epoch = numbers(train.eval_epoch(loader, step, meter, 0, cfg, feeder=fd))
    finally:
        if fd is not None:
            fd.close()
    torch.cuda.synchronize()
    return lines, epoch, meter.ring.clone()


def test_eval_epoch_with_the_step_logs_what_the_eager_twin_logs(net):
    from svit_amd.graph import GraphedEvalStep
    cfg, model = net
    g = torch.Generator().manual_seed(4)
    loader = []
    for k, sz in enumerate([[(20, 24), (12, 16)], [(3, 3), (20, 24)], [(16, 12), (20, 17)]]):
        clips = clips_of(cfg, sz, 40 + k, 20, 24, 2)[0]
        loader.append(([clips], torch.randint(0, 174, (4,), generator=g).cuda(), None, {}))
    with torch.no_grad():                                               # one clip per batch is labelled with its best class
        for inp, lab, _, _ in loader:
            lab[0] = model(inp, {})[0].argmax(dim=1)[0]
    first = (loader[0][0][0], loader[0][1])
    a = _run_val(cfg, GraphedEvalStep, model, loader, first)
    b = _run_val(cfg, _eager_twin(), model, loader, first)
    assert [l is not None for l in a[0]] == [False, True, False]
    assert a[0] == b[0] and a[1] == b[1]
    assert "extra_meter_video_image_desc_l2_loss" in a[1] and a[1]["top1_err"] < 100.0
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))  # the ring's rows, bit for bit


# --------------------------------------------------------------------------------------------------- 7. feeder ----
def _host_batches(cfg, num_crops, labels_v):
    """2 full batches (2 videos) + 1 short one (1 video) of host videos -> [(videos, records, clip ids, video labels)]"""
    from svit_amd.augment import build_sampler
    from svit_amd.evaluate import test_views
    sampler, out, first = build_sampler(cfg, "test"), [], 0
    for k, sz in enumerate([[(20, 24), (12, 16)], [(16, 12), (20, 17)], [(9, 24)]]):
        recs, ids = test_views(sampler, sz, first, num_crops)
        out.append((videos_of(sz, 50 + k), recs, ids, labels_v[ids // num_crops]))
        first += len(sz)
    return out


def _device_batch(cfg, videos, recs):
    from svit_amd.augment import AugClips, pack_videos
    frames, ext = pack_videos(videos, 20, 24)
    return AugClips(frames.cuda(), 64, recs, cfg.DATA.MEAN, cfg.DATA.STD, extents=ext)


def test_perform_test_fed_equals_the_direct_route(net):
    from svit_amd import evaluate
    from svit_amd.feeder import ClipFeeder
    from svit_amd.graph import GraphedEvalStep
    cfg, model = net
    labels_v = torch.tensor([5, 17, 101, 33, 9])
    host = _host_batches(cfg, 2, labels_v)
    results = []
    for fed in (False, True):
        meter = evaluate.TestMeter(5, 2, 174, len(host))
        tree0 = {"labels": host[0][3].cuda(), "clip_ids": host[0][2].cuda()}
        step = GraphedEvalStep(model, [_device_batch(cfg, host[0][0], host[0][1])], tree0, test_meter=meter, repeat=2)
        if fed:
            loader = [(v, r, {"labels": lab, "clip_ids": ids}, ids, {}) for v, r, ids, lab in host]
            with ClipFeeder.for_step(step) as fd:
                evaluate.perform_test(loader, step, meter, cfg, feeder=fd)
        else:
            loader = [([_device_batch(cfg, v, r)], {"labels": lab.cuda(), "clip_ids": ids.cuda()}, ids, {})
                      for v, r, ids, lab in host]
            evaluate.perform_test(loader, step, meter, cfg)
        torch.cuda.synchronize()
        results.append(meter)
    a, b = results
    assert a.clip_count.tolist() == [4] * 5
    for name in ("video_preds", "video_labels", "clip_count", "errors"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.stats == b.stats and set(a.stats) == {"split", "top1_acc", "top5_acc"}


def test_eval_epoch_fed_equals_the_direct_route(net):
    from svit_amd.graph import GraphedEvalStep
    cfg, model = net
    labels_v = torch.tensor([5, 17, 101, 33, 9])
    host = _host_batches(cfg, 2, labels_v)
    first = (_device_batch(cfg, host[0][0], host[0][1]), host[0][3].cuda())
    direct = [([_device_batch(cfg, v, r)], lab.cuda(), None, {}) for v, r, ids, lab in host]
    fed = [(v, r, lab, None, {}) for v, r, ids, lab in host]
    a = _run_val(cfg, GraphedEvalStep, model, direct, first)
    b = _run_val(cfg, GraphedEvalStep, model, fed, first, feeder=True)
    assert [l is not None for l in a[0]] == [False, True, False]
    assert a[0] == b[0] and a[1] == b[1]
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 8. refusals ----
def test_refusals(net):
    from svit_amd import meters
    from svit_amd.graph import GraphedEvalStep
    from svit_amd.hip import SvitHipError
    cfg, model = net
    clips = clips_of(cfg, [(20, 24), (12, 16)], 60, 20, 24, 2)[0]
    y = torch.zeros(4, dtype=torch.int64).cuda()
    model.train()
    try:
        with pytest.raises(SvitHipError, match="model.eval"):
            GraphedEvalStep(model, [clips], y)
    finally:
        model.eval()
    with pytest.raises(SvitHipError, match="frames_pass=True is the fp32 route"):
        GraphedEvalStep(model, [clips], y, frames_pass=True)
    with pytest.raises(SvitHipError, match="the meter lives on"):
        GraphedEvalStep(model, [clips], y, cfg=cfg, val_meter=meters.ValMeter(3, cfg, device="cpu"))
    with pytest.raises(SvitHipError, match="needs cfg="):
        GraphedEvalStep(model, [clips], y, val_meter=meters.ValMeter(3, cfg))
    step = GraphedEvalStep(model, [clips], y)
    out = step([clips], y)[0].clone()
    with pytest.raises(SvitHipError, match="captured for a frame buffer"):
        step([clips_of(cfg, [(20, 24), (12, 16)], 60, 20, 28, 2)[0]], y)
    with pytest.raises(SvitHipError, match="captured for input"):
        step([clips_of(cfg, [(20, 24), (12, 16)], 60, 20, 24, 3)[0]], torch.zeros(6, dtype=torch.int64).cuda())
    torch.cuda.synchronize()
    assert torch.equal(step.preds, out)                                 # a refused batch enqueued nothing
