"""cfg.MIXUP on the device (svit_amd/mixup.py): the three kernels that read the 32-byte mix record -- svit_mixup_clips,
svit_im2col_patch_u8_mix, svit_ce_loss_soft -- against exact references, then the model step and the replayed HIP graph
against the eager step on a torch-mixed clone with the dense target and F.cross_entropy.  Needs a real MI355X."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import smoke_impl as S

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from svit_amd import hip
    from svit_amd import ops as o
    hip.load()
    return o


def _rec(mode, lam, box=(0, 0, 0, 0)):
    from svit_amd.mixup import MixRecord
    return MixRecord(mode, lam, *box)


def _dev(rec):
    return torch.from_numpy(rec.pack()).to(DEV)


def _np_mixed(x, rec):
    """the CPU formula in numpy fp32 (bit-equal to the reference's mul_/add_ sequence, tests/test_mixup_cpu.py)"""
    x = x.copy()
    if rec.mode == 1:
        return (x * np.float32(rec.lam)) + (x[::-1] * np.float32(1.0 - rec.lam))
    if rec.mode == 2:
        yl, yh, xl, xh = rec.box
        x[..., yl:yh, xl:xh] = x[::-1][..., yl:yh, xl:xh].copy()
    return x


def _torch_mixed(x, rec):
    """what the reference does to a host tensor (a copy is mixed)"""
    x = x.detach().cpu().clone()
    if rec.mode == 1:
        partner = x.flip(0).mul_(1.0 - rec.lam)
        x.mul_(rec.lam).add_(partner)
    elif rec.mode == 2:
        yl, yh, xl, xh = rec.box
        x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]
    return x


def _boxes(H, W):
    return [(0, 5, 3, 9), (H - 4, H, 2, 7), (2, 6, 0, 5), (3, 8, W - 5, W), (4, 4, 2, 9), (2, 9, 5, 5),
            (0, H, 0, W), (1, H - 1, 1, W - 1), (1, 2, 1, 2)]


# ------------------------------------------------------------------------------------------ 1. the clip kernel ----
@pytest.mark.parametrize("B", [2, 3, 8])
@pytest.mark.parametrize("H,W,offset", [(16, 16, 0), (12, 18, 0), (10, 15, 0), (16, 16, 1)])
def test_mixup_clips_bit_equal_to_the_cpu_formula(ops, B, H, W, offset):
    """modes 0 / 1 / 2, even and odd B (the middle clip blends with itself), widths that are and are not multiples
    of 4, an unaligned base (scalar path on a vector-friendly width), boxes on every border, empty and full frame"""
    shape = (B, 3, 2, H, W)
    n = int(np.prod(shape))
    x0 = P.tensor("mix:clips:%d:%d:%d" % (B, H, W), shape, 1.7).numpy()
    recs = [_rec(0, 1.0), _rec(1, 0.3), _rec(1, 0.7316), _rec(1, 1e-3)] + [_rec(2, 0.5, b) for b in _boxes(H, W)]
    for rec in recs:
        buf = torch.zeros(n + 8, device=DEV)
        x = buf[offset:offset + n].view(shape)
        assert x.data_ptr() % 16 == (4 * offset) % 16
        x.copy_(torch.from_numpy(x0))
        guard = buf.clone()
        out = ops.mixup_clips(x, _dev(rec))
        torch.cuda.synchronize()
        assert out is x
        want = _np_mixed(x0, rec)
        got = x.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (rec, int((got != want).sum()))
        assert np.array_equal(want.view(np.int32), _torch_mixed(torch.from_numpy(x0), rec).numpy().view(np.int32))
        if rec.mode == 0:
            assert np.array_equal(got.view(np.int32), x0.view(np.int32))           # bit-unchanged
        # nothing outside the tensor was written
        assert torch.equal(buf[:offset], guard[:offset]) and torch.equal(buf[offset + n:], guard[offset + n:])
    if B == 3:
        mid = _np_mixed(x0, recs[1])[1]
        assert not np.array_equal(mid, x0[1])               # x*lam + x*oml is not x in fp32: the middle clip is not skipped


def test_mixup_clips_through_the_reference_call(ops):
    """MixUp.__call__ / MixUp.mix on a device tensor: the same bits as on the host copy, after the same seed"""
    from svit_amd import mixup
    fn = mixup.MixUp(0.8, 1.0, num_classes=174)
    y = torch.tensor([3, 171, 42, 3])
    x0 = P.frames(4, 2, 32)
    for seed in range(6):
        np.random.seed(seed)
        xh, th = fn(x0.clone(), y)
        np.random.seed(seed)
        xd, td = fn(x0.clone().cuda(), y.cuda())
        assert torch.equal(xd.cpu(), xh) and torch.equal(td.cpu(), th)
        np.random.seed(seed)
        xf, mixed = fn.mix(x0.clone().cuda(), y.cuda())
        assert torch.equal(xf.cpu(), xh) and torch.equal(mixed.dense().cpu(), th)


# ----------------------------------------------------------------------------------------- 2. the uint8 route ----
def _ref_normalize(u8, mean, std):
    """slowfast/datasets/utils.py:287-303 (tensor_normalize), then T H W C -> C T H W."""
    t = u8.float()
    t = t / 255.0
    t = t - torch.tensor(mean)
    t = t / torch.tensor(std)
    return t.permute(0, 4, 1, 2, 3).contiguous()        # [V,3,T,H,W]


@pytest.mark.parametrize("V,T,Hs,Ws,S,table,boxes", [
    # partners (0,3) and (1,2) differ in source video and in x0 mod 4 (5 / 26, 29 / 0)
    (3, 4, 70, 93, 64, [(0, 3, 5), (1, 0, 29), (2, 6, 0), (1, 6, 26)], [(5, 40, 3, 61), (0, 64, 0, 64), (7, 7, 1, 9)]),
    (2, 3, 41, 59, 37, [(0, 4, 22), (1, 1, 0), (0, 0, 7)], [(0, 9, 30, 37), (20, 37, 0, 5)]),     # odd B, odd sizes
    (2, 2, 312, 415, 312, [(0, 0, 0), (1, 0, 103)], [(3, 300, 100, 290)]),                        # two chunks per row
])
def test_im2col_patch_u8_mix_bit_equal_to_the_fp32_route(ops, V, T, Hs, Ws, S, table, boxes):
    from svit_amd.input import U8Clips
    g = torch.Generator().manual_seed(V * 1000 + S)
    u8 = torch.randint(0, 256, (V, T, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    mean, std = [0.45, 0.40, 0.5], [0.225, 0.25, 0.2]
    clips = U8Clips(u8.cuda(), S, torch.tensor(table, dtype=torch.int32), mean=mean, std=std)
    plain, thw = ops.im2col_patch_u8(clips)
    f32 = _ref_normalize(u8, mean, std)
    crops = torch.stack([f32[v, :, :, y:y + S, x:x + S] for v, y, x in table]).contiguous()
    assert torch.equal(clips.lut_f32.to(torch.bfloat16).view(torch.int16), clips.lut.view(torch.int16))
    recs = [_rec(0, 1.0), _rec(1, 0.3), _rec(1, 0.8125)] + [_rec(2, 0.5, b) for b in boxes]
    for rec in recs:
        clips.mix = _dev(rec)
        cols, thw2 = ops.im2col_patch_u8(clips)
        ref_cols, ref_thw = ops.im2col_patch(_torch_mixed(crops, rec).cuda().contiguous())
        torch.cuda.synchronize()
        assert thw2 == ref_thw == thw
        assert torch.equal(cols.view(torch.int16), ref_cols.view(torch.int16)), rec
        if rec.mode == 0:
            assert torch.equal(cols.view(torch.int16), plain.view(torch.int16))
        else:
            assert not torch.equal(cols.view(torch.int16), plain.view(torch.int16)) or rec.box[0] == rec.box[1]
    clips.mix = None
    again, _ = ops.im2col_patch_u8(clips)
    assert torch.equal(again.view(torch.int16), plain.view(torch.int16))


# --------------------------------------------------------------------------------------------- 3. the loss ----
def _rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def _ce64(x, t):
    """float64 CPU reference: loss = (1/B) sum_b sum_c t (lse_b - x_bc), grad = (softmax * sum_c t - t) / B"""
    x, t = x.double().cpu(), t.double().cpu()
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    loss = (t * (lse - x)).sum() / x.shape[0]
    grad = (torch.softmax(x, dim=1) * t.sum(1, keepdim=True) - t) / x.shape[0]
    return float(loss), grad


def _target64(y, C, lam, oml, on, off, partner=None):
    y = y.cpu()
    t1 = torch.full((len(y), C), off, dtype=torch.float64).scatter_(1, y.view(-1, 1), on)
    y2 = y.flip(0) if partner is None else partner
    t2 = torch.full((len(y), C), off, dtype=torch.float64).scatter_(1, y2.view(-1, 1), on)
    return t1 * lam + t2 * oml


@pytest.mark.parametrize("B", [2, 8, 9])
@pytest.mark.parametrize("C", [174, 5])
def test_ce_loss_soft(ops, B, C, capsys):
    """svit_ce_loss_soft, dense and fused, against a float64 CPU computation.  The bar is 4 x the error of torch's own fp32
    F.cross_entropy (CPU, probability targets) against the same float64 reference on the same inputs -- both are fp32 sums
    over C terms in different orders -- with the floors of test_ce_loss_fused (2e-6 relative on the loss, 1e-5 rel_err on
    the gradient).  Three mutants (no smoothing; lam and oml swapped; partner = the row itself) must each move the loss
    by more than 100 x the bar.  The test prints every measured error, yardstick, bar and ratio.
    Measured on an MI355X over the six (B, C) cases: torch's own fp32 error is at most 1.3e-7 on the loss and 1.3e-7 on
    the gradient, so the floors decide both bars (2e-6, 1e-5); worst kernel error / bar = 0.058 on the loss (1.2e-7, B = 8,
    C = 174) and 0.008 on the gradient (8.3e-8, B = 9, C = 5), dense and fused alike; the weakest mutant (no smoothing,
    B = 9, C = 5) moves the loss by 1086 bars."""
    from svit_amd import losses, mixup
    lam, smoothing = 0.3, 0.1
    rec = _rec(1, lam)
    on, off = mixup.smoothed_one_hot_values(smoothing, C)
    x = P.tensor("mix:ce:%d:%d" % (B, C), (B, C), 3.0).to(DEV)
    y = torch.empty(B, dtype=torch.int64)
    for b in range((B + 1) // 2):
        y[b], y[B - 1 - b] = (2 * b) % C, (2 * b + 1) % C
    assert all(int(y[b]) != int(y[B - 1 - b]) for b in range(B // 2))
    mixed = mixup.MixedLabels(y.to(DEV), _dev(rec), on, off, C)
    dense = mixed.dense()
    oml = float(np.float32(1.0 - lam))
    assert _rel_err(dense, _target64(y, C, float(np.float32(lam)), oml, float(np.float32(on)), float(np.float32(off)))) < 2e-7

    ref_loss, ref_grad = _ce64(x, dense)
    # torch's own fp32 op against the float64 reference: the yardstick
    xc = x.cpu().clone().requires_grad_(True)
    t_loss = F.cross_entropy(xc, dense.cpu())
    t_loss.backward()
    torch_loss_err = abs(float(t_loss) - ref_loss) / max(1.0, abs(ref_loss))
    torch_grad_err = _rel_err(xc.grad, ref_grad)
    bar_loss, bar_grad = max(4 * torch_loss_err, 2e-6), max(4 * torch_grad_err, 1e-5)

    results = {}
    for name, kw in (("dense", dict(target=dense)), ("fused", dict(labels=mixed.labels, mix=mixed.record, on=on, off=off))):
        loss, dl = ops.ce_loss_soft(x, **kw)
        torch.cuda.synchronize()
        e_loss = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))
        e_grad = _rel_err(dl, ref_grad)
        results[name] = (float(loss), dl)
        with capsys.disabled():
            print("\n[ce_loss_soft B=%d C=%d %s] loss err %.3g (torch fp32 %.3g, bar %.3g, ratio %.3f) | grad rel_err %.3g "
                  "(torch fp32 %.3g, bar %.3g, ratio %.3f)" % (B, C, name, e_loss, torch_loss_err, bar_loss, e_loss / bar_loss,
                                                                e_grad, torch_grad_err, bar_grad, e_grad / bar_grad))
        assert e_loss <= bar_loss, (name, e_loss, bar_loss)
        assert e_grad <= bar_grad, (name, e_grad, bar_grad)
    # fused == dense on MixedLabels.dense(), within the same bar
    assert abs(results["fused"][0] - results["dense"][0]) <= bar_loss * max(1.0, abs(ref_loss))
    assert _rel_err(results["fused"][1], results["dense"][1]) <= bar_grad

    # the bar cannot hide a wrong target: each mutant moves the float64 loss by more than 100 bars
    lam32, on32, off32 = float(np.float32(lam)), float(np.float32(on)), float(np.float32(off))
    mutants = {"no smoothing": _target64(y, C, lam32, oml, 1.0, 0.0),
               "lam and oml swapped": _target64(y, C, oml, lam32, on32, off32),
               "partner = the row itself": _target64(y, C, lam32, oml, on32, off32, partner=y)}
    for name, t in mutants.items():
        moved = abs(_ce64(x, t)[0] - ref_loss) / max(1.0, abs(ref_loss))
        with capsys.disabled():
            print("[ce_loss_soft B=%d C=%d] mutant '%s' moves the loss by %.3g = %.0f bars" % (B, C, name, moved, moved / bar_loss))
        assert moved > 100 * bar_loss, (name, moved, bar_loss)

    # mix == NULL means lam = 1: the smoothed one-hot target of the row's own label
    loss1, dl1 = ops.ce_loss_soft(x, labels=mixed.labels, on=on, off=off)
    l1, g1 = _ce64(x, _target64(y, C, 1.0, 0.0, on32, off32))
    assert abs(float(loss1) - l1) <= bar_loss * max(1.0, abs(l1)) and _rel_err(dl1, g1) <= bar_grad

    # a dense target whose rows do not sum to 1: the sum_c t factor of the gradient
    scale = torch.linspace(0.4, 1.9, B, device=DEV).view(B, 1)
    odd = (dense * scale).contiguous()
    l2, g2 = _ce64(x, odd)
    xo = x.cpu().clone().requires_grad_(True)
    lo = F.cross_entropy(xo, odd.cpu())
    lo.backward()
    bl = max(4 * abs(float(lo) - l2) / max(1.0, abs(l2)), 2e-6)
    bg = max(4 * _rel_err(xo.grad, g2), 1e-5)
    loss2, dl2 = ops.ce_loss_soft(x, target=odd)
    assert abs(float(loss2) - l2) <= bl * max(1.0, abs(l2)) and _rel_err(dl2, g2) <= bg

    # through losses.cross_entropy with an upstream gradient other than 1, both kinds of label
    for lab in (dense, mixed):
        xg = x.clone().requires_grad_(True)
        out = losses.cross_entropy(xg, lab)
        (out * 0.37).backward()
        assert abs(float(out) - ref_loss) <= bar_loss * max(1.0, abs(ref_loss))
        assert _rel_err(xg.grad, ref_grad * 0.37) <= bar_grad
    # a label outside [0, C) poisons the loss, whichever side of the pair it is on
    for pos in (0, B - 1):
        bad = y.clone()
        bad[pos] = C
        assert bool(torch.isnan(ops.ce_loss_soft(x, labels=bad.to(DEV), mix=mixed.record, on=on, off=off)[0]))
    bad = y.clone()
    bad[0] = -100                                        # there is no ignore index
    assert bool(torch.isnan(ops.ce_loss_soft(x, labels=bad.to(DEV), mix=mixed.record, on=on, off=off)[0]))


# --------------------------------------------------------------------------------- 4. / 5. model step and graph ----
RECORDS = [(0, 1.0, (0, 0, 0, 0)), (1, 0.3, (0, 0, 0, 0)), (2, 1.0 - 30 * 40 / 4096.0, (10, 40, 0, 40)),
           (1, 0.8125, (0, 0, 0, 0)), (2, 1.0, (20, 20, 5, 9)), (2, 0.0, (0, 64, 0, 64))]


def _mixup_fn():
    from svit_amd import mixup
    return mixup.MixUp(0.8, 1.0, label_smoothing=0.1, num_classes=174)


def _dense(y, rec):
    from svit_amd import mixup
    on, off = mixup.smoothed_one_hot_values(0.1, 174)
    return mixup.dense_target(y, 174, rec.lam, 1.0 - rec.lam, on, off)


def _eager_ref(model, x, y, rec, frames_loss=None):
    """the reference's step: the clip mixed by torch ops on a clone, the dense target, F.cross_entropy"""
    xm = _torch_mixed(x, rec).cuda()
    model.flat.grad.zero_()
    logits, extra = model([xm], {})
    loss = F.cross_entropy(logits, _dense(y, rec))
    if frames_loss is not None:
        loss = loss + frames_loss(model, xm, extra)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), logits.detach().clone(), model.flat.grad.clone()


def _assert_step(got_loss, got_logits, got_grad, ref, noise):
    """the bars of tests/test_graph_gpu.py::test_graphed_step_equals_eager_step, its measured eager-noise term included"""
    assert abs(float(got_loss) - ref[0]) < 1e-4 * max(1.0, abs(ref[0]))
    assert float((got_logits - ref[1]).abs().max()) < 1e-4
    assert S.cosine(got_grad, ref[2]) > 0.99999
    assert float((got_grad - ref[2]).abs().max()) <= max(4 * noise, 2e-3 * float(ref[2].abs().max()))


def _noise(model, x, y, rec):
    a = _eager_ref(model, x, y, rec)
    b = _eager_ref(model, x, y, rec)
    return float((a[2] - b[2]).abs().max())


def test_model_step_device_route_equals_torch_mixed_eager_step():
    """MixUp.mix (clip kernel + MixedLabels) + VideoImageLoss against the eager step on a torch-mixed clone with the dense
    target and F.cross_entropy: loss, logits, flat gradient"""
    from svit_amd import losses
    cfg, model, spec, sd = S.build_hip_model(4, 64)
    fn, loss_mod = _mixup_fn(), losses.VideoImageLoss(cfg)
    x, y = P.frames(2, 4, 64).cuda(), P.labels(2).cuda()
    noise = _noise(model, x, y, _rec(*RECORDS[1]))
    for r in RECORDS:
        rec = _rec(*r)
        ref = _eager_ref(model, x, y, rec)
        xd = x.clone()
        xd, mixed = fn.mix(xd, y, record=rec)
        assert torch.equal(xd.cpu(), _torch_mixed(x, rec))
        model.flat.grad.zero_()
        logits, extra = model([xd], {})
        d = loss_mod(logits, extra, mixed, {})
        loss = loss_mod.total(d)
        loss.backward()
        torch.cuda.synchronize()
        _assert_step(loss, logits.detach(), model.flat.grad, ref, noise)


def test_graph_replay_reads_the_record_at_replay_time():
    """one capture, six records covering every mode: each replay equals the eager reference for its record; the same batch
    under another record gives another loss (the record is read at replay time, not baked in at capture); mixup=None
    captures what it always captured"""
    from svit_amd import hip, losses
    from svit_amd.graph import GraphedTrainStep
    cfg, model, spec, sd = S.build_hip_model(4, 64)
    fn, loss_mod = _mixup_fn(), losses.VideoImageLoss(cfg)
    x, y = P.frames(2, 4, 64).cuda(), P.labels(2).cuda()
    x2, y2 = (x.flip(0) * 0.5 + 0.1).contiguous(), (y + 3) % 174

    def loss_fun(preds, extra, labels):
        return loss_mod.total(loss_mod(preds, extra, labels, {}))

    recs = [_rec(*r) for r in RECORDS]
    noise = _noise(model, x, y, recs[1])
    refs = [_eager_ref(model, x, y, rec) for rec in recs]
    refs2 = [_eager_ref(model, x2, y2, rec) for rec in recs]
    plain_ref = None
    model.flat.grad.zero_()
    logits, _ = model([x], {})
    pl = F.cross_entropy(logits, y)
    pl.backward()
    torch.cuda.synchronize()
    plain_ref = (float(pl), logits.detach().clone(), model.flat.grad.clone())

    step = GraphedTrainStep(model, loss_fun, [x], y, mixup=fn)
    losses_seen = []
    for _ in range(2):
        for i, rec in enumerate(recs):
            loss, (logits, extra) = step([x], y, mix=rec)
            torch.cuda.synchronize()
            _assert_step(loss, logits, model.flat.grad, refs[i], noise)
            losses_seen.append(float(loss))
            loss, (logits, extra) = step([x2], y2, mix=rec)
            torch.cuda.synchronize()
            _assert_step(loss, logits, model.flat.grad, refs2[i], noise)
    assert abs(losses_seen[1] - losses_seen[3]) > 1e-3 and abs(losses_seen[1] - losses_seen[2]) > 1e-3
    # the static input was mixed where it lies, as the reference mutates its input
    loss, _ = step([x], y, mix=recs[1])
    torch.cuda.synchronize()
    assert torch.equal(step.static_inputs[0].cpu(), _torch_mixed(x, recs[1])) and not torch.equal(step.static_inputs[0], x)
    # no record passed: one is drawn from np.random, as the reference's call would
    np.random.seed(4)
    want = fn.draw(x.shape)
    np.random.seed(4)
    loss, (logits, _) = step([x], y)
    torch.cuda.synchronize()
    _assert_step(loss, logits, model.flat.grad, _eager_ref(model, x, y, want), noise)

    plain = GraphedTrainStep(model, lambda p, e, l: losses.cross_entropy(p, l), [x], y)
    assert plain.n_graphs == step.n_graphs and plain.mix_record is None
    loss, (logits, _) = plain([x], y)
    torch.cuda.synchronize()
    _assert_step(loss, logits, model.flat.grad, plain_ref, noise)
    with pytest.raises(hip.SvitHipError):
        plain([x], y, mix=recs[1])


def test_graph_replay_with_frames_pass_sees_the_mixed_clip():
    """frames_pass=True: the no-grad single-frame pass inside the replayed step runs on the MIXED clip, as in the reference
    (tools/train_net.py:92-110 mixes inputs[0] first).  The eager reference does so on the torch-mixed clone; a frames pass
    on the unmixed clip would miss the loss bar by far (asserted), so matching the reference proves which clip it saw."""
    from svit_amd import losses
    from svit_amd.graph import GraphedTrainStep
    cfg, model, spec, sd = S.build_hip_model(4, 64)
    cfg.SVIT.CONSISTENCY = "l1"
    fn, loss_mod = _mixup_fn(), losses.VideoImageLoss(cfg)
    x, y = P.frames(2, 4, 64).cuda(), P.labels(2).cuda()

    def loss_fun(preds, extra, labels):
        return loss_mod.total(loss_mod(preds, extra, labels, {}))

    def consistency(frames_of):
        def term(model, xm, extra):
            src = xm if frames_of is None else frames_of
            with torch.no_grad():
                fp, fe = model([src.transpose(1, 2).flatten(0, 1).unsqueeze(2)], {})
            tar = fe["obj_desc"].reshape(extra["obj_desc"].shape).detach()
            return cfg.SVIT.LAMBDA_CON * F.l1_loss(extra["obj_desc"], tar)
        return term

    recs = [_rec(1, 0.3), _rec(*RECORDS[2])]
    refs = [_eager_ref(model, x, y, rec, consistency(None)) for rec in recs]
    wrong = [_eager_ref(model, x, y, rec, consistency(x)) for rec in recs]        # frames pass on the unmixed clip
    for r, w in zip(refs, wrong):
        assert abs(r[0] - w[0]) > 10 * 1e-4 * max(1.0, abs(r[0]))
    step = GraphedTrainStep(model, loss_fun, [x], y, frames_pass=True, mixup=fn)
    for _ in range(2):
        for rec, ref in zip(recs, refs):
            loss, (logits, extra) = step([x], y, mix=rec)
            torch.cuda.synchronize()
            assert abs(float(loss) - ref[0]) < 1e-4 * max(1.0, abs(ref[0]))
            assert float((logits - ref[1]).abs().max()) < 1e-4
            assert S.cosine(model.flat.grad, ref[2]) > 0.99999


def test_graph_replay_with_u8_clips():
    """The U8Clips route under replay, on the clip content the other model-level tests use: P.frames, quantised to the
    uint8 video the decoder would have delivered.  Against the eager reference with the bars of
    test_graphed_step_equals_eager_step, and against the fp32 replay of the same normalised crops (the im2col operand is
    bit-equal, so the two replays may differ by the eager noise only).
    Measured on an MI355X with uniform random BYTES as frames instead (white noise, |x| up to 2.44): the u8 and the fp32
    replay agree to 4.5e-8, both differ from the eager reference by 2.4e-3 x max|g| (bar 2e-3; cosine 0.999991) for the
    records whose lambda is 1, 0 or 0.8125 and by 3e-8 for the other two -- last-bit differences between torch's soft-target
    cross-entropy backward and svit_ce_loss_soft (each 5-8e-8 from float64, test_ce_loss_soft), amplified by the bf16
    backward; nothing of the uint8 route."""
    from svit_amd import losses
    from svit_amd.graph import GraphedTrainStep
    from svit_amd.input import U8Clips
    cfg, model, spec, sd = S.build_hip_model(4, 64)
    fn, loss_mod = _mixup_fn(), losses.VideoImageLoss(cfg)
    mean, std = (0.45, 0.45, 0.45), (0.225, 0.225, 0.225)
    video = P.frames(3, 4, 96)                                   # [V,3,T,96,96], |x| <= 1.7 -> bytes in [17, 212]
    u8 = ((video * 0.225 + 0.45) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()
    table = [(0, 3, 5), (2, 6, 26)]
    clips = U8Clips(u8.cuda(), 64, torch.tensor(table, dtype=torch.int32), mean=mean, std=std)
    f32 = _ref_normalize(u8, list(mean), list(std))
    x = torch.stack([f32[v, :, :, yy:yy + 64, xx:xx + 64] for v, yy, xx in table]).contiguous().cuda()
    y = P.labels(2).cuda()

    def loss_fun(preds, extra, labels):
        return loss_mod.total(loss_mod(preds, extra, labels, {}))

    recs = [_rec(*r) for r in RECORDS]
    noise = _noise(model, x, y, recs[1])
    refs = [_eager_ref(model, x, y, rec) for rec in recs]
    step = GraphedTrainStep(model, loss_fun, [clips], y, mixup=fn)
    step32 = GraphedTrainStep(model, loss_fun, [x], y, mixup=fn)
    for i, rec in enumerate(recs):
        loss, (logits, extra) = step([clips], y, mix=rec)
        torch.cuda.synchronize()
        _assert_step(loss, logits, model.flat.grad, refs[i], noise)
        got = (float(loss), logits.clone(), model.flat.grad.clone())
        loss, (logits, extra) = step32([x], y, mix=rec)
        torch.cuda.synchronize()
        _assert_step(loss, logits, model.flat.grad, got, noise)
        assert float((model.flat.grad - got[2]).abs().max()) <= max(4 * noise, 1e-6 * float(got[2].abs().max()))
    assert clips.mix is None                                   # the caller's clips are not tagged: the step's copy is
    # eager: MixUp.mix tags the clips, the model's im2col mixes
    _, mixed = fn.mix(clips, y, record=recs[1])
    model.flat.grad.zero_()
    logits, extra = model([clips], {})
    loss = loss_mod.total(loss_mod(logits, extra, mixed, {}))
    loss.backward()
    torch.cuda.synchronize()
    _assert_step(loss, logits.detach(), model.flat.grad, refs[1], noise)
