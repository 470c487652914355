"""Layer-wise lr decay on the GPU: svit_adamw_step_guarded_lr against the `_seg` kernel fed the premultiplied learning
rate, and the model under SOLVER.LAYER_DECAY / SVIT.LR_MULT -- both optimizer tails, torch.optim.AdamW, the captured
and the accumulated step, a frozen cut, a checkpoint round trip.  Bit equality unless said otherwise.  Needs a real
MI355X."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from oracle import svit_ref as R
from tests import layer_decay_cases as L

DEV = "cuda"
N = 6 * 1024 + 7                # six windows of 1024 floats, n % 4 = 3
N4 = N // 4 * 4
BETAS, EPS = (0.9, 0.999), 1e-8
LRS, WDS = (1e-3, 3e-3), (0.05, 0.01)
INEXACT = np.float32(1.0 / 3.0)
SCALES = [np.float32(1.0), np.float32(0.75 ** 17), np.float32(10.0), INEXACT]


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ===================================================================================================== kernels ====
@pytest.fixture(scope="module")
def table():
    from svit_amd import ops
    return torch.from_numpy(ops.adamw_bias_table(*BETAS)).to(DEV)


def _segs(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(-1, 2))


class Tail:
    """p, g, m, v f32 [N] + the two step records"""

    def __init__(self, table, g_amp=1.0, clip=1.0, clip_value=None, grad_scale=1.0, applied=5):
        self.table = table
        self.kw = dict(clip=clip, clip_value=clip_value, grad_scale=grad_scale)
        self.p = P.tensor("lrdecay:p", (N,), 0.1).to(DEV)
        self.g = P.tensor("lrdecay:g", (N,), g_amp).to(DEV)
        self.m = P.tensor("lrdecay:m", (N,), 0.01).to(DEV)
        self.v = P.tensor("lrdecay:v", (N,), 0.01).to(DEV).square()
        self.host = self.record(np.float32(1.0))
        self.rec = torch.zeros(12, dtype=torch.int32, device=DEV)
        self.rec.view(torch.int64)[0:1].fill_(applied)
        self.ws = torch.zeros(1024, device=DEV)

    def record(self, c):
        """the host record with both learning rates premultiplied by the fp32 scale c: ONE fp32 multiply each"""
        from svit_amd.optim import pack_step_host
        lr = tuple(float(np.float32(x) * np.float32(c)) for x in LRS)
        return torch.from_numpy(pack_step_host(lr, WDS, self.kw["clip"], self.kw["clip_value"],
                                               self.kw["grad_scale"])).to(DEV)

    def twin(self):
        t = Tail.__new__(Tail)
        t.table, t.kw, t.host, t.ws = self.table, self.kw, self.host, torch.zeros(1024, device=DEV)
        t.p, t.g, t.m, t.v, t.rec = (x.clone() for x in (self.p, self.g, self.m, self.v, self.rec))
        return t

    def guard(self, segs):
        from svit_amd import ops
        ops.step_guard_seg(self.g, _segs(segs), self.host, self.rec, self.table, self.ws)

    def run_lr(self, segs, scales, nd):
        from svit_amd import ops
        self.guard(segs)
        ops.adamw_step_guarded_lr(self.p, self.g, self.m, self.v, nd, _segs(segs), np.asarray(scales, dtype=np.float32),
                                  self.host, self.rec, *BETAS, EPS)
        torch.cuda.synchronize()

    def run_seg(self, segs, nd, only=None, host=None):
        """the `_seg` pair: the guard over `segs`, AdamW over `only` (default: the same table) with `host`"""
        from svit_amd import ops
        self.guard(segs)
        ops.adamw_step_guarded_seg(self.p, self.g, self.m, self.v, nd, _segs(segs if only is None else only),
                                   self.host if host is None else host, self.rec, *BETAS, EPS)
        torch.cuda.synchronize()

    def stats(self):
        from svit_amd import hip
        return hip.StepDev.from_buffer_copy(self.rec.cpu().numpy().tobytes())


def split_at(rows, scales, nd):
    """no range across n_decay: one that would cross is cut there, both parts keep its scale"""
    out_r, out_s = [], []
    for (a, b), c in zip(rows, scales):
        for lo, hi in ((a, min(b, nd)), (max(a, nd), b)) if a < nd < b else ((a, b),):
            out_r.append([lo, hi])
            out_s.append(c)
    return out_r, out_s


def _tables(nd):
    S = SCALES
    t = {}
    # bounds exactly on window edges; the last whole quad [6144, 6148) and the tail outside every range
    t["window edges"] = ([[0, 1024], [1024, 2048], [2048, 4096], [5120, 6144]], [S[0], S[1], S[2], S[3]])
    # 4, 8 and 12 floats inside the window [1024, 2048)
    t["three in a window"] = ([[0, 8], [1028, 1032], [1040, 1048], [1100, 1112], [4000, 5000]],
                              [S[1], S[2], S[3], S[0], S[1]])
    # every range begins where the one before ends, the scales differ; reaches the last whole quad
    t["touching"] = ([[0, 512], [512, 516], [516, 2048], [2048, 2052], [2052, N4]], [S[3], S[2], S[1], S[0], S[2]])
    # the limit: 64 ranges of 4 .. 20 floats
    t["64 ranges"] = ([[96 * i, 96 * i + 4 * (1 + i % 5)] for i in range(64)], [S[i % 4] for i in range(64)])
    return {k: split_at(r, s, nd) for k, (r, s) in t.items()}


def _mask(rows):
    m = torch.zeros(N, dtype=torch.bool, device=DEV)
    for a, b in rows:
        assert not bool(m[a:b].any())
        m[a:b] = True
    return m


def _poison_outside(t, inside):
    """canaries: NaN / +-inf / 1e30 gradients outside the ranges, marker values in p, m, v"""
    out = ~inside
    bad = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e30], device=DEV).repeat(N // 4 + 1)[:N]
    t.g[out] = bad[out]
    t.p[out], t.m[out], t.v[out] = 123.456, -7.0, 9.0e9


MODES = {"norm clip": {}, "clip by value": dict(g_amp=0.05, clip_value=0.01), "grad_scale 0.5": dict(grad_scale=0.5)}
# n_decay on a scale boundary and window edge (2048); inside a window, where it cuts a range in two (3000)
NDS = (2048, 3000)


def test_the_designated_scale_has_an_inexact_product():
    for lr in LRS:
        exact = float(np.float32(lr)) * float(INEXACT)
        assert float(np.float32(lr) * INEXACT) != exact


@pytest.mark.parametrize("nd", NDS)
def test_a_all_scales_one_is_the_seg_kernel(table, nd):
    for name, (rows, _) in _tables(nd).items():
        a = Tail(table)
        _poison_outside(a, _mask(rows))
        b = a.twin()
        a.run_lr(rows, [1.0] * len(rows), nd)
        b.run_seg(rows, nd)
        for what in ("p", "m", "v", "rec"):
            assert same(getattr(a, what), getattr(b, what)), (name, what)
        assert a.stats().apply == 1 and a.stats().applied == 6


@pytest.mark.parametrize("nd", NDS)
def test_a_whole_buffer_as_two_ranges_is_the_plain_pair(table, nd):
    """on the first N4 floats (a range cannot reach the n % 4 tail the plain kernel also steps)"""
    from svit_amd import ops
    a = Tail(table)
    b = a.twin()
    ops.step_guard(a.g[:N4], a.host, a.rec, a.table, a.ws)
    ops.adamw_step_guarded_lr(a.p[:N4], a.g[:N4], a.m[:N4], a.v[:N4], nd, _segs([[0, nd], [nd, N4]]),
                              np.ones(2, dtype=np.float32), a.host, a.rec, *BETAS, EPS)
    ops.step_guard(b.g[:N4], b.host, b.rec, b.table, b.ws)
    ops.adamw_step_guarded(b.p[:N4], b.g[:N4], b.m[:N4], b.v[:N4], nd, b.host, b.rec, *BETAS, EPS)
    torch.cuda.synchronize()
    for what in ("p", "m", "v", "rec"):
        assert same(getattr(a, what), getattr(b, what)), what
    assert not same(a.p[:N4], Tail(table).p[:N4]) and same(a.p[N4:], Tail(table).p[N4:])


@pytest.mark.parametrize("nd", NDS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["window edges", "three in a window", "touching", "64 ranges"])
def test_b_scaled_ranges_against_the_seg_kernel_at_the_premultiplied_lr(table, name, mode, nd):
    rows, scales = _tables(nd)[name]
    assert len(rows) <= 64 and (name != "64 ranges" or len(rows) == 64)
    a = Tail(table, **MODES[mode])
    inside = _mask(rows)
    _poison_outside(a, inside)
    start = a.twin()
    a.run_lr(rows, scales, nd)
    # the yardstick: per distinct scale c, the `_seg` kernel on a fresh copy, its record holding fp32(lr) * fp32(c), over
    # that class's ranges only (the guard runs over the whole table: the step has one coefficient)
    want = {k: getattr(start, k).clone() for k in "pmv"}
    for c in sorted(set(float(s) for s in scales)):
        mine = [r for r, s in zip(rows, scales) if float(s) == c]
        t = start.twin()
        t.run_seg(rows, nd, only=mine, host=t.record(np.float32(c)))
        assert same(t.rec, a.rec), (name, mode, c)
        sel = _mask(mine)
        for k in "pmv":
            want[k][sel] = getattr(t, k)[sel]
    s = a.stats()
    assert s.apply == 1 and s.applied == 6 and s.skipped == 0      # NaN / inf / 1e30 outside did not drop the step
    if mode == "norm clip":
        assert 0.0 < s.coef < 1.0
    if mode == "grad_scale 0.5":
        assert 0.0 < s.coef <= 0.5
    for k in "pmv":
        x, y, x0 = getattr(a, k), want[k], getattr(start, k)
        assert same(x[inside], y[inside]), (name, mode, k, int((bits(x[inside]) != bits(y[inside])).sum()))
        assert same(x[~inside], x0[~inside]), (name, mode, k, "an element outside the ranges was written")
        assert same(x, y)
        assert not same(x[inside], x0[inside])
    # the scales did something: the ranges at 0.75^17 (7.5e-3) moved far less than those at 10
    lo = _mask([r for r, c in zip(rows, scales) if c == SCALES[1]])
    hi = _mask([r for r, c in zip(rows, scales) if c == SCALES[2]])
    d = (a.p - start.p).abs()
    assert float(d[lo].mean()) < 0.1 * float(d[hi].mean())


@pytest.mark.parametrize("nd", NDS)
def test_c_a_nan_inside_a_range_drops_the_step(table, nd):
    rows, scales = _tables(nd)["three in a window"]
    a = Tail(table)
    _poison_outside(a, _mask(rows))
    a.g[1041] = float("nan")
    b = a.twin()
    before = [x.clone() for x in (a.p, a.g, a.m, a.v)]
    r0 = a.stats()
    a.run_lr(rows, scales, nd)
    b.run_seg(rows, nd)
    for what, x, x0 in zip("pgmv", (a.p, a.g, a.m, a.v), before):
        assert same(x, x0), what
    s, sb = a.stats(), b.stats()
    assert (s.apply, s.applied, s.skipped, s.consecutive) == (0, r0.applied, r0.skipped + 1, r0.consecutive + 1)
    assert (s.apply, s.applied, s.skipped, s.consecutive) == (sb.apply, sb.applied, sb.skipped, sb.consecutive)
    assert same(a.rec, b.rec)


def test_d_wrapper_refuses_bad_scales_and_bad_tables(table):
    from svit_amd import hip, ops
    nd = 2048
    a = Tail(table)
    rows, scales = _tables(nd)["window edges"]

    def refused(rows, scales):
        before = [x.clone() for x in (a.p, a.m, a.v, a.rec)]
        with pytest.raises(hip.SvitHipError):
            ops.adamw_step_guarded_lr(a.p, a.g, a.m, a.v, nd, _segs(rows), scales, a.host, a.rec, *BETAS, EPS)
        torch.cuda.synchronize()
        assert all(same(x, y) for x, y in zip((a.p, a.m, a.v, a.rec), before))

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for at in range(len(rows)):
            sc = np.array(scales, dtype=np.float32)
            sc[at] = bad
            refused(rows, sc)
    # every table the `_seg` wrapper refuses, and one across n_decay
    for bad in ([[8, 16], [0, 8]], [[0, 6]], [[0, N + 1]], [[16, 16]], [[0, 16], [8, 24]], [[nd - 8, nd + 8]]):
        refused(bad, np.ones(len(bad), dtype=np.float32))
    refused([[8 * i, 8 * i + 4] for i in range(65)], np.ones(65, dtype=np.float32))
    # scales that are not float32 [S] on the host
    refused(rows, np.ones(len(rows), dtype=np.float64))
    refused(rows, np.ones(len(rows) + 1, dtype=np.float32))
    refused(rows, [1.0] * len(rows))


# ======================================================================================================= model ====
LR = 1e-3


def build(mode="deterministic"):
    """the tiny model of the other step tests with the procedural weights, in train mode"""
    from svit_amd import config
    from svit_amd.model import MODEL_REGISTRY
    cfg = config.ssv2_cfg(num_frames=4, crop=64)
    cfg.MVIT.DROPPATH_RATE = 0.0
    cfg.MODEL.DROPOUT_RATE = 0.0
    if mode == "reproducible":
        cfg.SVIT.REPRODUCIBLE = True
    model = MODEL_REGISTRY.get("SViT")(cfg).cuda()
    model.load_state_dict(P.state_dict(R.param_shapes(R.make_spec(4, 64, drop_path_rate=0.0, dropout_rate=0.0))))
    model.train()
    if mode == "deterministic":
        model.engine.deterministic = True
    assert len(model.plan.blocks) == L.DEPTH == cfg.MVIT.DEPTH
    return cfg, model


def batch(tag=""):
    return P.frames(2, 4, 64, tag="clip" + tag).cuda(), P.labels(2, tag="label" + tag).cuda()


def ce(p, e, y):
    return torch.nn.functional.cross_entropy(p, y)


def fwd_bwd(model, x, y):
    for p in model.parameters():
        p.grad = None
    model.flat.grad.zero_()
    logits, _ = model([x], {})
    torch.nn.functional.cross_entropy(logits, y).backward()
    torch.cuda.synchronize()
    return model.flat.grad.clone()


def scale_of(name, mult=()):
    return float(L.scale(name, L.DECAY, mult))


def solver_cfg(cfg, decayed, guarded, mult=L.LR_MULT, wd=0.05):
    cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY, cfg.SOLVER.CLIP_GRAD_L2NORM = LR, wd, 1.0
    if decayed:
        cfg.SOLVER.LAYER_DECAY = L.DECAY
        cfg.SVIT.LR_MULT = [list(p) for p in mult]
    if guarded:
        cfg.SVIT.GUARDED_STEP = True
    return cfg


def _three_steps(decayed):
    """classic and guarded tails through construct_optimizer and torch.optim.AdamW with one group per range, three steps
    on the same clipped gradients: weight decay 0 on the first step, 0.05 after.  -> per-element |ours - torch|, the
    weights, and what the first step's checks need"""
    from svit_amd import optim
    x, y = batch()
    cfg_c, mc = build()
    cfg_g, mg = build()
    oc = optim.construct_optimizer(mc, solver_cfg(cfg_c, decayed, False, wd=0.0))
    og = optim.construct_optimizer(mg, solver_cfg(cfg_g, decayed, True, wd=0.0))
    assert type(oc) is optim.FusedClipAdamW and type(og) is optim.GuardedClipAdamW
    flat = mg.flat
    if decayed:
        ranges = [(int(a), int(b), np.float32(c)) for (a, b), c in zip(og.lr_segments, og.lr_scales)]
    else:
        ranges = [(0, flat.n_decay, np.float32(1.0)), (flat.n_decay, flat.total, np.float32(1.0))]
    w0 = flat.data.clone()
    tp = [torch.nn.Parameter(w0[a:b].cpu().clone()) for a, b, _ in ranges]
    topt = torch.optim.AdamW([{"params": [q], "lr": LR, "weight_decay": 0.0} for q in tp], lr=LR, betas=BETAS, eps=EPS)
    first = None
    for i in range(3):
        lr = LR * (i + 1)
        wd = 0.0 if i == 0 else 0.05
        for o in (oc, og):
            optim.set_lr(o, lr)
            o.param_groups[0]["weight_decay"] = wd
        gc, gg = fwd_bwd(mc, x, y), fwd_bwd(mg, x, y)
        assert same(gc, gg)
        oc.step()
        og.step()
        torch.cuda.synchronize()
        st = og.stats()
        assert st["applied"] == i + 1 and 0.0 < st["clip_coef"] <= 1.0
        clipped = (gg * st["clip_coef"]).cpu()                  # one fp32 multiply, as the kernels form g * coef
        for q, grp, (a, b, c) in zip(tp, topt.param_groups, ranges):
            q.grad = clipped[a:b].clone()
            grp["lr"] = float(np.float32(lr) * c)
            grp["weight_decay"] = wd if a < flat.n_decay else 0.0
        topt.step()
        for what, p, q in (("weights", mc.flat.data, mg.flat.data), ("exp_avg", oc.exp_avg, og.exp_avg),
                           ("exp_avg_sq", oc.exp_avg_sq, og.exp_avg_sq)):
            assert same(p, q), ("step %d" % (i + 1), what, int((bits(p) != bits(q)).sum()))
        if i == 0:
            first = dict(w0=w0.cpu(), w1=flat.data.cpu().clone(), g=clipped, ranges=ranges, lr=lr)
    ours = flat.data.cpu()
    theirs = torch.empty_like(ours)
    covered = torch.zeros(ours.numel(), dtype=torch.bool)
    for q, (a, b, _) in zip(tp, ranges):
        theirs[a:b] = q.detach()
        covered[a:b] = True
    assert bool(covered.all())
    return dict(dev=(ours.double() - theirs.double()).abs(), w=ours, first=first)


def test_e_three_steps_classic_guarded_and_torch():
    """Measured on an MI355X (tiny model, three steps): max |ours - torch| 3.576e-07 for the unscaled control, 3.651e-07
    scaled; the assertion message prints both figures of the run."""
    scaled = _three_steps(True)
    f = scaled["first"]
    # the first step, weight decay 0: |dw| = lr_eff * |g| / (|g| + eps) -- lr_eff wherever |g| >> eps -- so the ranges move
    # in the ratios of their scales.  Tolerance: AdamW's fp32 arithmetic (a few 2^-24 relative: 1e-5 is generous) plus the
    # rounding of the stored weight (one ulp of it).  Without the feature every range moves by lr itself.
    dw = (f["w1"].double() - f["w0"].double()).abs()
    g = f["g"].double().abs()
    ulp = f["w0"].double().abs() * 2.0 ** -23 + 2.0 ** -149
    seen = set()
    for a, b, c in f["ranges"]:
        lr_eff = float(np.float32(f["lr"]) * c)
        want = lr_eff * g[a:b] / (g[a:b] + EPS)
        err = (dw[a:b] - want).abs() - ulp[a:b] - 1e-5 * lr_eff
        assert float(err.max()) <= 0.0, ("range [%d, %d) at scale %r: |dw| is not lr_eff |g| / (|g| + eps)" % (a, b, float(c)),
                                         float(dw[a:b].max()), lr_eff)
        if float(g[a:b].max()) >= 1e-4:         # eps is 1e-4 of that: the largest step of the range is lr_eff
            top = float(dw[a:b].max())
            slack = float(ulp[a:b].max()) + 2e-4 * lr_eff
            assert lr_eff - slack <= top <= lr_eff + slack, (a, b, float(c), top, lr_eff)
            seen.add(float(c))
    assert len(seen) >= 3, "too few ranges with a usable gradient: %s" % sorted(seen)
    assert {float(np.float32(4.0)), float(np.float32(2.0)), float(np.float32(0.75 ** 17))} & seen
    # against torch: the unscaled control's deviation, measured here, sets the bar -- twice that, floored at one fp32 ulp of
    # the weight (the scale adds one rounding)
    control = _three_steps(False)
    d_control, d_scaled = float(control["dev"].max()), float(scaled["dev"].max())
    floor = scaled["w"].double().abs() * 2.0 ** -23
    over = scaled["dev"] - torch.clamp(floor, min=2.0 * d_control)
    msg = "max |ours - torch| after three steps: control (LAYER_DECAY 1) %.3e, scaled %.3e" % (d_control, d_scaled)
    print(msg)
    assert float(over.max()) <= 0.0, msg


def _trace_names(monkeypatch, fn):
    """names of the library launches issued while fn() runs, in order"""
    from svit_amd import hip
    names = []
    real = hip.call

    def logging(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    monkeypatch.setattr(hip, "call", logging)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(hip, "call", real)
    return out, names


def _tail(names):
    """the optimizer tail's launches among `names`"""
    return [n for n in names if n.startswith("svit_step_guard") or n.startswith("svit_adamw_step")]


def test_f_graphed_step_replays_the_scaled_tail(monkeypatch):
    from svit_amd import optim
    from svit_amd.graph import GraphedTrainStep
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return torch.nn.functional.cross_entropy(p, y) * poison

    x, y = batch()
    cfg_g, mg = build()
    cfg_e, me = build()
    og = optim.construct_optimizer(mg, solver_cfg(cfg_g, True, True, mult=()))
    oe = optim.construct_optimizer(me, solver_cfg(cfg_e, True, True, mult=()))
    assert og.lr_segments is not None and len(og.lr_segments) == 38
    w0 = mg.flat.data.clone()
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(mg, loss_fun, [x], y, optimizer=og))
    assert _tail(names) == ["svit_step_guard", "svit_adamw_step_guarded_lr"]
    assert names.index("svit_adamw_step_guarded_lr") == names.index("svit_step_guard") + 1
    torch.cuda.synchronize()
    assert same(mg.flat.data, w0) and og.stats()["applied"] == 0

    def eager():
        oe.zero_grad()
        logits, extra = me([x], {})
        loss = loss_fun(logits, extra, y)
        loss.backward()
        oe.step()
        return loss.detach()

    def compare(what):
        torch.cuda.synchronize()
        for name, a, b in (("weights", mg.flat.data, me.flat.data), ("exp_avg", og.exp_avg, oe.exp_avg),
                           ("exp_avg_sq", og.exp_avg_sq, oe.exp_avg_sq), ("grad", mg.flat.grad, me.flat.grad)):
            assert same(a, b), (what, name, int((bits(a) != bits(b)).sum()))
        assert og.stats() == oe.stats(), what

    for i in range(3):
        optim.set_lr(og, LR * (i + 1))
        optim.set_lr(oe, LR * (i + 1))
        lg, _ = step([x], y)
        le = eager()                    # (steps at the lr set_lr just wrote: equality says it reached the replay)
        assert same(lg, le)
        compare("step %d" % (i + 1))
    poison.fill_(float("nan"))
    before = mg.flat.data.clone()
    step([x], y)
    eager()
    compare("poisoned step")
    assert same(mg.flat.data, before) and og.stats()["skipped"] == 1 and og.stats()["applied"] == 3
    poison.fill_(1.0)
    step([x], y)
    eager()
    compare("the step after the poisoned one")
    assert og.stats()["applied"] == 4


def test_g_cut_4_and_decay_combine():
    from svit_amd import ops, optim
    from svit_amd.optim import pack_step_host
    cut = 4
    x, y = batch()
    _, model = build()
    flat = model.flat
    w0 = flat.data.clone()
    model.freeze_below(cut)
    fn = lambda n: scale_of(n, L.LR_MULT)
    opt = optim.GuardedClipAdamW(model, lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0, lr_scale=fn)
    tsegs = model.trainable_segments(cut)
    # the table is the intersection: exactly the trainable slots, each at its scale
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert 0 < len(names) < 405
    L.check_table(opt.lr_segments, opt.lr_scales,
                  L.element_scales(flat.slots, names, flat.total, L.DECAY, L.LR_MULT), flat.n_decay)
    inside = torch.zeros(flat.total, dtype=torch.bool, device=DEV)
    for a, b in tsegs:
        inside[int(a):int(b)] = True
    # the twin: the `_seg` guard over the trainable segments, then per distinct scale one `_seg` AdamW launch over that
    # class's ranges with the premultiplied lr
    tw = types.SimpleNamespace(p=w0.clone(), m=torch.zeros_like(w0), v=torch.zeros_like(w0),
                               rec=torch.zeros(12, dtype=torch.int32, device=DEV), ws=torch.zeros(1024, device=DEV))
    for i in range(2):
        lr = LR * (i + 1)
        optim.set_lr(opt, lr)
        g = fwd_bwd(model, x, y)
        opt.step()
        host = torch.from_numpy(pack_step_host((lr, lr), (0.05, 0.0), 1.0, None, 1.0)).to(DEV)
        ops.step_guard_seg(g, tsegs, host, tw.rec, opt.bias_table, tw.ws)
        for c in sorted(set(float(s) for s in opt.lr_scales)):
            mine = np.ascontiguousarray(opt.lr_segments[opt.lr_scales == np.float32(c)])
            le = float(np.float32(lr) * np.float32(c))
            host_c = torch.from_numpy(pack_step_host((le, le), (0.05, 0.0), 1.0, None, 1.0)).to(DEV)
            ops.adamw_step_guarded_seg(tw.p, g, tw.m, tw.v, flat.n_decay, mine, host_c, tw.rec, *BETAS, EPS)
        torch.cuda.synchronize()
        for what, a, b in (("weights", flat.data, tw.p), ("exp_avg", opt.exp_avg, tw.m), ("exp_avg_sq", opt.exp_avg_sq, tw.v),
                           ("record", opt.dev_rec, tw.rec)):
            assert same(a, b), ("step %d" % (i + 1), what, int((bits(a) != bits(b)).sum()))
    assert opt.step_count == 2
    assert same(flat.data[~inside], w0[~inside]), "a frozen weight moved"
    assert not same(flat.data[inside], w0[inside])
    assert int(torch.count_nonzero(opt.exp_avg[~inside])) == 0 and int(torch.count_nonzero(opt.exp_avg_sq[~inside])) == 0


def test_h_accumulated_step_k2_reproducible():
    """k = 2 micro-steps under SVIT.REPRODUCIBLE = one guarded decayed step at grad_scale 1/2 on the accumulated buffer"""
    from svit_amd import optim
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    _, model = build("reproducible")
    flat = model.flat
    A, B = batch(), batch("B")
    fn = lambda n: scale_of(n, L.LR_MULT)
    kw = dict(lr=LR, weight_decay=0.05, clip_grad_l2norm=1.0, lr_scale=fn)
    opt = optim.GuardedClipAdamW(model, **kw)
    micro = GraphedTrainStep(model, ce, [A[0]], A[1], accumulate=True)
    step = AccumulatedTrainStep(model, [micro, micro], opt)
    w0 = flat.data.clone()
    step([([A[0]], A[1]), ([B[0]], B[1])])
    torch.cuda.synchronize()
    assert opt.stats()["applied"] == 1 and not same(flat.data, w0)
    summed = flat.grad.clone()
    assert float(summed.abs().max()) > 0
    holder = types.SimpleNamespace(flat=types.SimpleNamespace(total=flat.total, n_decay=flat.n_decay, slots=flat.slots,
                                                              data=w0.clone(), grad=summed))
    twin = optim.GuardedClipAdamW(holder, grad_scale=0.5, **kw)
    assert np.array_equal(twin.lr_segments, opt.lr_segments) and np.array_equal(twin.lr_scales, opt.lr_scales)
    twin.step()
    torch.cuda.synchronize()
    for what, a, b in (("weights", flat.data, holder.flat.data), ("exp_avg", opt.exp_avg, twin.exp_avg),
                       ("exp_avg_sq", opt.exp_avg_sq, twin.exp_avg_sq)):
        assert same(a, b), (what, int((bits(a) != bits(b)).sum()))
    assert opt.stats() == twin.stats()


def test_i_checkpoint_round_trip(tmp_path):
    from svit_amd import checkpoint, optim
    x, y = batch()

    def make(decayed):
        cfg, model = build()
        return cfg, model, optim.construct_optimizer(model, solver_cfg(cfg, decayed, True))

    def one_step(model, opt):
        optim.set_lr(opt, LR)
        opt.zero_grad()
        logits, _ = model([x], {})
        torch.nn.functional.cross_entropy(logits, y).backward()
        opt.step()
        torch.cuda.synchronize()

    cfg, model, opt = make(True)
    for _ in range(2):
        one_step(model, opt)
    path = checkpoint.save_checkpoint(str(tmp_path), model, opt, 3, cfg)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    groups = ck["optimizer_state"]["param_groups"]
    assert len(groups) > 2 and all("layer_decay" in g for g in groups) and len(ck["optimizer_state"]["state"]) == 405
    assert sorted(j for g in groups for j in g["params"]) == list(range(405))
    # decayed -> file -> a fresh decayed optimizer continues bit for bit
    cfg2, model2, opt2 = make(True)
    model2.flat.data.zero_()
    assert checkpoint.load_checkpoint(path, model2, data_parallel=False, optimizer=opt2) == 3
    assert same(model2.flat.data, model.flat.data)
    assert same(opt2.exp_avg, opt.exp_avg) and same(opt2.exp_avg_sq, opt.exp_avg_sq) and opt2.step_count == 2
    assert all(np.float32(g["lr"]) == np.float32(LR) or abs(g["lr"] / LR - 1.0) < 2.0 ** -22 for g in opt2.param_groups)
    one_step(model, opt)
    one_step(model2, opt2)
    assert same(model2.flat.data, model.flat.data) and same(opt2.exp_avg, opt.exp_avg) and same(opt2.exp_avg_sq, opt.exp_avg_sq)
    assert opt2.step_count == 3
    # a two-group state loads into a decayed optimizer with equal moments, and the other way round
    cfg3, model3, plain = make(False)
    assert plain.lr_segments is None
    one_step(model3, plain)
    two = plain.state_dict()
    assert len(two["param_groups"]) == 2
    opt2.load_state_dict(two)
    assert same(opt2.exp_avg, plain.exp_avg) and same(opt2.exp_avg_sq, plain.exp_avg_sq) and opt2.step_count == 1
    assert [g["lr"] for g in opt2.param_groups] == [LR, LR]
    plain.load_state_dict(opt.state_dict())
    assert same(plain.exp_avg, opt.exp_avg) and same(plain.exp_avg_sq, opt.exp_avg_sq) and plain.step_count == 3


def test_j_without_the_keys_nothing_changes(monkeypatch):
    """the captured step of a cfg without LAYER_DECAY / LR_MULT issues the launches it issued before the optimizer knew
    about scales: the body of a capture without an optimizer, then the guard and the plain guarded AdamW"""
    from svit_amd import optim
    from svit_amd.graph import GraphedTrainStep
    x, y = batch()
    cfg, ma = build()
    _, mb = build()
    opt = optim.construct_optimizer(ma, solver_cfg(cfg, False, True))
    assert opt.lr_segments is None and opt.lr_scales is None and len(opt.param_groups) == 2
    _, bare = _trace_names(monkeypatch, lambda: GraphedTrainStep(mb, ce, [x], y))
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(ma, ce, [x], y, optimizer=opt))
    assert _tail(bare) == [] and _tail(names) == ["svit_step_guard", "svit_adamw_step_guarded"]
    assert names.index("svit_adamw_step_guarded") == names.index("svit_step_guard") + 1
    assert [n for n in names if n not in _tail(names)] == bare
    assert not [n for n in names if n.endswith("_lr")]
    step([x], y)
    torch.cuda.synchronize()
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 2 and all("layer_decay" not in g for g in sd["param_groups"])
    assert [g["params"] for g in sd["param_groups"]] == [list(range(len(opt._order()[0]))),
                                                         list(range(len(opt._order()[0]), 405))]
    assert [g["lr"] for g in sd["param_groups"]] == [LR, LR]
