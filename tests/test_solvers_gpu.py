"""SGD and Adam on the guarded tail, on the GPU: svit_sgd_step_guarded / svit_adam_step_guarded against their NumPy
float32 restatements (optim.sgd_step_host / adam_step_host), and the model under SOLVER.OPTIMIZING_METHOD sgd / adam --
the captured and the accumulated step, a frozen cut with LAYER_DECAY, a checkpoint round trip.  Bit equality throughout.
Needs a real MI355X."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from oracle import svit_ref as R
from tests import layer_decay_cases as L

DEV = "cuda"
N = 8 * 1024 + 11               # eight windows of 1024 floats and a ninth of 11: n % 4 = 3
N4 = N // 4 * 4
BETAS, EPS = (0.9, 0.999), 1e-8
LRS, WDS = (1e-2, 3e-2), (1e-4, 0.0)        # the two sides of n_decay: decayed, not decayed
INEXACT = np.float32(1.0 / 3.0)
SCALES = [np.float32(1.0), np.float32(0.75 ** 17), np.float32(10.0), INEXACT]
assert all(float(np.float32(lr) * INEXACT) != float(np.float32(lr)) * float(INEXACT) for lr in LRS)   # inexact products


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def same_np(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _segs(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(-1, 2))


# ===================================================================================================== kernels ====
@pytest.fixture(scope="module")
def table():
    from svit_amd import ops
    return torch.from_numpy(ops.adamw_bias_table(*BETAS)).to(DEV)


SGD_KINDS = {
    "sgd momentum 0": dict(momentum=0.0, dampening=0.0, nesterov=False),
    "sgd momentum 0.9": dict(momentum=0.9, dampening=0.0, nesterov=False),
    "sgd dampening 0.1": dict(momentum=0.9, dampening=0.1, nesterov=False),
    "sgd nesterov": dict(momentum=0.9, dampening=0.0, nesterov=True),
}
KINDS = list(SGD_KINDS) + ["adam"]


class Tail:
    """p, g and the solver's state f32 [n] + the two step records.  kind: a key of SGD_KINDS or "adam" """

    def __init__(self, kind, table, n=N, g_amp=1.0, clip=1.0, clip_value=None, grad_scale=1.0, applied=0, null_buf=False):
        self.kind, self.n = kind, n
        self.cv = clip_value
        self.p = P.tensor("solver:p", (n,), 0.1).to(DEV)
        self.g = P.tensor("solver:g", (n,), g_amp).to(DEV)
        if kind == "adam":
            self.state = [P.tensor("solver:m", (n,), 0.01).to(DEV), P.tensor("solver:v", (n,), 0.01).to(DEV).square()]
            self.table = table
        else:
            # with momentum 0 the buffer is NULL, or a canary the kernel must not touch
            self.state = [] if null_buf else [P.tensor("solver:b", (n,), 0.01).to(DEV)]
            self.table = torch.zeros((0, 2), device=DEV)        # no bias corrections: the guard records 1.0 for both
        from svit_amd.optim import pack_step_host
        self.host = torch.from_numpy(pack_step_host(LRS, WDS, clip, clip_value, grad_scale)).to(DEV)
        self.rec = torch.zeros(12, dtype=torch.int32, device=DEV)
        self.rec.view(torch.int64)[0:1].fill_(applied)
        self.ws = torch.zeros(1024, device=DEV)

    def snapshot(self):
        return [x.cpu().numpy().copy() for x in [self.p, self.g] + self.state]

    def stats(self):
        from svit_amd import hip
        return hip.StepDev.from_buffer_copy(self.rec.cpu().numpy().tobytes())

    def launch(self, rows, scales, nd, host=None):
        """the solver's launch alone (the guard has run)"""
        from svit_amd import ops
        sc = np.asarray(scales, dtype=np.float32) if isinstance(scales, list) else scales
        host = self.host if host is None else host
        if self.kind == "adam":
            ops.adam_step_guarded(self.p, self.g, self.state[0], self.state[1], nd, _segs(rows), sc, host, self.rec,
                                  *BETAS, EPS)
        else:
            k = SGD_KINDS[self.kind]
            ops.sgd_step_guarded(self.p, self.g, self.state[0] if self.state else None, nd, _segs(rows), sc, host,
                                 self.rec, k["momentum"], k["dampening"], k["nesterov"])

    def step(self, rows, scales, nd):
        """the guard over the ranges, then the solver's one launch"""
        from svit_amd import ops
        ops.step_guard_seg(self.g, _segs(rows), self.host, self.rec, self.table, self.ws)
        self.launch(rows, scales, nd)
        torch.cuda.synchronize()

    def expected(self, before, rows, scales, nd, st, lrs=LRS):
        """the restatement applied to `before` on the elements inside the ranges, with the coefficient, the corrections
        and `first` the guard's record holds -> what snapshot() must now give"""
        from svit_amd import optim
        lr = np.zeros(self.n, dtype=np.float32)
        wd = np.zeros(self.n, dtype=np.float32)
        inside = np.zeros(self.n, dtype=bool)
        for (a, b), c in zip(rows, [1.0] * len(rows) if scales is None else scales):
            w = 0 if a < nd else 1
            lr[a:b] = np.float32(lrs[w]) * np.float32(c)        # ONE fp32 multiply
            wd[a:b] = WDS[w]
            assert not inside[a:b].any()
            inside[a:b] = True
        want = [x.copy() for x in before]
        p, g = before[0][inside], before[1][inside]
        if self.kind == "adam":
            new = optim.adam_step_host(p, g, before[2][inside], before[3][inside], st.coef, st.bc1, st.bc2_sqrt, lr[inside],
                                       wd[inside], BETAS, EPS, clip_value=self.cv)
            for k, x in zip((0, 2, 3), new):
                want[k][inside] = x
        else:
            k = SGD_KINDS[self.kind]
            buf = before[2][inside] if k["momentum"] != 0 else None
            pn, bn = optim.sgd_step_host(p, g, buf, st.coef, lr[inside], wd[inside], first=(st.applied == 1),
                                         clip_value=self.cv, **k)
            want[0][inside] = pn
            if bn is not None:
                want[2][inside] = bn
        return want, inside


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
    t["whole buffer"] = ([[0, N4]], [S[0]])
    t["window edges"] = ([[0, 1024], [1024, 2048], [2048, 4096], [5120, 6144], [7168, N4]], [S[0], S[1], S[2], S[3], S[1]])
    # 4, 8 and 12 floats inside the window [1024, 2048)
    t["three in a window"] = ([[0, 8], [1028, 1032], [1040, 1048], [1100, 1112], [4000, 5000]],
                              [S[1], S[2], S[3], S[0], S[1]])
    # every range begins where the one before ends, the scales differ; reaches the last whole quad
    t["touching"] = ([[0, 512], [512, 516], [516, 2048], [2048, 2052], [2052, N4]], [S[3], S[2], S[1], S[0], S[2]])
    # the limit: 64 ranges of 4 .. 20 floats
    t["64 ranges"] = ([[128 * i, 128 * i + 4 * (1 + i % 5)] for i in range(64)], [S[i % 4] for i in range(64)])
    return {k: split_at(r, s, nd) for k, (r, s) in t.items()}


def _poison_outside(t, inside):
    """canaries: NaN / +-inf / 1e30 gradients outside the ranges, marker values in p and the state"""
    out = torch.from_numpy(~inside).to(DEV)
    bad = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e30], device=DEV).repeat(t.n // 4 + 1)[:t.n]
    t.g[out] = bad[out]
    t.p[out] = 123.456
    for x, mark in zip(t.state, (-7.0, 9.0e9)):
        x[out] = mark


def _inside(rows, n=N):
    m = np.zeros(n, dtype=bool)
    for a, b in rows:
        m[a:b] = True
    return m


def _check(t, before, rows, scales, nd, what):
    st = t.stats()
    want, inside = t.expected(before, rows, scales, nd, st)
    got = t.snapshot()
    names = ["p", "g"] + (["m", "v"] if t.kind == "adam" else ["buf"])
    for name, x, y, x0 in zip(names, got, want, before):
        assert same_np(x[~inside], x0[~inside]), (what, name, "an element outside the ranges was written")
        assert same_np(x, y), (what, name, int((x.view(np.int32) != y.view(np.int32)).sum()))
    assert not same_np(got[0][inside], before[0][inside]), (what, "the weights did not move")
    return st


MODES = {"norm clip": {}, "clip by value": dict(g_amp=0.05, clip_value=0.01), "grad_scale 0.5": dict(grad_scale=0.5)}
# n_decay on a window edge (2048); inside a window, where it cuts a range in two (3000)
NDS = (2048, 3000)


@pytest.mark.parametrize("nd", NDS)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", KINDS)
def test_a_kernel_is_the_restatement(table, kind, mode, nd):
    """every table, three steps each (step 1 is "first": the buffer becomes gi exactly; Adam's corrections are those of
    steps 1-3), canaries outside every range"""
    for name, (rows, scales) in _tables(nd).items():
        assert len(rows) <= 64 and (name != "64 ranges" or len(rows) == 64)
        t = Tail(kind, table, **MODES[mode])
        inside = _inside(rows)
        _poison_outside(t, inside)
        for i in range(3):
            before = t.snapshot()
            t.step(rows, None if name == "whole buffer" else scales, nd)       # (scales == NULL: every scale is 1.0)
            st = _check(t, before, rows, scales, nd, (name, "step %d" % (i + 1)))
            assert (st.apply, st.applied, st.skipped) == (1, i + 1, 0)       # NaN / inf / 1e30 outside did not drop it
            if mode == "norm clip":
                assert 0.0 < st.coef < 1.0
            if mode == "grad_scale 0.5":
                assert 0.0 < st.coef <= 0.5
            if kind != "adam":
                assert st.bc1 == 1.0 and st.bc2_sqrt == 1.0
            if i == 0 and kind not in ("adam", "sgd momentum 0"):
                # the first applied step: the buffer is gi itself, whatever it held
                gi = before[1][inside] * np.float32(st.coef)
                if t.cv:
                    gi = np.minimum(np.maximum(gi, -np.float32(t.cv)), np.float32(t.cv))
                wd = np.where(np.arange(N) < nd, np.float32(WDS[0]), np.float32(WDS[1]))[inside]
                gi = np.where(wd != 0, gi + before[0][inside] * wd, gi)
                assert same_np(t.snapshot()[2][inside], gi), name
            t.g.mul_(0.5 + 0.25 * i)            # another gradient for the next step (the canaries stay non-finite / huge)
        if name == "touching" and kind != "adam":
            # the scales did something: the ranges at 0.75^17 (7.5e-3) moved far less than those at 10
            d = np.abs(t.snapshot()[0] - P.tensor("solver:p", (N,), 0.1).numpy())
            lo = _inside([r for r, c in zip(rows, scales) if c == SCALES[1]])
            hi = _inside([r for r, c in zip(rows, scales) if c == SCALES[2]])
            assert float(d[lo].mean()) < 0.1 * float(d[hi].mean())


@pytest.mark.parametrize("null_buf", [True, False])
def test_a_momentum_0_never_touches_the_buffer(table, null_buf):
    nd = 3000
    rows, scales = _tables(nd)["three in a window"]
    t = Tail("sgd momentum 0", table, null_buf=null_buf)
    assert (t.state == []) == null_buf
    before = t.snapshot()
    t.step(rows, scales, nd)
    _check(t, before, rows, scales, nd, "momentum 0")      # (with a buffer: it is in the snapshot and must be unchanged)


def test_a_n_decay_at_the_ends(table):
    """one range over the whole buffer, all of it decayed / none of it"""
    for kind in ("sgd nesterov", "adam"):
        for nd in (N4, 0):
            t = Tail(kind, table)
            before = t.snapshot()
            t.step([[0, N4]], None, nd)
            _check(t, before, [[0, N4]], None, nd, (kind, nd))
            assert same_np(t.snapshot()[0][N4:], before[0][N4:])        # the n % 4 tail is outside every range


def test_a_adam_past_the_bias_table(table):
    assert table.shape[0] == 17321
    nd = 3000
    rows, scales = _tables(nd)["touching"]
    t = Tail("adam", table, applied=17400)
    before = t.snapshot()
    t.step(rows, scales, nd)
    st = _check(t, before, rows, scales, nd, "past the table")
    assert st.applied == 17401 and st.bc1 == 1.0 and st.bc2_sqrt == 1.0


def test_a_adam_tiny_and_denormal_second_moments(table):
    """the square root's scaled path (inputs below 2^-96), denormal and zero second moments, gradients whose squares
    are denormal: every one of them has to come out as NumPy's correctly rounded operations give it"""
    nd = 3000
    rows, scales = _tables(nd)["touching"]
    t = Tail("adam", table, g_amp=1e-16)
    t.state[0].mul_(1e-14)
    t.state[1].mul_(1e-30)                      # ~1e-34 and below: under 2^-96 = 1.3e-29
    t.state[1][1000:2000].mul_(1e-6)            # denormal
    t.state[1][2000:2600].zero_()
    t.g[2000:2300].zero_()                      # v stays exactly 0 there: the root passes zero through
    t.g[4000:5000].mul_(1e-4)                   # g * g ~ 1e-40: a denormal product
    v = t.state[1].cpu().numpy()
    assert 0 < v[1000:2000].max() < 1.18e-38 and v[:1000].max() < 2.0 ** -96
    for i in range(2):
        before = t.snapshot()
        t.step(rows, scales, nd)
        st = _check(t, before, rows, scales, nd, "tiny, step %d" % (i + 1))
        assert st.apply == 1 and st.coef == 1.0


@pytest.mark.parametrize("kind", ["sgd momentum 0.9", "adam"])
def test_a_more_windows_than_the_grid_holds(table, kind):
    """4096 workgroups at most: past 4096 x 1024 floats a workgroup takes a second window"""
    n = 4096 * 1024 + 3 * 1024 + 8
    nd = 4096 * 1024 + 512
    rows = [[0, 2048], [4096 * 1024 - 256, nd], [nd, nd + 1000], [n - 520, n]]
    scales = [SCALES[2], SCALES[3], SCALES[0], SCALES[1]]
    t = Tail(kind, table, n=n)
    inside = _inside(rows, n)
    _poison_outside(t, inside)
    before = t.snapshot()
    t.step(rows, scales, nd)
    st = t.stats()
    want, _ = t.expected(before, rows, scales, nd, st)
    for name, x, y in zip("pgsv", t.snapshot(), want):
        assert same_np(x, y), (name, int((x.view(np.int32) != y.view(np.int32)).sum()))
    assert st.applied == 1 and not same_np(want[0][inside], before[0][inside])


@pytest.mark.parametrize("kind", ["sgd dampening 0.1", "adam"])
def test_b_a_nan_inside_a_range_drops_the_step(table, kind):
    nd = 3000
    rows, scales = _tables(nd)["three in a window"]
    t = Tail(kind, table)
    _poison_outside(t, _inside(rows))
    good = float(t.g[1041])
    t.g[1041] = float("nan")
    before = t.snapshot()
    t.step(rows, scales, nd)
    for name, x, x0 in zip("pgsv", t.snapshot(), before):
        assert same_np(x, x0), name
    st = t.stats()
    assert (st.apply, st.applied, st.skipped, st.consecutive) == (0, 0, 1, 1)
    # the dropped step was step 1: the finite step that follows is still "first"
    t.g[1041] = good
    before = t.snapshot()
    t.step(rows, scales, nd)
    st = _check(t, before, rows, scales, nd, "after the dropped step")
    assert (st.apply, st.applied, st.skipped, st.consecutive) == (1, 1, 1, 0)
    if kind != "adam":
        inside = _inside(rows)
        wd = np.where(np.arange(N) < nd, np.float32(WDS[0]), np.float32(WDS[1]))[inside]
        gi = before[1][inside] * np.float32(st.coef)
        gi = np.where(wd != 0, gi + before[0][inside] * wd, gi)
        assert same_np(t.snapshot()[2][inside], gi)         # buf == gi, no trace of what the buffer held, no dampening


def test_c_wrappers_refuse_before_any_launch(table):
    from svit_amd import hip, ops
    nd = 2048
    good_rows, good_scales = _tables(nd)["window edges"]
    for kind in ("sgd nesterov", "adam"):
        t = Tail(kind, table)
        before = t.snapshot() + [t.rec.cpu().numpy().copy()]

        def refused(rows, scales, **kw):
            with pytest.raises(hip.SvitHipError):
                if kw:
                    ops.sgd_step_guarded(t.p, t.g, kw.pop("buf", t.state[0]), nd, _segs(rows), scales, t.host, t.rec, **kw)
                else:
                    t.launch(rows, scales, nd)
            torch.cuda.synchronize()
            assert all(same_np(x, y) for x, y in zip(t.snapshot() + [t.rec.cpu().numpy()], before))

        for bad in ([[8, 16], [0, 8]], [[0, 6]], [[2, 8]], [[0, N + 1]], [[16, 16]], [[0, 16], [8, 24]], [[nd - 8, nd + 8]]):
            refused(bad, None)                              # unsorted; bounds not multiples of 4; past n; empty; overlap; across n_decay
        refused([[8 * i, 8 * i + 4] for i in range(65)], None)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            for at in (0, len(good_rows) - 1):
                sc = np.array(good_scales, dtype=np.float32)
                sc[at] = bad
                refused(good_rows, sc)
        refused(good_rows, np.ones(len(good_rows), dtype=np.float64))
        refused(good_rows, np.ones(len(good_rows) + 1, dtype=np.float32))
        if kind != "adam":
            refused(good_rows, None, momentum=0.9, dampening=0.1, nesterov=True)
            refused(good_rows, None, momentum=0.0, dampening=0.0, nesterov=True)
            refused(good_rows, None, momentum=0.9, dampening=0.0, nesterov=False, buf=None)


# ======================================================================================================= model ====
LR = {"sgd": 0.05, "adam": 1e-3}


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


def solver_cfg(cfg, method, clip=1.0, decayed=False, wd=1e-4, nesterov=True, momentum=0.9):
    s = cfg.SOLVER
    s.OPTIMIZING_METHOD, s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = method, LR[method], wd, clip
    s.MOMENTUM, s.DAMPENING, s.NESTEROV = momentum, 0.0, nesterov
    if decayed:
        s.LAYER_DECAY = L.DECAY
    return cfg


def host_twin(opt):
    """the restatement over copies of the optimizer's flat buffers: per-element rates from its own table"""
    flat = opt.flat
    segs, scales = opt._ranges()
    tw = types.SimpleNamespace(p=flat.data.cpu().numpy().copy(), segs=segs, scales=scales,
                               state=[getattr(opt, k).cpu().numpy().copy() for k in opt.STATE])
    tw.inside = _inside(segs.tolist(), flat.total)
    return tw


def host_step(tw, opt, g, st):
    from svit_amd import optim
    n, nd = opt.flat.total, opt.flat.n_decay
    lr, wd = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    for i, (a, b) in enumerate(tw.segs.tolist()):
        grp = opt.param_groups[0 if a < nd else 1]
        lr[a:b] = np.float32(grp["lr"]) * (np.float32(1.0) if tw.scales is None else tw.scales[i])
        wd[a:b] = grp["weight_decay"]
    m = tw.inside
    cv = opt.clip_value
    if isinstance(opt, optim.GuardedClipSGD):
        buf = tw.state[0][m] if opt.momentum != 0 else None
        pn, bn = optim.sgd_step_host(tw.p[m], g[m], buf, st["clip_coef"], lr[m], wd[m], opt.momentum, opt.dampening,
                                     opt.nesterov, first=(st["applied"] == 1), clip_value=cv)
        new = [bn] if bn is not None else []
    else:
        r = opt.dev_rec.cpu().numpy().view(np.float32)
        pn, mn, vn = optim.adam_step_host(tw.p[m], g[m], tw.state[0][m], tw.state[1][m], st["clip_coef"], r[7], r[8],
                                          lr[m], wd[m], opt.betas, opt.eps, clip_value=cv)
        new = [mn, vn]
    tw.p[m] = pn
    for x, y in zip(tw.state, new):
        x[m] = y


def assert_twin(tw, opt, what):
    assert same_np(opt.flat.data.cpu().numpy(), tw.p), (what, "weights")
    for k, x in zip(opt.STATE, tw.state):
        got = getattr(opt, k).cpu().numpy()
        assert same_np(got, x), (what, k, int((got.view(np.int32) != x.view(np.int32)).sum()))


@pytest.mark.parametrize("decayed", [False, True])
@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_d_three_steps_through_construct_optimizer(method, decayed):
    """(on the parent commit construct_optimizer raises NotImplementedError for either method)"""
    from svit_amd import optim
    x, y = batch()
    cfg, model = build()
    opt = optim.construct_optimizer(model, solver_cfg(cfg, method, decayed=decayed))
    assert type(opt) is {"sgd": optim.GuardedClipSGD, "adam": optim.GuardedClipAdam}[method]
    assert (opt.lr_segments is not None) == decayed
    tw = host_twin(opt)
    assert bool(tw.inside.all())
    for i in range(3):
        optim.set_lr(opt, LR[method] * (i + 1))
        g = fwd_bwd(model, x, y).cpu().numpy()
        opt.step()
        torch.cuda.synchronize()
        st = opt.stats()
        assert st["applied"] == i + 1 and 0.0 < st["clip_coef"] <= 1.0
        host_step(tw, opt, g, st)
        assert_twin(tw, opt, "step %d" % (i + 1))
    assert opt.step_count == 3


@pytest.mark.parametrize("decayed", [False, True])
def test_d_sgd_first_step_moves_every_range_by_its_own_rate(decayed):
    """no clipping, momentum without nesterov: step 1 is w - lr_eff (g + wd w).  |dw| is compared in float64 with the
    fp32 roundings allowed for: w wd, g + w wd and gi lr_eff, each 2^-24 relative to |g| + wd |w| at most, and the
    stored weight, half an ulp of the result: 2^-24 (|w| + lr_eff (|g| + wd |w|)), doubled for a result in the binade
    above w's.  In all 4 x 2^-24 lr_eff (|g| + wd |w|) + 2^-23 |w|."""
    from svit_amd import optim
    x, y = batch()
    cfg, model = build()
    opt = optim.construct_optimizer(model, solver_cfg(cfg, "sgd", clip=None, decayed=decayed, wd=0.05, nesterov=False))
    flat = model.flat
    w0 = flat.data.cpu().double()
    g = fwd_bwd(model, x, y).cpu().double()
    opt.step()
    torch.cuda.synchronize()
    st = opt.stats()
    assert st["applied"] == 1 and st["clip_coef"] == 1.0
    dw = (flat.data.cpu().double() - w0).abs()
    segs, scales = opt._ranges()
    rates = set()
    for i, (a, b) in enumerate(segs.tolist()):
        c = np.float32(1.0) if scales is None else scales[i]
        lr_eff = float(np.float32(LR["sgd"]) * c)
        wd = 0.05 if a < flat.n_decay else 0.0
        gi = (g[a:b] + float(np.float32(wd)) * w0[a:b]).abs()
        want = lr_eff * gi
        slack = 4 * 2.0 ** -24 * lr_eff * (g[a:b].abs() + wd * w0[a:b].abs()) + 2.0 ** -23 * w0[a:b].abs() + 2.0 ** -149
        over = (dw[a:b] - want).abs() - slack
        assert float(over.max()) <= 0.0, (a, b, float(c), float(over.max()))
        if float(gi.max()) > 1e-6:
            rates.add(float(c))
    assert len(rates) >= (3 if decayed else 1)
    if decayed:
        assert float(np.float32(L.DECAY ** 17)) in rates and float(np.float32(1.0)) in rates


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
    return [n for n in names if n.startswith(("svit_step_guard", "svit_adamw_step", "svit_sgd_", "svit_adam_"))]


def _state_pairs(a, b):
    return [("weights", a.flat.data, b.flat.data)] + [(k, getattr(a, k), getattr(b, k)) for k in a.STATE]


def test_e_graphed_step_replays_the_sgd_tail(monkeypatch):
    from svit_amd import optim
    from svit_amd.graph import GraphedTrainStep
    poison = torch.ones(1, device=DEV)

    def loss_fun(p, e, y):
        return torch.nn.functional.cross_entropy(p, y) * poison

    x, y = batch()
    cfg_g, mg = build()
    cfg_e, me = build()
    og = optim.construct_optimizer(mg, solver_cfg(cfg_g, "sgd"))
    oe = optim.construct_optimizer(me, solver_cfg(cfg_e, "sgd"))
    assert type(og) is optim.GuardedClipSGD
    w0 = mg.flat.data.clone()
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(mg, loss_fun, [x], y, optimizer=og))
    assert _tail(names) == ["svit_step_guard", "svit_sgd_step_guarded"]
    assert names.index("svit_sgd_step_guarded") == names.index("svit_step_guard") + 1
    torch.cuda.synchronize()
    assert same(mg.flat.data, w0) and og.stats()["applied"] == 0 and int(torch.count_nonzero(og.momentum_buffer)) == 0

    def eager():
        oe.zero_grad()
        logits, extra = me([x], {})
        loss = loss_fun(logits, extra, y)
        loss.backward()
        oe.step()
        return loss.detach()

    def compare(what):
        torch.cuda.synchronize()
        for name, a, b in _state_pairs(og, oe) + [("grad", mg.flat.grad, me.flat.grad)]:
            assert same(a, b), (what, name, int((bits(a) != bits(b)).sum()))
        assert og.stats() == oe.stats(), what

    # the first replay is poisoned: step 1 is dropped, and the replay after it is the "first" one in the graph too
    poison.fill_(float("nan"))
    step([x], y)
    eager()
    compare("poisoned step")
    assert same(mg.flat.data, w0) and og.stats()["skipped"] == 1 and og.stats()["applied"] == 0
    poison.fill_(1.0)
    for i in range(3):
        optim.set_lr(og, LR["sgd"] * (i + 1))
        optim.set_lr(oe, LR["sgd"] * (i + 1))
        lg, _ = step([x], y)
        le = eager()                    # (steps at the lr set_lr just wrote: equality says it reached the replay)
        assert same(lg, le)
        compare("step %d" % (i + 1))
    assert og.stats()["applied"] == 3 and not same(mg.flat.data, w0)
    assert int(torch.count_nonzero(og.momentum_buffer)) > 0


def test_e_accumulated_step_k2_reproducible():
    """k = 2 micro-steps under SVIT.REPRODUCIBLE = one guarded SGD step at grad_scale 1/2 on the accumulated buffer"""
    from svit_amd import optim
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    _, model = build("reproducible")
    flat = model.flat
    A, B = batch(), batch("B")
    kw = dict(lr=LR["sgd"], momentum=0.9, nesterov=True, weight_decay=1e-4, clip_grad_l2norm=1.0)
    opt = optim.GuardedClipSGD(model, **kw)
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
    twin = optim.GuardedClipSGD(holder, grad_scale=0.5, **kw)
    twin.step()
    torch.cuda.synchronize()
    for what, a, b in _state_pairs(opt, twin):
        assert same(a, b), (what, int((bits(a) != bits(b)).sum()))
    assert opt.stats() == twin.stats()


def test_e_accumulated_step_k2_replays_equal_the_eager_accumulated_steps():
    """AccumulatedTrainStep(k = 2, GuardedClipSGD) under SVIT.REPRODUCIBLE against the eager micro-steps + optimizer.step()
    (train.accumulate_step) on a second model: a first call with a poisoned micro-step -- the whole step is dropped and
    the next one is still "first" -- then three calls with lr changes (the second and third take the momentum branch).
    Weights, momentum buffer, gradient buffer, losses and stats() bit for bit after every call."""
    from svit_amd import optim, train
    from svit_amd.graph import AccumulatedTrainStep, GraphedTrainStep
    A, B, C = batch(), batch("B"), batch("C")
    bad = P.frames(2, 4, 64, tag="clipB").cuda()
    bad[1, 2, 3, 17, 40] = float("nan")                     # the input clip of micro-step 2 of 2
    cfg_g, mg = build("reproducible")
    cfg_e, me = build("reproducible")
    og = optim.construct_optimizer(mg, solver_cfg(cfg_g, "sgd"))
    oe = optim.construct_optimizer(me, solver_cfg(cfg_e, "sgd"))
    assert type(og) is optim.GuardedClipSGD and og.momentum == 0.9 and og.nesterov
    micro = GraphedTrainStep(mg, ce, [A[0]], A[1], accumulate=True)
    step = AccumulatedTrainStep(mg, [micro, micro], og)
    w0 = mg.flat.data.clone()

    def both(batches, what):
        batches = [([x], y) for x, y in batches]
        lg = [l.clone() for l in step(batches)]
        le = train.accumulate_step(me, [ce, ce], batches, oe)
        torch.cuda.synchronize()
        for name, a, b in _state_pairs(og, oe) + [("grad", mg.flat.grad, me.flat.grad)]:
            assert same(a, b), (what, name, int((bits(a) != bits(b)).sum()))
        for i, (a, b) in enumerate(zip(lg, le)):
            assert same(a.reshape(()), b.reshape(())), (what, "loss of micro-step %d" % i)
        assert og.stats() == oe.stats(), what
        assert og.grad_scale == oe.grad_scale == 1.0          # the 1/2 was this step's alone
        return og.stats()

    st = both([A, (bad, B[1])], "poisoned call")
    assert (st["applied"], st["skipped"]) == (0, 1) and same(mg.flat.data, w0)
    assert int(torch.count_nonzero(og.momentum_buffer)) == 0 and not bool(torch.isfinite(mg.flat.grad).all())
    buffers = []
    for i, batches in enumerate(([A, B], [C, A], [B, C])):
        optim.set_lr(og, LR["sgd"] * (i + 1))
        optim.set_lr(oe, LR["sgd"] * (i + 1))
        st = both(batches, "call %d after the poisoned one" % (i + 1))
        assert (st["applied"], st["skipped"], st["consecutive_skipped"]) == (i + 1, 1, 0)
        buffers.append(og.momentum_buffer.clone())
        if i == 0:
            # still "first": the buffer is gi = g * coef + wd w itself (coef carries the 1/2 of k = 2)
            flat = mg.flat
            gi = flat.grad * st["clip_coef"]
            wd = torch.zeros_like(gi)
            wd[:flat.n_decay] = og.param_groups[0]["weight_decay"]
            gi = torch.where(wd != 0, gi + w0 * wd, gi)
            assert 0.0 < st["clip_coef"] <= 0.5 and same(og.momentum_buffer, gi)
    assert not same(buffers[0], buffers[1]) and not same(buffers[1], buffers[2]) and not same(mg.flat.data, w0)


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_f_cut_4_and_decay_combine(method):
    """one table launch = per scale class one launch of the same kernel, scales NULL, the record's lr premultiplied"""
    from svit_amd import ops, optim
    from svit_amd.optim import pack_step_host
    cut = 4
    x, y = batch()
    cfg, model = build()
    flat = model.flat
    w0 = flat.data.clone()
    model.freeze_below(cut)
    opt = optim.construct_optimizer(model, solver_cfg(cfg, method, decayed=True, wd=0.05))
    tsegs = model.trainable_segments(cut)
    assert opt.cut == cut and opt.lr_segments is not None
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    L.check_table(opt.lr_segments, opt.lr_scales, L.element_scales(flat.slots, names, flat.total, L.DECAY, ()), flat.n_decay)
    inside = torch.from_numpy(_inside(tsegs.tolist(), flat.total)).to(DEV)
    tw = types.SimpleNamespace(p=w0.clone(), state=[torch.zeros_like(w0) for _ in opt.STATE],
                               rec=torch.zeros(12, dtype=torch.int32, device=DEV), ws=torch.zeros(1024, device=DEV))
    lr0 = LR[method]
    for i in range(2):
        lr = lr0 * (i + 1)
        optim.set_lr(opt, lr)
        g = fwd_bwd(model, x, y)
        opt.step()
        host = torch.from_numpy(pack_step_host((lr, lr), (0.05, 0.0), 1.0, None, 1.0)).to(DEV)
        ops.step_guard_seg(g, tsegs, host, tw.rec, opt.bias_table, tw.ws)
        for c in sorted(set(float(s) for s in opt.lr_scales)):
            mine = np.ascontiguousarray(opt.lr_segments[opt.lr_scales == np.float32(c)])
            le = float(np.float32(lr) * np.float32(c))
            host_c = torch.from_numpy(pack_step_host((le, le), (0.05, 0.0), 1.0, None, 1.0)).to(DEV)
            if method == "sgd":
                ops.sgd_step_guarded(tw.p, g, tw.state[0], flat.n_decay, mine, None, host_c, tw.rec, opt.momentum,
                                     opt.dampening, opt.nesterov)
            else:
                ops.adam_step_guarded(tw.p, g, tw.state[0], tw.state[1], flat.n_decay, mine, None, host_c, tw.rec,
                                      *opt.betas, opt.eps)
        torch.cuda.synchronize()
        pairs = [("weights", flat.data, tw.p), ("record", opt.dev_rec, tw.rec)]
        pairs += [(k, getattr(opt, k), s) for k, s in zip(opt.STATE, tw.state)]
        for what, a, b in pairs:
            assert same(a, b), ("step %d" % (i + 1), what, int((bits(a) != bits(b)).sum()))
    assert opt.step_count == 2
    assert same(flat.data[~inside], w0[~inside]), "a frozen weight moved"
    assert not same(flat.data[inside], w0[inside])
    for k in opt.STATE:
        assert int(torch.count_nonzero(getattr(opt, k)[~inside])) == 0


@pytest.mark.parametrize("method", ["sgd", "adam"])
def test_g_checkpoint_round_trip(tmp_path, method):
    from svit_amd import checkpoint, optim
    x, y = batch()

    def make():
        cfg, model = build()
        return cfg, model, optim.construct_optimizer(model, solver_cfg(cfg, method, decayed=True))

    def one_step(model, opt):
        opt.zero_grad()
        logits, _ = model([x], {})
        torch.nn.functional.cross_entropy(logits, y).backward()
        opt.step()
        torch.cuda.synchronize()

    cfg, model, opt = make()
    for _ in range(2):
        one_step(model, opt)
    path = checkpoint.save_checkpoint(str(tmp_path), model, opt, 3, cfg)
    ck = torch.load(path, map_location="cpu", weights_only=False)["optimizer_state"]
    assert len(ck["param_groups"]) > 2 and all("layer_decay" in g for g in ck["param_groups"]) and len(ck["state"]) == 405
    assert sorted(ck["state"][0]) == (["momentum_buffer"] if method == "sgd" else ["exp_avg", "exp_avg_sq", "step"])
    cfg2, model2, opt2 = make()
    model2.flat.data.zero_()
    assert checkpoint.load_checkpoint(path, model2, data_parallel=False, optimizer=opt2) == 3
    assert same(model2.flat.data, model.flat.data)
    for what, a, b in _state_pairs(opt, opt2):
        assert same(a, b), what
    # SGD's counter is at least 1 (the resumed step is not "first"), Adam's is the checkpoint's
    assert opt2.step_count == (1 if method == "sgd" else 2)
    one_step(model, opt)
    one_step(model2, opt2)
    for what, a, b in _state_pairs(opt, opt2):
        assert same(a, b), ("the step after the reload", what, int((bits(a) != bits(b)).sum()))
    assert opt2.step_count == opt2.stats()["applied"] == (2 if method == "sgd" else 3)


def test_h_adamw_is_untouched(monkeypatch):
    """a capture built through construct_optimizer with OPTIMIZING_METHOD adamw issues today's launches: the body of a
    capture without an optimizer, then the guard and the plain guarded AdamW; nothing of solver.hip is called"""
    from svit_amd import optim
    from svit_amd.graph import GraphedTrainStep
    x, y = batch()
    cfg, ma = build()
    _, mb = build()
    s = cfg.SOLVER
    assert s.OPTIMIZING_METHOD == "adamw"
    s.BASE_LR, s.WEIGHT_DECAY, s.CLIP_GRAD_L2NORM = 1e-3, 0.05, 1.0
    cfg.SVIT.GUARDED_STEP = True
    opt = optim.construct_optimizer(ma, cfg)
    assert type(opt) is optim.GuardedClipAdamW and opt.STATE == ("exp_avg", "exp_avg_sq")
    _, bare = _trace_names(monkeypatch, lambda: GraphedTrainStep(mb, ce, [x], y))
    step, names = _trace_names(monkeypatch, lambda: GraphedTrainStep(ma, ce, [x], y, optimizer=opt))
    assert _tail(bare) == [] and _tail(names) == ["svit_step_guard", "svit_adamw_step_guarded"]
    assert names.index("svit_adamw_step_guarded") == names.index("svit_step_guard") + 1
    assert [n for n in names if n not in _tail(names)] == bare
    assert not [n for n in names if n.startswith(("svit_sgd_", "svit_adam_"))]
    step([x], y)
    torch.cuda.synchronize()
    sd = opt.state_dict()
    assert [list(g) for g in sd["param_groups"]] == [
        ["lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable", "differentiable",
         "fused", "decoupled_weight_decay", "params"]] * 2
    assert all(g["decoupled_weight_decay"] is True for g in sd["param_groups"])
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and len(sd["state"]) == 405
