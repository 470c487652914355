"""Reproducible training at full speed (Engine.reproducible / cfg.SVIT.REPRODUCIBLE): the weight-gradient GEMMs keep
their row splits but flush into slabs that a second launch sums in split order (svit_gemm_tn_grouped_slab).  The
kernel against fp32 math with the bar of the atomic form, bit-equality run to run at kernel, step, optimizer-step and
graph-replay level, and a check that the steps under test really took the slab path.  Needs a real MI355X."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import procedural as P
from tests import smoke_impl as S

DEV = "cuda"
BF16 = torch.bfloat16
# the eleven shapes of tests/test_kernels_gpu.py::_tn_grouped_case, and the block-0 problem of the bench step
# (8 clips of 16x224^2: M = 201 224 rows, so many row splits meet in every dW element)
SHAPES = [(1000, 288, 96), (4100, 384, 1536), (70, 96, 441), (13064, 384, 384), (333, 40, 96),
          (64, 3072, 768), (2000, 1152, 384), (5000, 96, 96), (129, 128, 96), (8000, 64, 96),
          (700, 768, 768)]
BLOCK0 = (201224, 384, 96)
ATOMIC_CALLS = ("svit_gemm_tn", "svit_gemm_tn_grouped", "svit_gemm_tn_grouped_ex")
SLAB_CALL = "svit_gemm_tn_grouped_slab"


@pytest.fixture(scope="module")
def ops():
    from svit_amd import hip
    from svit_amd import ops as o
    hip.load()
    return o


def rnd(name, shape, amp=1.0, dtype=torch.float32):
    return P.tensor("rw:" + name, shape, amp).to(DEV).to(dtype)


def rel_err(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-12))


def _slab_case(ops, shapes, repeats=3):
    """the operands of _tn_grouped_case (row-strided a, padded ldb, every third problem without a bias, dW pre-filled
    with 0.5, dbias with 0.25, dW rows wider than K on every fourth problem), run `repeats` times from identical
    dW / dbias: parity with fp32 math at the bar of the atomic kernel (rel_err < 2e-4), then bit-equality pairwise"""
    ins, refs = [], []
    for i, (M, N, K) in enumerate(shapes):
        wide = rnd("ga%d" % i, (M, N + 16), 1.0, BF16)
        a = wide[:, 8:8 + N]                                  # row-strided view
        b = rnd("gb%d" % i, (M, (K + 7) // 8 * 8), 1.0, BF16)
        ins.append((a, b, i % 3 != 2, K + 5 if i % 4 == 1 else K))
        refs.append((a.float().t() @ b.float()[:, :K] + 0.5,
                     None if i % 3 == 2 else a.float().sum(0) + 0.25))
    runs = []
    for _ in range(repeats):
        probs = []
        for (a, b, bias, lddw), (M, N, K) in zip(ins, shapes):
            dw = torch.full((N, lddw), 0.5, device=DEV)[:, :K]          # lddw > K: the columns beyond stay untouched
            probs.append((a, b, dw, torch.full((N,), 0.25, device=DEV) if bias else None))
        ops.gemm_tn_grouped_slab(probs)
        torch.cuda.synchronize()
        runs.append(probs)
    for i, ((_, _, dw, db), (rw, rb)) in enumerate(zip(runs[0], refs)):
        ew = rel_err(dw, rw)
        eb = None if db is None else rel_err(db, rb)
        print("slab problem %d %s: rel_err dW %.3g dbias %s" % (i, shapes[i], ew, eb))
        assert ew < 2e-4, (i, shapes[i], ew)
        if db is not None:
            assert eb < 2e-4, (i, shapes[i], eb)
        if dw.stride(0) > dw.shape[1]:
            pad = torch.as_strided(dw, (dw.shape[0], dw.stride(0) - dw.shape[1]), dw.stride(), dw.shape[1])
            assert float((pad - 0.5).abs().max()) == 0.0, (i, "columns past K were written")
    for r in runs[1:]:
        for i, ((_, _, dw0, db0), (_, _, dw, db)) in enumerate(zip(runs[0], r)):
            assert torch.equal(dw0, dw), (i, shapes[i], int((dw0 != dw).sum()))
            if db0 is not None:
                assert torch.equal(db0, db), (i, shapes[i], int((db0 != db).sum()))


@pytest.mark.parametrize("tile_mode", [1, 0, 2])
@pytest.mark.parametrize("count", [1, 5, 11])
def test_slab_gemm_parity_and_bit_equality(ops, count, tile_mode):
    from svit_amd import hip
    lib = hip.load()
    lib.svit_debug_set_tn_tile.restype, lib.svit_debug_set_tn_tile.argtypes = C.c_int32, [C.c_int32]
    lib.svit_debug_set_tn_tile(tile_mode)
    try:
        _slab_case(ops, SHAPES[:count])
    finally:
        lib.svit_debug_reset()


def test_slab_gemm_block0_shape_many_splits(ops):
    """M = 201 224: the planner cuts the rows into many splits, all of which meet in every element of the 384 x 96 dW"""
    from svit_amd import hip
    arr, _ = ops._tn_problem_array([(rnd("s0a", (64, 384), 1.0, BF16), rnd("s0b", (64, 96), 1.0, BF16),
                                     torch.zeros(384, 96, device=DEV), None)])
    arr[0].M = BLOCK0[0]
    need = hip.load().svit_gemm_tn_grouped_workspace(arr, 1)
    splits = need // (128 * 96 * 3)          # three n-tiles of at most 128 x 96 slab floats per split
    print("block-0 problem: workspace %d floats, >= %d row splits" % (need, splits))
    assert splits >= 8, (need, splits)
    _slab_case(ops, [BLOCK0])


def test_slab_gemm_more_problems_than_one_group_and_explicit_workspace(ops):
    """past SVIT_TN_GROUP_MAX problems the (GEMM, reduce) pairs reuse the workspace in stream order; a caller's own
    workspace of exactly the queried size serves, one float less is refused"""
    from svit_amd import hip
    shapes = (SHAPES + SHAPES)[:19]
    _slab_case(ops, shapes, repeats=2)
    a, b = rnd("xa", (3000, 200), 1.0, BF16), rnd("xb", (3000, 96), 1.0, BF16)
    dw, db = torch.zeros(200, 96, device=DEV), torch.zeros(200, device=DEV)
    arr, _ = ops._tn_problem_array([(a, b, dw, db)])
    need = ops.gemm_tn_slab_workspace(arr, 1)
    ops.gemm_tn_grouped_slab([(a, b, dw, db)], ws=torch.empty(need, device=DEV))
    assert rel_err(dw, a.float().t() @ b.float()) < 2e-4 and rel_err(db, a.float().sum(0)) < 2e-4
    with pytest.raises(hip.SvitHipError):
        ops.gemm_tn_grouped_slab([(a, b, dw, db)], ws=torch.empty(need - 1, device=DEV))


# ------------------------------------------------------------------------------ steps ----
def _eager(model, x, y):
    model.flat.grad.zero_()
    logits, _ = model([x], {})
    loss = torch.nn.functional.cross_entropy(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return model.flat.grad.clone()


def _first_diff(model, u, v):
    bad = (u != v).nonzero()
    if len(bad) == 0:
        return None
    i = int(bad[0])
    for n, (off, numel, _) in model.flat.slots.items():
        if off <= i < off + numel:
            return n, len(bad)
    return "padding", len(bad)


def _traced_calls(fn):
    from svit_amd import hip
    hip.start_trace()
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        trace = hip.stop_trace()
    return [t[0] for t in trace]


def test_video_step_is_bit_reproducible_at_split_speed():
    """Mirror of test_overlap_wgrad_is_bit_equal_to_stream_order with `reproducible` in place of `deterministic`: the
    flat gradient of 2 clips of 8x224^2 is bit-equal over two stream-ordered and two overlapped eager steps, agrees
    with the unsplit `deterministic` mode to the bar that test uses between modes (cosine > 0.9999), and one AdamW
    step from the same state gives bit-equal weights."""
    from svit_amd import optim
    cfg, model, spec, sd = S.build_hip_model(8, 224)
    eng = model.engine
    assert eng.reproducible is False            # opt-in
    x, y = P.frames(2, 8, 224).cuda(), P.labels(2).cuda()
    eng.reproducible = True

    def run(overlap):
        eng.overlap_wgrad = overlap
        return _eager(model, x, y)

    a, b = run(False), run(False)
    c, d = run(True), run(True)
    eng.overlap_wgrad = False
    assert _first_diff(model, a, b) is None, ("reproducible mode not reproducible", _first_diff(model, a, b))
    assert _first_diff(model, a, c) is None, ("overlap changed the gradients", _first_diff(model, a, c))
    assert _first_diff(model, a, d) is None, ("overlap changed the gradients", _first_diff(model, a, d))
    # `deterministic` keeps its meaning and wins when both are set: no slab call, the unsplit atomic form
    eng.deterministic = True
    names = _traced_calls(lambda: _eager(model, x, y))
    assert SLAB_CALL not in names and "svit_gemm_tn_grouped_ex" in names
    e = _eager(model, x, y)
    eng.deterministic = False
    cos = S.cosine(a, e)
    print("reproducible vs deterministic: cosine %.7f" % cos)
    assert cos > 0.9999
    # one optimizer step after each of two reproducible steps from the same state
    cfg.SOLVER.CLIP_GRAD_L2NORM = 1.0
    w0 = model.flat.data.clone()
    weights = []
    for _ in range(2):
        model.flat.data.copy_(w0)
        opt = optim.construct_optimizer(model, cfg)
        optim.set_lr(opt, 2e-4)
        _eager(model, x, y)
        opt.step()
        torch.cuda.synchronize()
        weights.append(model.flat.data.clone())
    assert not torch.equal(weights[0], w0)
    assert _first_diff(model, weights[0], weights[1]) is None, _first_diff(model, weights[0], weights[1])
    eng.reproducible = False


def test_graph_replay_is_bit_reproducible():
    """two replays of a captured reproducible step from the same parameter state (stochastic depth and dropout at 0)
    leave bit-equal gradients; the slab workspace was sized in the warm-up pass, so the capture allocated nothing"""
    from svit_amd.graph import GraphedTrainStep
    cfg, model, spec, sd = S.build_hip_model(8, 224)
    model.engine.reproducible = True
    x, y = P.frames(2, 8, 224).cuda(), P.labels(2).cuda()
    step = GraphedTrainStep(model, lambda p, e, l: torch.nn.functional.cross_entropy(p, l), [x], y)
    assert step.n_graphs >= 1
    grads = []
    for _ in range(3):
        step([x], y)
        torch.cuda.synchronize()
        grads.append(model.flat.grad.clone())
    assert float(grads[0].abs().max()) > 0
    assert _first_diff(model, grads[0], grads[1]) is None, _first_diff(model, grads[0], grads[1])
    assert _first_diff(model, grads[0], grads[2]) is None, _first_diff(model, grads[0], grads[2])
    # and the replay computes what the eager reproducible step computes (same kernels, same order)
    eager = _eager(model, x, y)
    assert _first_diff(model, grads[0], eager) is None, _first_diff(model, grads[0], eager)


def test_image_rank_step_is_bit_reproducible():
    """One HAOG-loss step on still images, set up as test_image_rank_step_parity_vs_oracle sets it up, with 20 images:
    B*T*O = 80 object rows = three 32-row chunks of the head's box / contact weight gradients.  Those chunks meet in
    fp32 atomics in the default step (csrc/head.hip); three addends commit in any order, so their sum is not fixed --
    `reproducible` therefore runs that part of the head backward with one block per channel chunk walking all rows
    in order (svit_head_bwd_args.ordered), which this test covers together with the stand-alone weight-gradient
    GEMMs of a T = 1 pass (patch embed, interpolated rel-pos tables), which go through the slab form as one-problem
    groups."""
    from svit_amd import losses
    batch = 20
    cfg, model, spec, sd = S.build_hip_model(4, 64)
    assert batch * 1 * cfg.SVIT.O > 2 * 32
    model.engine.reproducible = True
    x = P.frames(batch, 1, 64).cuda()
    meta = {k: v.cuda() for k, v in P.haog_meta(batch).items()}
    fn = losses.VideoImageLoss(cfg, is_video_rank=False)

    def run():
        model.flat.grad.zero_()
        logits, extra = model([x], {})
        loss = fn.total(fn(logits, extra, None, meta))
        loss.backward()
        torch.cuda.synchronize()
        return model.flat.grad.clone()

    names = _traced_calls(run)
    assert SLAB_CALL in names and not [n for n in names if n in ATOMIC_CALLS], sorted(set(names))
    a, b, c = run(), run(), run()
    assert float(a.abs().max()) > 0
    assert _first_diff(model, a, b) is None, _first_diff(model, a, b)
    assert _first_diff(model, a, c) is None, _first_diff(model, a, c)
    # the ordered head sums the same products: against the default step to the bar between modes
    model.engine.reproducible = False
    cos = S.cosine(a, run())
    print("image rank, reproducible vs default: cosine %.7f" % cos)
    assert cos > 0.9999


def test_reproducible_step_takes_the_slab_path_and_the_default_step_does_not():
    """setting an unknown attribute on a Python object succeeds silently: without this check the step tests above
    could pass without the feature, by luck"""
    cfg, model, spec, sd = S.build_hip_model(4, 64)
    x, y = P.frames(2, 4, 64).cuda(), P.labels(2).cuda()
    default = _traced_calls(lambda: _eager(model, x, y))
    assert SLAB_CALL not in default
    n_grouped = default.count("svit_gemm_tn_grouped")
    assert n_grouped >= 1 and default.count("svit_gemm_tn") >= 1       # (patch embed: the stand-alone call)
    model.engine.reproducible = True
    repro = _traced_calls(lambda: _eager(model, x, y))
    assert not [n for n in repro if n in ATOMIC_CALLS], sorted(set(repro))
    assert repro.count(SLAB_CALL) >= n_grouped + default.count("svit_gemm_tn")
    # the public switch: read where the engine is created
    cfg.SVIT.REPRODUCIBLE = True
    from svit_amd.model import build_model
    m2 = build_model(cfg)
    assert m2.engine.reproducible is True
