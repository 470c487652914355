"""Fused attention (svit_attn_fwd / svit_attn_bwd) against the float64 reference of tests/attn_reference.py, on the
ATTENTION-ONLY part of the output, with bars derived from the dense rounding-point emulation (3 x its own distance
from the reference; tests/test_attention_reference_cpu.py proves that every mutant lies at >= 3 x those bars).

Per case and input family (flat / peaked scores, attn_reference.make_inputs):
  forward   attention-only `ctx - residual` (peaked), lse2 at 1e-3, and the probability read-out: one launch per
            block of 96 keys with v = 256 * one-hot, whose `ctx - residual` IS P[:, block] -- element for element
            against the float64 softmax, so a mis-addressed key, a mask slip or a rescale slip is an O(1) error at
            a known (batch, head, row, key), which the assertion message names.  Kernels: the one svit_attn_fwd
            picks (short / w4 = 4 waves, 2 stages / w8 = 8 waves, 3 stages) and, where that is the short-key
            kernel, also the generic one (svit_attn_debug_set(3, 0)).
  backward  dqa[..., :96], dqa[..., 96:96+J], dk, dv, each on its own, from the ctx / lse2 of the GPU forward;
            dkv kernel by heuristic with the automatic split plan, and both forms forced (halves 1 / 2) with the
            automatic plan and q_splits = 3.  dqa past column 96 + J is exactly zero (svit_hip.h).
The ids name forward form, k-step count (KSU 7..10) of the forward and of the backward, the dkv form and the plan.

Measured on an MI355X, worst got / bar over all cases of a path (evidence of the margin, never an input to a bar):
  forward form              KSU   attn  read-out  lse2
  short                       7   0.36    0.43    0.34
  short                       8   0.33    0.34    0.27
  w4                          7   0.34    0.41    0.13
  w4                          8   0.37    0.43    0.11
  w4                          9   0.34    0.36    0.02
  w4                         10   0.34    0.43    0.08
  w4 (forced on Nk <= 64)     7   0.36    0.43    0.34
  w4 (forced on Nk <= 64)     8   0.33    0.34    0.27
  w8                          8   0.38    0.43    0.09
  w8                          9   0.36    0.36    0.04
  w8                         10   0.37    0.45    0.11
  backward KSU  dkv form    dqa[:96]  dqa[96:96+J]  dk    dv
         7      halves1     0.43      0.46          0.50  0.41
         7      halves2     0.43      0.46          0.50  0.41
         7      heuristic   0.43      0.46          0.50  0.41
         8      halves1     0.36      0.35          0.36  0.45
         8      halves2     0.36      0.35          0.36  0.45
         8      heuristic   0.36      0.35          0.36  0.45
         9      halves1     0.43      0.46          0.36  0.41
         9      halves2     0.43      0.46          0.36  0.41
         9      heuristic   0.43      0.46          0.36  0.41
        10      halves1     0.48      0.49          0.55  0.41
        10      halves2     0.48      0.49          0.55  0.41
        10      heuristic   0.48      0.49          0.55  0.41
(a correct kernel sits at 1.0 - 1.7 x the emulation's floor, i.e. 0.33 - 0.55 of its bar; the forced dkv forms and
the q_splits = 3 plan give the same maxima as the heuristic to the digits shown)
"""
import ctypes as C
import functools

import pytest
import torch

from tests import attn_reference as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
FAMILIES = ("flat", "peaked")
MULTI_PART_CASES = ("step_blocks4_13", "frames_J15")       # where the automatic plan must cut the query range


@pytest.fixture(scope="module")
def ops():
    from svit_amd import ops as o
    from svit_amd import hip
    hip.load()
    return o


def _lib():
    from svit_amd import hip
    lib = hip.load()
    lib.svit_attn_debug_set.restype, lib.svit_attn_debug_set.argtypes = C.c_int32, [C.c_int32, C.c_int32]
    return lib


@functools.lru_cache(maxsize=4)
def _inputs(name, family):
    return A.make_inputs(A.CASE_BY_NAME[name], family)


def _report(record_property, ratios, where):
    """ratios {tensor: (got, bar)}: every got / bar goes to the report; all of them must be <= 1."""
    lines = []
    for t, (got, bar) in ratios.items():
        record_property(t, "%.3f (got %.3g / bar %.3g)" % (got / bar, got, bar))
        lines.append("%s: got %.4g / bar %.4g = %.2f%s" % (t, got, bar, got / bar, where.get(t, "")))
    print("\n".join(lines))
    assert all(got <= bar for got, bar in ratios.values()), "\n" + "\n".join(lines)


def _fwd_params():
    out = []
    for c in A.CASES:
        for fam in FAMILIES:
            out.append(pytest.param(c.name, fam, False, id="%s-%s" % (c.fwd_id(), fam)))
            if c.form == "short":        # the generic kernel on the same short inputs
                out.append(pytest.param(c.name, fam, True,
                                        id="%s-fwd_generic_w4_ksu%d-tiles1-%s" % (c.name, c.fwd_ksu, fam)))
    return out


@pytest.mark.parametrize("name,family,generic", _fwd_params())
def test_forward_and_probability_read_out(ops, name, family, generic, record_property):
    case = A.CASE_BY_NAME[name]
    B, h, Nq, Nk, J = case.B, case.h, case.Nq, case.Nk, case.J
    qa, ka, v, _ = _inputs(name, family)
    bars = A.case_bars(name, family)
    qd, kd = qa.to(DEV), ka.to(DEV)
    nblk = (Nk + A.READOUT_BLOCK - 1) // A.READOUT_BLOCK
    lib = _lib()
    try:
        if generic:
            assert lib.svit_attn_debug_set(3, 0) == 0
        ctx, lse2 = ops.attn_fwd(qd, kd, v.to(DEV), A.SCALE, bias_cols=J)
        reads = []
        for blk in range(nblk):
            vb = A.readout_v(Nk, blk).to(DEV).expand(B, h, Nk, A.HD).contiguous()
            cb, lb = ops.attn_fwd(qd, kd, vb, A.SCALE, bias_cols=J)
            assert torch.equal(lb, lse2)          # the row sum does not depend on v
            reads.append(cb.cpu())
        torch.cuda.synchronize()
    finally:
        lib.svit_attn_debug_set(3, 1)
    ctx, lse2 = ctx.cpu(), lse2.cpu()
    assert bool(torch.isfinite(ctx.float()).all()) and bool(torch.isfinite(lse2).all())
    ms, worst, where = A.Measure(), 0.0, {}
    for b, hd in A.slices(B, h):
        attn, res, lse_ref, P = A.reference_fwd_2d(qa[b, hd], ka[b, hd], v[b, hd], J)
        if family == "peaked":
            ms.add("attn", A.ctx_slice(ctx, b, hd).to(F64) - res, attn)
        ms.add("lse2", lse2[b, hd], lse_ref)
        got = torch.cat([(A.ctx_slice(cb, b, hd).to(F64) - res) / A.READOUT_GAIN for cb in reads], 1)
        ref = torch.cat([P, torch.zeros(Nq, nblk * A.READOUT_BLOCK - Nk, dtype=F64)], 1)   # columns past Nk read nothing
        ms.add("readout", got, ref)
        err = (got - ref).abs()
        if float(err.max()) > worst:
            worst = float(err.max())
            r, k = divmod(int(err.argmax()), err.shape[1])
            where["readout"] = "  (worst at batch %d head %d row %d key %d: got %.4g, P %.4g)" % (
                b, hd, r, k, float(got[r, k]), float(ref[r, k]))
    rel = ms.rel()
    _report(record_property, {t: (rel[t], bars[t]) for t in rel}, where)


def _bwd_params():
    out = []
    for c in A.CASES:
        for fam in FAMILIES:
            for halves, tag in ((0, "dkv_heuristic-auto_plan"), (1, "dkv_halves1"), (2, "dkv_halves2")):
                multi = "_multi_part" if (halves == 0 and c.name in MULTI_PART_CASES) else ""
                out.append(pytest.param(c.name, fam, halves,
                                        id="%s-bwd_ksu%d-dq-%s%s-%s" % (c.name, c.bwd_ksu, tag, multi, fam)))
    return out


@functools.lru_cache(maxsize=2)
def _bwd_reference(name, family):
    case = A.CASE_BY_NAME[name]
    qa, ka, v, dctx = _inputs(name, family)
    return A.reference_bwd(qa, ka, v, dctx, case.J)


@pytest.mark.parametrize("name,family,halves", _bwd_params())
def test_backward(ops, name, family, halves, record_property):
    case = A.CASE_BY_NAME[name]
    J, je = case.J, A.jeff(case.DA, case.J)
    qa, ka, v, dctx = _inputs(name, family)
    bars = A.case_bars(name, family)
    ref = _bwd_reference(name, family)
    qd, kd, vd, dd = (t.to(DEV) for t in (qa, ka, v, dctx))
    ctx, lse2 = ops.attn_fwd(qd, kd, vd, A.SCALE, bias_cols=J)
    lib = _lib()
    ratios, runs = {}, []
    try:
        assert lib.svit_attn_debug_set(0, halves) == 0
        for splits in ((0,) if halves == 0 else (0, 3)):
            dqa, dk, dv = ops.attn_bwd(qd, kd, vd, ctx, dd, lse2, A.SCALE, q_splits=splits, bias_cols=J)
            torch.cuda.synchronize()
            runs.append((splits, dqa.cpu(), dk.sum(0).cpu(), dv.sum(0).cpu(), dk.shape[0]))
    finally:
        lib.svit_attn_debug_set(0, 0)
    for splits, dqa, dk, dv, parts in runs:
        tag = "" if halves == 0 else "[q_splits=%d]" % splits
        record_property("parts" + tag, parts)
        if splits == 0 and halves == 0 and name in MULTI_PART_CASES:
            assert parts > 1, "the automatic plan did not cut the query range"
        if splits == 3:
            nqt = (case.Nq + A.QR - 1) // A.QR           # 64-query stages; a part is a whole number of them
            per = -(-nqt // min(3, nqt))
            assert parts == -(-nqt // per)
        got = {"dq_main": dqa[..., :A.HD], "dq_bias": dqa[..., A.HD:A.HD + je], "dk": dk, "dv": dv}
        for t in A.BWD_TENSORS:
            assert bool(torch.isfinite(got[t].float()).all()), t
            ratios[t + tag] = (A.rel_max(got[t], ref[t]), bars[t])
        # columns past 96 + bias_cols: the keys carry zeros there, so does the gradient (svit_hip.h)
        tail = dqa[..., A.HD + je:].float()
        assert tail.numel() == 0 or float(tail.abs().max()) == 0.0
    _report(record_property, ratios, {})
