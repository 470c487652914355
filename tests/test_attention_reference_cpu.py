"""The measure of tests/test_attention_parity_gpu.py has teeth -- proved on the CPU, without looking at a kernel.

For every case of the GPU test (on batch 0 and at most two heads of its inputs) the dense rounding-point emulation
of tests/attn_reference.py gives the `floor` of every tensor (its distance from the float64 reference); the GPU
bar is 3 x floor.  Every applicable mutant -- the reference with one plausible kernel bug -- has to lie at
>= 3 x bar in at least one tensor of at least one input family of the case: an order of magnitude between
"correct" and "wrong".  A mutant judged in one family only (fwd_mutant_applies says why) is not asked for in the
other.  No case may go without its mutants and no mutant without a case that rejects it."""
import functools
import math

import pytest
import torch

from tests import attn_reference as A

F64 = torch.float64
FAMILIES = ("flat", "peaked")
GAP = 3.0                      # a mutant sits at >= GAP x bar = GAP x BAR_FACTOR x floor


@functools.lru_cache(maxsize=None)
def mutant_ratios(name):
    """{mutant: [(metric / bar, family, tensor), ...]} over the families the mutant applies to."""
    case = A.CASE_BY_NAME[name]
    out = {}
    for fam in FAMILIES:
        bars = A.case_bars(name, fam)
        qa, ka, v, d = A.reduced_inputs(case, fam)
        for m in A.FWD_MUTANTS:
            if A.fwd_mutant_applies(m, *case.shape, fam):
                r = A.measure_case(case, fam, A.mutant_fwd_variant(case, m), None, qa, ka, v, d)
                out.setdefault(m, []).extend((r[t] / bars[t], fam, t) for t in r)
        for m in A.BWD_MUTANTS:
            if A.bwd_mutant_applies(m, *case.shape, fam):
                r = A.measure_case(case, fam, A.exact_fwd_variant(case), A.mutant_bwd_variant(case, m), qa, ka, v, d)
                out.setdefault(m, []).extend((r[t] / bars[t], fam, t) for t in A.BWD_TENSORS)
    return out


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_every_applicable_mutant_lies_far_above_the_bar(name, record_property):
    case = A.CASE_BY_NAME[name]
    for fam in FAMILIES:
        floors = A.case_floors(name, fam)
        record_property("floors_" + fam, {t: round(f, 5) for t, f in floors.items()})
        assert set(floors) >= {"lse2", "readout", "dq_main", "dq_bias", "dk", "dv"}
        assert ("attn" in floors) == (fam == "peaked")
        # a floor is a handful of bf16 roundings (2^-9 relative each) of O(1) quantities -- if it were larger the
        # inputs would not make the tensor O(1) and 3 x floor would be no bar at all
        for t, f in floors.items():
            assert 0 < f < 2e-2, (fam, t, f)
        assert floors["lse2"] < A.LSE_BAR / 2      # the fixed lse2 bar leaves a correct kernel room (worst: 20 keys, 3e-4)
    ratios = mutant_ratios(name)
    assert len(ratios) >= (12 if case.Nq >= 8 else 10), sorted(ratios)      # (a single query row has no ragged-row or re-base mutants)
    for m, l in ratios.items():
        top = max(l)
        record_property(m, "%.1f x bar (%s, %s)" % top)
        assert top[0] >= GAP, "%s: mutant %s reaches only %.2f x bar (%s, %s)" % (case, m, *top)


def test_every_mutant_is_rejected_by_some_case():
    seen = set()
    for c in A.CASES:
        seen |= {m for m, l in mutant_ratios(c.name).items() if max(l)[0] >= GAP}
    assert seen == set(A.FWD_MUTANTS) | set(A.BWD_MUTANTS)


def test_cases_name_every_path():
    """forward forms x k-step counts, the backward's four instantiations, tile counts and ragged query tiles."""
    assert {c.form for c in A.CASES} == {"short", "w4", "w8"}
    assert {c.fwd_ksu for c in A.CASES if c.form == "w4"} == {7, 8, 9, 10}
    assert {c.fwd_ksu for c in A.CASES if c.form == "w8"} >= {8, 9, 10}
    assert {c.fwd_ksu for c in A.CASES if c.form == "short"} == {7, 8}
    assert {c.bwd_ksu for c in A.CASES} == {7, 8, 9, 10}
    assert {c.J for c in A.CASES} >= {0, 15, 22, 29, 36}
    assert {c.tiles for c in A.CASES} >= {1, 2, 3, 4, 6, 8, 26}
    assert any(c.Nk <= 32 for c in A.CASES) and any(c.Nk == 64 for c in A.CASES)
    assert any(c.Nq == 1 for c in A.CASES)
    assert any(c.Nq % 128 and c.Nq % 32 and c.Nq > 128 for c in A.CASES)
    for c in A.CASES:
        if c.form == "w8":
            assert c.DA == 160 and (c.Nq + 255) // 256 * c.B * c.h >= 200
    grids = {(c.B, c.h, c.Nq, c.Nk, c.DA, c.J) for c in A.CASES}
    assert {(8, 4, 1633, 457, 128, 22), (8, 4, 1633, 1633, 160, 36), (8, 8, 457, 457, 128, 22),
            (2, 2, 300, 54, 128, 15), (2, 2, 300, 201, 160, 29)} <= grids


def test_written_out_backward_is_autograd():
    case = A.CASE_BY_NAME["frames_J29"]
    for fam in FAMILIES:
        qa, ka, v, dctx = (t.to(F64) for t in A.make_inputs(case, fam, B=1))
        q2, k2, v2, d2 = qa[0, 1], ka[0, 1], v[0, 1], A.ctx_slice(dctx, 0, 1)
        qr, kr, vr = (t.clone().requires_grad_(True) for t in (q2, k2, v2))
        p = ((qr @ kr.t()) * A.LN2).softmax(-1)            # the score in nat: qa . ka^T is in the log2 domain
        (p @ vr).backward(d2)                               # the residual's gradient is not the kernels' business
        ref = A.reference_bwd_2d(q2, k2, v2, d2, case.J)
        je = A.jeff(case.DA, case.J)
        assert A.rel_max(ref["dq_main"], qr.grad[:, :96]) < 1e-11
        assert A.rel_max(ref["dq_bias"], qr.grad[:, 96:96 + je]) < 1e-11
        assert float(ref["dq_tail"].abs().max()) == 0.0     # the keys carry zeros there
        # dk with respect to the UN-scaled keys: ka[:, :96] = scale * log2(e) * k
        assert A.rel_max(ref["dk"], kr.grad[:, :96] * A.KSC) < 1e-11
        assert A.rel_max(ref["dv"], vr.grad) < 1e-11
        attn, res, lse2, P = A.reference_fwd_2d(q2, k2, v2, case.J)
        assert A.rel_max(P, p.detach()) < 1e-12 and A.rel_max(attn, (p @ vr).detach()) < 1e-12
        assert A.rel_max(lse2, torch.logsumexp((q2 @ k2.t()) * A.LN2, -1) * A.LOG2E) < 1e-13
        assert torch.equal(res[1:], q2[1:, :96]) and float(res[0].abs().max()) == 0.0
        whole = A.reference_fwd(qa, ka, v, case.J)          # the [B, h, ...] wrappers are the slices, stacked
        assert all(torch.equal(w[0, 1], s) for w, s in zip(whole, (attn, res, lse2, P)))
        assert torch.equal(A.reference_bwd(qa, ka, v, dctx, case.J)["dk"][0, 1], ref["dk"])


def test_tile_sweep_without_the_bug_is_the_reference():
    """the tile-by-tile online softmax that carries the no-rescale mutant is, with the rescale in place, the dense
    softmax -- and the peaked inputs do make the running maximum jump in it."""
    case = A.CASE_BY_NAME["six_tiles"]
    qa, ka, v, _ = A.reduced_inputs(case, "peaked")
    M, lse2, _ = A._fwd_dense(qa[0, 0], ka[0, 0], case.J)
    Ms, lses, _ = A._fwd_dense(qa[0, 0], ka[0, 0], case.J, mutant="tile_sweep")
    assert A.rel_max(Ms, M) < 1e-12 and A.rel_max(lses, lse2) < 1e-13
    S = qa[0, 0].to(F64) @ ka[0, 0].to(F64).t()
    jumps = set()
    for k, r, _ in A.plants(case.Nq, case.Nk):
        t = k // A.KT
        if t > 0 and float(S[r, k] - S[r, :t * A.KT].max()) > A.RESCALE_THR:
            jumps.add(t)
    assert jumps >= {1, 2, 3, case.Nk // A.KT - 1, case.tiles - 1}


def test_emulated_read_out_is_the_emulated_forward_on_one_hot_values():
    case = A.CASE_BY_NAME["frames_J29"]
    for fam in FAMILIES:
        qa, ka, v, _ = A.reduced_inputs(case, fam)
        q2, k2 = qa[0, 0], ka[0, 0]
        dense, _ = A.emulate_readout_2d(q2, k2)
        for blk in range((case.Nk + A.READOUT_BLOCK - 1) // A.READOUT_BLOCK):
            ctx, res, _ = A.emulate_fwd_2d(q2, k2, A.readout_v(case.Nk, blk))
            got = A.readout_of_ctx(ctx, res, blk, case.Nk)
            assert torch.equal(got, dense[:, blk * 96: blk * 96 + got.shape[1]])


def test_old_measure_accepts_a_wrong_key_tile():
    """The gap this file closes: max-error over max |ref| < 2e-2 and cosine > 0.9999 on the residual-included output
    with flat scores (what tests/test_kernels_gpu.py asserts) accepts V rows rotated inside a key tile and 16 keys
    missing from P V at Nk = 1633, DA = 160 -- the read-out rejects both by more than an order of magnitude."""
    case = A.Case("old_measure", 1, 1, 400, 1633, 160, 36)
    qa, ka, v, _ = A.make_inputs(case, "flat")
    q2, k2, v2 = qa[0, 0], ka[0, 0], v[0, 0]
    attn, res, _, P = A.reference_fwd_2d(q2, k2, v2, case.J)
    ref = attn + res
    _, _, _, floor_read = A.emulated_fwd_variant(q2, k2, v2)
    bar = A.BAR_FACTOR * A.rel_max(floor_read, P)
    for m in ("v_rot_tile", "pv_skip16"):
        a_m, r_m, _, M = A.reference_fwd_2d(q2, k2, v2, case.J, mutant=m)
        got = (a_m + r_m).to(torch.bfloat16).to(F64)        # even rounded once only
        rel = A.rel_max(got, ref)
        cos = float(torch.dot(got.flatten(), ref.flatten()) / (got.norm() * ref.norm()))
        assert rel < 2e-2 and cos > 0.9999, (m, rel, cos)   # the old measure lets it through
        assert A.rel_max(M, P) >= GAP * bar, (m, A.rel_max(M, P), bar)
    assert math.isclose(A.KSC, (96 ** -0.5) * math.log2(math.e))
